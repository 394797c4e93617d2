"""ViTAutoencoder (models/vit.py:66-240) on the HIP kernels: its layers, the hand-scheduled forward and backward, and
the autograd functions for its stand-alone use."""
import math
from typing import Dict

import numpy as np
import torch
import torch.nn as nn

from . import ops
from ._base import _Acts
from ._lib import Event, on_stream
from .tuning import hooks


# ------------------------------------------------------------------------------------ helpers
def _sincos_1d(embed_dim: int, pos: np.ndarray) -> np.ndarray:
    omega = np.arange(embed_dim // 2, dtype=np.float64) / (embed_dim / 2.0)
    omega = 1.0 / 10000 ** omega
    out = np.einsum("m,d->md", pos.reshape(-1).astype(np.float64), omega)
    return np.concatenate([np.sin(out), np.cos(out)], axis=1)


def get_2d_sincos_pos_embed(embed_dim: int, grid_size: int, cls_token: bool = False) -> np.ndarray:
    """tools/utils.py:131-178 (float64; w-coordinate first, CLS row zeros)."""
    gh = np.arange(grid_size, dtype=np.float32)
    gw = np.arange(grid_size, dtype=np.float32)
    grid = np.stack(np.meshgrid(gw, gh), axis=0).reshape(2, 1, grid_size, grid_size)
    emb = np.concatenate([_sincos_1d(embed_dim // 2, grid[0]), _sincos_1d(embed_dim // 2, grid[1])], axis=1)
    if cls_token:
        emb = np.concatenate([np.zeros([1, embed_dim]), emb], axis=0)
    return emb



def _xavier_(t: torch.Tensor, fan_out: int, fan_in: int):
    a = math.sqrt(6.0 / (fan_in + fan_out))
    return t.uniform_(-a, a)


class _Affine(nn.Module):
    """Holder with ``weight`` / ``bias`` Parameters (Linear, LayerNorm, Conv2d-as-proj)."""

    def __init__(self, wshape, bshape):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(wshape))
        self.bias = nn.Parameter(torch.empty(bshape))


class _Attention(nn.Module):          # models/vit.py:16-26
    def __init__(self, dim, heads):
        super().__init__()
        self.num_heads = heads
        self.scale = (dim // heads) ** -0.5
        self.qkv = _Affine((3 * dim, dim), (3 * dim,))
        self.proj = _Affine((dim, dim), (dim,))


class Block(nn.Module):               # models/vit.py:45-57
    def __init__(self, dim, heads, mlp_ratio):
        super().__init__()
        hidden = int(dim * mlp_ratio)
        self.dim, self.heads, self.hidden = dim, heads, hidden
        self.norm1 = _Affine((dim,), (dim,))
        self.attn = _Attention(dim, heads)
        self.norm2 = _Affine((dim,), (dim,))
        self.mlp = nn.ModuleDict({"0": _Affine((hidden, dim), (hidden,)), "2": _Affine((dim, hidden), (dim,))})


class _PatchEmbed(nn.Module):         # timm PatchEmbed attribute surface used by the reference
    def __init__(self, img_size, patch_size, in_chans, embed_dim):
        super().__init__()
        self.patch_size = (patch_size, patch_size)
        self.num_patches = (img_size // patch_size) ** 2
        self.proj = _Affine((embed_dim, in_chans, patch_size, patch_size), (embed_dim,))


def _trainable_order(vit: "ViTAutoencoder"):
    """(state-dict name, parameter) in forward order: weight then bias of each layer adjacent."""
    return [(n, p) for n, p in vit.named_parameters() if p.requires_grad]



# ------------------------------------------------------------------------------------ backward schedule
class _BackwardSchedule:
    """What one backward pass runs where: built by whoever drives the pass (_ViTOwner._backward; the autograd functions
    below, single stream) and handed down to _decoder_bwd / _encoder_bwd / _block_bwd.

    side     the stream of the weight-gradient GEMMs, or None: everything on the launch stream
    pending  one event per block whose side work the main stream has not yet waited for
    jobs     the pass's ops.LayerNormJobs (dgamma / dbeta reductions left to the owner's flushes), or None
    WT       weight -> its transposed copy or None; None when the driver keeps no copies
    G        parameter name (without the owner's prefix) -> its gradient view

    Weight-gradient GEMMs (and their slab reductions) are off the backward's critical path: nothing
    reads dW before the optimizer.  With a side stream they run concurrently with the dX / LayerNorm /
    attention chain and fill its tail rounds and the small-grid gaps.  Ordering: (1) a side GEMM waits
    for the main-stream kernel that produced its dY; (2) the dY buffers (gout / g1 from a ring of five,
    dh / dqkv from two sets) are rewritten two blocks later at the earliest, and the entry of block j
    waits for the side work of block j+2 (_side_join) -- a wait that has normally long been satisfied,
    so the main stream does not stall on the ~15 us cross-stream signalling latency a wait on the
    PREVIOUS block costs; (3) the driver joins the side stream before anything reads the gradients.
    The saved activations the GEMMs read are not written during a backward pass."""
    __slots__ = ("side", "pending", "jobs", "WT", "G")

    def __init__(self, G, side=None, jobs=None, WT=None):
        self.G, self.side, self.jobs, self.WT = G, side, jobs, WT
        self.pending = []

    def _event(self):
        """A pooled library event: the next of Event.POOL in turn, so each record of a pass has an event of its own until
        POOL - 1 further pooled calls have been made.  Re-recording one is safe once the waits on its previous record are
        enqueued; the pool is far longer than the few events whose wait is deferred by a block or two (_side_join)."""
        return Event.pooled()

    def _dx(self, dy, weight, dx, **kw):
        """dX = dY W: from the transposed weight copy when the driver keeps one (NT kernel family)."""
        wt = self.WT(weight) if self.WT is not None else None
        if wt is not None:
            return ops.linear_bwd_input_t(dy, wt, dx, **kw)
        return ops.linear_bwd_input(dy, weight, dx, **kw)

    def _dw(self, dy, x, gw, gb):
        side = self.side
        if side is None:
            return ops.linear_bwd_weight(dy, x, gw, gb)
        self._event().record().wait(side)       # recorded on the main (current) stream: dy is final here
        with on_stream(side):
            ops.linear_bwd_weight(dy, x, gw, gb)

    def _side_join(self, keep: int = 1):
        """Main stream waits for the side work of all but the `keep` most recent blocks."""
        while len(self.pending) > keep:
            self.pending.pop(0).wait()

    def _side_mark(self):
        if self.side is not None:
            self.pending.append(self._event().record(self.side))

    def _ln_bwd(self, dy, x, mean, rstd, gamma, resid, dx, dgamma, dbeta):
        """LayerNorm backward; with a job list the dgamma / dbeta reduction is left to the driver's next flush."""
        if self.jobs is not None and ops.layernorm_bwd_deferrable(*x.shape):
            return self.jobs.bwd(dy, x, mean, rstd, gamma, resid, dx, dgamma, dbeta)
        return ops.layernorm_bwd(dy, x, mean, rstd, gamma, resid, dx, dgamma, dbeta)

    def _dx_ln(self, dy, weight, da, x, mean, rstd, gamma, resid, dx, dgamma, dbeta):
        """dX of a Linear, then the backward of the LayerNorm whose output fed it: one launch (the LayerNorm backward in
        the GEMM's epilogue, the product never stored) where the transposed weight copy, the shape and the GEMM mode allow
        it (hooks.ln_bwd_fused), else the GEMM into the scratch `da` and _ln_bwd.  Same dX bits either way."""
        wt = self.WT(weight) if (self.WT is not None and hooks.ln_bwd_fused) else None
        if wt is not None and ops.linear_bwd_input_ln_supported(dy.shape[0], dy.shape[1], x.shape[1]):
            if self.jobs is not None:
                return self.jobs.bwd_linear_fused(dy, wt, x, mean, rstd, gamma, resid, dx, dgamma, dbeta)
            return ops.linear_bwd_input_ln(dy, wt, x, mean, rstd, gamma, resid, dx, dgamma, dbeta)
        self._dx(dy, weight, da)
        return self._ln_bwd(da, x, mean, rstd, gamma, resid, dx, dgamma, dbeta)


# ------------------------------------------------------------------------------------ ViT autoencoder
class ViTAutoencoder(nn.Module):
    """MAE-style unmasked ViT autoencoder (models/vit.py:66-240); compute on the HIP kernels."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768, depth=12, num_heads=12,
                 decoder_embed_dim=512, decoder_depth=8, decoder_num_heads=16, mlp_ratio=4.0, norm_layer=None,
                 norm_pix_loss=False, eps: float = 1e-6):
        super().__init__()
        self.img_size, self.in_chans, self.eps = img_size, in_chans, eps
        self.embed_dim, self.decoder_embed_dim = embed_dim, decoder_embed_dim
        self.num_heads, self.decoder_num_heads = num_heads, decoder_num_heads
        self.patch_embed = _PatchEmbed(img_size, patch_size, in_chans, embed_dim)
        n = self.patch_embed.num_patches
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, n + 1, embed_dim), requires_grad=False)
        self.blocks = nn.ModuleList([Block(embed_dim, num_heads, mlp_ratio) for _ in range(depth)])
        self.norm = _Affine((embed_dim,), (embed_dim,))
        self.decoder_embed = _Affine((decoder_embed_dim, embed_dim), (decoder_embed_dim,))
        self.decoder_pos_embed = nn.Parameter(torch.zeros(1, n + 1, decoder_embed_dim), requires_grad=False)
        self.decoder_blocks = nn.ModuleList([Block(decoder_embed_dim, decoder_num_heads, mlp_ratio)
                                             for _ in range(decoder_depth)])
        self.decoder_norm = _Affine((decoder_embed_dim,), (decoder_embed_dim,))
        self.decoder_pred = _Affine((patch_size ** 2 * in_chans, decoder_embed_dim), (patch_size ** 2 * in_chans,))
        self.initialize_weights()
        self._acts: Dict[int, _Acts] = {}
        self._dec_only = None       # the decoder-only buffer set of decode_prototypes (_decoder_buffers_for)
        self._fwd_side = None       # the stream the last forward ran its second chain on; None: it was not split

    # -- init: same distributions as vit.py:100-125 ------------------------------------------
    def initialize_weights(self):
        g = int(self.patch_embed.num_patches ** 0.5)
        with torch.no_grad():
            self.pos_embed.copy_(torch.from_numpy(get_2d_sincos_pos_embed(self.embed_dim, g, True)).float().unsqueeze(0))
            self.decoder_pos_embed.copy_(
                torch.from_numpy(get_2d_sincos_pos_embed(self.decoder_embed_dim, g, True)).float().unsqueeze(0))
            w = self.patch_embed.proj.weight
            _xavier_(w, w.shape[0], w[0].numel())
            bound = 1.0 / math.sqrt(w[0].numel())                    # Conv2d default bias init (untouched by _init_weights)
            self.patch_embed.proj.bias.uniform_(-bound, bound)
            self.cls_token.normal_(std=0.02)
            for name, m in self.named_modules():
                if not isinstance(m, _Affine) or m is self.patch_embed.proj:
                    continue
                if m.weight.ndim == 2:                                # nn.Linear: xavier_uniform / zero bias
                    _xavier_(m.weight, m.weight.shape[0], m.weight.shape[1])
                    m.bias.zero_()
                else:                                                 # nn.LayerNorm
                    m.weight.fill_(1.0)
                    m.bias.zero_()

    # -- pure index shuffles kept for API parity (torch view ops: no arithmetic) -------------
    def patchify(self, imgs):
        p = self.patch_embed.patch_size[0]
        assert imgs.shape[2] == imgs.shape[3] and imgs.shape[2] % p == 0
        h = w = imgs.shape[2] // p
        c = imgs.shape[1]
        x = imgs.reshape(imgs.shape[0], c, h, p, w, p)
        return torch.einsum("nchpwq->nhwpqc", x).reshape(imgs.shape[0], h * w, p ** 2 * c)

    def unpatchify(self, x):
        p = self.patch_embed.patch_size[0]
        h = w = int(x.shape[1] ** 0.5)
        assert h * w == x.shape[1]
        c = x.shape[2] // (p * p)
        x = x.reshape(x.shape[0], h, w, p, p, c)
        return torch.einsum("nhwpqc->nchpwq", x).reshape(x.shape[0], c, h * p, w * p)

    # -- buffers ------------------------------------------------------------------------------
    @staticmethod
    def _layer_acts(f, B: int, N: int, dim: int, heads: int, hidden: int) -> _Acts:
        """The forward tensors of one block for B images of N tokens."""
        T = B * N
        L = _Acts()
        L.a1, L.mean1, L.rstd1 = f(T, dim), f(T), f(T)
        L.qkv, L.ao, L.lse = f(T, 3 * dim), f(T, dim), f(B, heads, N)
        L.x1, L.a2, L.mean2, L.rstd2 = f(T, dim), f(T, dim), f(T), f(T)
        L.hpre, L.hact, L.x2 = f(T, hidden), f(T, hidden), f(T, dim)
        return L

    def _decoder_buffers_for(self, B: int, device) -> _Acts:
        """What _decode needs for B token sequences and nothing else: the input tokens (xe), dec0, the decoder blocks'
        forward tensors, dn and pred -- no encoder layer, no backward temporary (about a tenth of _buffers_for(B)).
        One set is kept, apart from self._acts: decoding prototypes between epochs neither evicts nor touches the
        training batch's buffers."""
        d = self._dec_only
        if d is not None and d.B == B and d.device == device:
            return d
        E, DE = self.embed_dim, self.decoder_embed_dim
        N = self.patch_embed.num_patches + 1
        T = B * N
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=device)   # noqa: E731
        self._dec_only = None                                                 # the old set goes before the new one comes
        d = _Acts()
        d.device, d.B, d.N, d.T = device, B, N, T
        d.xe = torch.zeros(T, E, dtype=torch.float32, device=device)          # the CLS rows stay zero (decode_prototype)
        d.dec0 = f(T, DE)
        d.dec = [self._layer_acts(f, B, N, DE, self.decoder_num_heads, b.hidden) for b in self.decoder_blocks]
        d.dn, d.mean_d, d.rstd_d = f(T, DE), f(T), f(T)
        d.pred = f(T, self.patch_embed.patch_size[0] ** 2 * self.in_chans)
        self._dec_only = d
        return d

    def _buffers_for(self, B: int, device) -> _Acts:
        a = self._acts.get(B)
        if a is not None and a.device == device:
            return a
        E, DE = self.embed_dim, self.decoder_embed_dim
        n = self.patch_embed.num_patches
        N, T = n + 1, B * (n + 1)
        p = self.patch_embed.patch_size[0]
        pd = p * p * self.in_chans
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=device)   # noqa: E731
        a = _Acts()
        a.device, a.B, a.N, a.T = device, B, N, T
        a.xp = f(B * n, pd)
        a.tok0 = f(T, E)
        layer = lambda dim, heads, hidden: self._layer_acts(f, B, N, dim, heads, hidden)   # noqa: E731
        a.enc = [layer(E, self.num_heads, b.hidden) for b in self.blocks]
        a.xe, a.mean_e, a.rstd_e = f(T, E), f(T), f(T)
        a.dec0 = f(T, DE)
        a.dec = [layer(DE, self.decoder_num_heads, b.hidden) for b in self.decoder_blocks]
        a.dn, a.mean_d, a.rstd_d = f(T, DE), f(T), f(T)
        a.pred = f(T, pd)
        # backward temporaries (shared by all layers; sized for the wider of encoder / decoder)
        W = max(E, DE)
        Hd = max([b.hidden for b in self.blocks] + [b.hidden for b in self.decoder_blocks])
        # five rotating [T, dim] gradient buffers and two dh / dqkv sets: a buffer the side stream reads
        # in one block is rewritten two blocks later at the earliest (see _side_join)
        a.g = [f(T * W) for _ in range(5)]
        a.dh2, a.dqkv2, a.da = [f(T * Hd), f(T * Hd)], [f(T * 3 * W), f(T * 3 * W)], f(T * W)
        a.delta = f(B * max(self.num_heads, self.decoder_num_heads) * N)
        a.dpred = f(T, pd)
        a.d_xe = f(T, E)
        a.version = 0            # bumped whenever the activation buffers are rewritten (staleness guard of the autograd bridges)
        # at most two batch sizes stay allocated (the training batch and, e.g., an evaluation batch; decode_prototypes has its own decoder-only set)
        keep = list(self._acts.items())[-1:]
        self._acts = dict(keep + [(B, a)])
        return a

    # -- forward ------------------------------------------------------------------------------
    def _block_fwd(self, blk: Block, L: _Acts, x_in: torch.Tensor, B: int, N: int):
        T = B * N
        ops.layernorm_fwd(x_in, blk.norm1.weight, blk.norm1.bias, L.a1, L.mean1, L.rstd1, self.eps)
        ops.linear_fwd(L.a1, blk.attn.qkv.weight, blk.attn.qkv.bias, L.qkv)
        ops.attention_fwd(L.qkv, L.ao, L.lse, B, N, blk.heads, blk.dim // blk.heads)
        ops.linear_residual_fwd(L.ao, blk.attn.proj.weight, blk.attn.proj.bias, x_in, T, L.x1)
        ops.layernorm_fwd(L.x1, blk.norm2.weight, blk.norm2.bias, L.a2, L.mean2, L.rstd2, self.eps)
        ops.linear_gelu_fwd(L.a2, blk.mlp["0"].weight, blk.mlp["0"].bias, L.hpre, L.hact)
        ops.linear_residual_fwd(L.hact, blk.mlp["2"].weight, blk.mlp["2"].bias, L.x1, T, L.x2)
        return L.x2

    def _encode(self, x: torch.Tensor, a: _Acts, side=None):
        cur = self._encode_trunk(x, a, len(self.blocks), side)
        ops.layernorm_fwd(cur, self.norm.weight, self.norm.bias, a.xe, a.mean_e, a.rstd_e, self.eps)
        return a.xe

    def _encode_trunk(self, x: torch.Tensor, a: _Acts, depth: int, side=None):
        """Patch embedding and encoder blocks [0, depth) -> the output of block depth - 1 ([T, E]; the tokens when 0).
        `side`: a stream to borrow for the second chain of a split forward (None: one the ViT creates and keeps)."""
        E = self.embed_dim
        p = self.patch_embed.patch_size[0]
        a.version += 1
        ops.patch_embed_fwd(x, self.patch_embed.proj.weight.view(E, -1), self.patch_embed.proj.bias, self.pos_embed[0],
                            self.cls_token.view(E), a.tok0, a.xp, p)
        cur = a.tok0
        if cur.is_cuda and a.B % 2 == 0 and a.B >= 64 and hooks.fwd_split:
            # the owner (ViTSOM) lends the stream its backward uses for the weight gradients -- idle during
            # the forward; a stream of its own would compete for the few hardware queues of the process
            # (measured: erratic, sometimes slower than one chain)
            if side is None or side.device != cur.device:
                side = self._fwd_side
                if side is None or side.device != cur.device:
                    side = torch.cuda.Stream(device=cur.device)
        else:
            side = None
        self._fwd_side = side
        if side is not None:
            # The forward is one dependent chain per image: the two halves of the batch run as two chains
            # on two streams (row-sliced views of the same buffers, so the results are the same bits and
            # the backward sees one batch); staggered against each other, one chain's latency-bound
            # kernels (attention, LayerNorm) run under the other's GEMMs.
            Bh, Th = a.B // 2, a.T // 2
            cuts = a.__dict__.get("_enc_halves")
            if cuts is None:
                def cut(L, h):
                    Lh = _Acts()
                    for k, v in L.__dict__.items():
                        Lh.__dict__[k] = v[h * Bh:(h + 1) * Bh] if k == "lse" else v[h * Th:(h + 1) * Th]
                    return Lh
                cuts = a.__dict__["_enc_halves"] = [[cut(L, h) for L in a.enc] for h in (0, 1)]
            Event.pooled().record().wait(side)
            # All blocks by default (A/B in one process, round 2: 0 / 6 / 12 of 12 blocks split -> 11.77 / 11.81 /
            # 11.68 ms per step; round 1 kept it to half because the f32-MFMA BMU pass ran slower right after a dense
            # forward -- the bf16 BMU pass does not).
            nsplit = len(self.blocks) if hooks.fwd_split_blocks is None else int(hooks.fwd_split_blocks)
            nsplit = max(0, min(nsplit, depth))
            # enqueue the two chains alternately, block by block: the host feeds both streams at the same pace (all
            # of chain 0 first left the second stream idle for the ~0.7 ms the host needs to enqueue six blocks)
            c0, c1 = a.tok0[:Th], a.tok0[Th:]
            for i in range(nsplit):
                c0 = self._block_fwd(self.blocks[i], cuts[0][i], c0, Bh, a.N)
                with on_stream(side):
                    c1 = self._block_fwd(self.blocks[i], cuts[1][i], c1, Bh, a.N)
            Event.pooled().record(side).wait()
            cur = a.enc[nsplit - 1].x2 if nsplit > 0 else a.tok0
            for blk, L in zip(self.blocks[nsplit:depth], a.enc[nsplit:depth]):
                cur = self._block_fwd(blk, L, cur, a.B, a.N)
        else:
            for blk, L in zip(self.blocks[:depth], a.enc[:depth]):
                cur = self._block_fwd(blk, L, cur, a.B, a.N)
        return cur

    def _decode(self, a: _Acts):
        ops.linear_residual_fwd(a.xe, self.decoder_embed.weight, self.decoder_embed.bias, self.decoder_pos_embed[0],
                                a.N, a.dec0)
        cur = a.dec0
        for blk, L in zip(self.decoder_blocks, a.dec):
            cur = self._block_fwd(blk, L, cur, a.B, a.N)
        ops.layernorm_fwd(cur, self.decoder_norm.weight, self.decoder_norm.bias, a.dn, a.mean_d, a.rstd_d, self.eps)
        ops.linear_fwd(a.dn, self.decoder_pred.weight, self.decoder_pred.bias, a.pred)
        return a.pred

    def _check_input(self, x):
        if x.dim() != 4 or x.shape[1] != self.in_chans or x.shape[2] != self.img_size or x.shape[3] != self.img_size:
            raise ValueError(f"expected input [B,{self.in_chans},{self.img_size},{self.img_size}], got {tuple(x.shape)}")
        return x.contiguous().float()

    def _attention_maps(self, blocks, layers, a: _Acts):
        """[B, heads, N, N] softmax probabilities of every block (vit.py:33-34,41-42), formed from the saved qkv / lse."""
        out = []
        for blk, L in zip(blocks, layers):
            probs = torch.empty(a.B, blk.heads, a.N, a.N, dtype=torch.float32, device=a.device)
            ops.attention_probs(L.qkv, L.lse, probs, a.B, a.N, blk.heads, blk.dim // blk.heads)
            out.append(probs)
        return out

    # -- attention rollout (attention_rollout.py) -----------------------------------------------------
    def _rollout(self, a: _Acts, query="cls", head_fusion="mean", residual=0.5, start_layer=0, _check_sign=True):
        """The rollout [B, N] from the buffers `a` that a full encoder forward has just filled: launches only, no second
        encoder pass (evaluate_attention calls it right after predict())."""
        from .attention_rollout import rollout_from_acts
        return rollout_from_acts(self, a, query, head_fusion, residual, start_layer, "attention_rollout", _check_sign)

    @torch.no_grad()
    def attention_rollout(self, x, query="cls", head_fusion="mean", residual=0.5, start_layer=0, _check_sign=True):
        """Attention rollout of the encoder for the images x -> [B, N] float32, each row summing to the query's weight: how much
        of the query's attention, folded through blocks start_layer .. L - 1 with `residual` of the identity mixed into every
        block, ends on each input token (column 0 is CLS; patch_map() reshapes the rest to the patch grid).
        query: 'cls'; 'patches' (1 / n on each patch token, 0 on CLS); an int token index; or a non-negative float tensor of
        shape [N] or [B, N].  head_fusion: 'mean', 'max' or 'min' over the heads.  residual in [0, 1); start_layer in [0, L).
        Runs the encoder in full under no_grad, then one kernel pair per block on the saved qkv; no N x N matrix is formed."""
        from .attention_rollout import check_arguments
        check_arguments("attention_rollout", head_fusion, residual, start_layer, len(self.blocks))
        x = self._check_input(x)
        if not x.is_cuda:
            raise ValueError("attention_rollout: input must live on the MI355X (there is no CPU path)")
        a = self._buffers_for(x.shape[0], x.device)
        self._encode(x, a)
        return self._rollout(a, query, head_fusion, residual, start_layer, _check_sign)

    def patch_map(self, r):
        """Columns 1: of a rollout [B, N] as [B, gh, gw] on the patch grid."""
        from .attention_rollout import patch_map
        return patch_map(self, r)

    def _wants_grad(self, *inputs):
        return torch.is_grad_enabled() and (any(p.requires_grad for _, p in _trainable_order(self))
                                            or any(t.requires_grad for t in inputs))

    def forward_features(self, x, return_attns=False):
        """vit.py:155-179 -> (cls_token_out [B,E], attns | None); differentiable w.r.t. the encoder parameters
        under autograd (``_VitForwardFn`` in features mode)."""
        x = self._check_input(x)
        if self._wants_grad(x):
            cls = _VitForwardFn.apply(x, self, "features", *[p for _, p in _trainable_order(self)])
            a = self._acts[x.shape[0]]
        else:
            with torch.no_grad():
                a = self._buffers_for(x.shape[0], x.device)
                cls = self._encode(x, a).view(a.B, a.N, self.embed_dim)[:, 0].clone()
        with torch.no_grad():
            attns = self._attention_maps(self.blocks, a.enc, a) if return_attns else None
        return cls, attns

    def forward(self, x, return_attns=False):
        """vit.py:202-240 -> (cls_token_out [B,E], patch_tokens_out [B,n,E], recon_img [B,C,S,S]) (+ the encoder's
        attention maps as a fourth element when return_attns, vit.py:238-239).  With autograd enabled the three
        outputs are differentiable w.r.t. every trainable parameter (``_VitForwardFn``: the stand-alone use of the
        sub-module; the fused training step of ViTSOM does not go through here)."""
        x = self._check_input(x)
        if self._wants_grad(x):
            out = _VitForwardFn.apply(x, self, "full", *[p for _, p in _trainable_order(self)])
        else:
            with torch.no_grad():
                out = self._forward_impl(x)
        if return_attns:
            with torch.no_grad():
                a = self._acts[x.shape[0]]
                return tuple(out) + (self._attention_maps(self.blocks, a.enc, a),)
        return out

    def _forward_impl(self, x):
        a = self._buffers_for(x.shape[0], x.device)
        xe = self._encode(x, a).view(a.B, a.N, self.embed_dim)
        self._decode(a)
        recon = torch.empty_like(x)
        scratch1 = torch.empty(1, dtype=torch.float32, device=x.device)
        ops.l1_unpatchify(a.pred, x, scratch1, recon=recon, p=self.patch_embed.patch_size[0])
        return xe[:, 0].clone(), xe[:, 1:].clone(), recon

    def forward_decoder(self, x, return_attn=False):
        """vit.py:182-200 -> (decoded_patches [B,n,p*p*C], attns | None): decoder_embed -> + decoder_pos_embed -> decoder
        blocks -> decoder_norm -> decoder_pred[:, 1:] on an ARBITRARY token tensor x [B,n+1,E] (tools/evaluation.py:209-222
        feeds a prototype behind a zero CLS row).  The reference's return_attn=False branch assigns the block's
        (x, attn) tuple to `decoded` (vit.py:195) and fails at decoder_norm; this is what it means.  Differentiable
        w.r.t. the decoder parameters and x under autograd."""
        n, E = self.patch_embed.num_patches, self.embed_dim
        if x.dim() != 3 or x.shape[1] != n + 1 or x.shape[2] != E:
            raise ValueError(f"forward_decoder: expected tokens [B,{n + 1},{E}], got {tuple(x.shape)}")
        if not x.is_cuda:
            raise ValueError("forward_decoder: input must live on the MI355X (there is no CPU path)")
        x = x.float()
        if self._wants_grad(x):
            patches = _VitDecoderFn.apply(x, self, *[p for _, p in _trainable_order(self)])
            a = self._acts[x.shape[0]]
        else:
            with torch.no_grad():
                a = self._decode_tokens(x)
                patches = a.pred.view(a.B, a.N, -1)[:, 1:].clone()
        with torch.no_grad():
            attns = self._attention_maps(self.decoder_blocks, a.dec, a) if return_attn else None
        return patches, attns

    def _decode_tokens(self, x):
        a = self._buffers_for(x.shape[0], x.device)
        a.version += 1
        a.xe.view(a.B, a.N, self.embed_dim).copy_(x)
        self._decode(a)
        return a

    @torch.no_grad()
    def decode_prototypes(self, prototypes, map_size=None, chunk: int = 512, gap: int = 1, want_canvas: bool = True):
        """tools/evaluation.py:209-222 for a whole map at once: every row of `prototypes` [K, n*E] behind a zero CLS
        row -> forward_decoder -> unpatchify, `chunk` prototypes per decoder pass, through the decoder-only buffers
        (self._acts and the launch tapes tied to it are not touched; no autograd).  Returns (images [K, C, S, S] float32,
        canvas): the uint8 RGB mosaic of the map_size = (rows, cols) grid with `gap` white pixels between cells
        (ops.proto_mosaic), or None when not wanted.  Both are fresh device tensors."""
        n, E = self.patch_embed.num_patches, self.embed_dim
        if prototypes.dim() != 2 or prototypes.shape[1] != n * E:
            raise ValueError(f"decode_prototypes: expected prototypes [K,{n * E}], got {tuple(prototypes.shape)}")
        if not prototypes.is_cuda:
            raise ValueError("decode_prototypes: prototypes must live on the MI355X (there is no CPU path)")
        if ops.tape_recording():
            raise RuntimeError("decode_prototypes: called while a launch tape is being recorded")
        K, C, S, p = prototypes.shape[0], self.in_chans, self.img_size, self.patch_embed.patch_size[0]
        rows, cols = (1, K) if map_size is None else (int(map_size[0]), int(map_size[1]))
        if rows * cols != K or gap < 0:
            raise ValueError(f"decode_prototypes: a {rows} x {cols} map with gap {gap} does not hold {K} prototypes")
        dev = prototypes.device
        B = max(1, min(int(chunk), K))
        d = self._decoder_buffers_for(B, dev)
        images = torch.empty(K, C, S, S, dtype=torch.float32, device=dev)
        canvas = None
        if want_canvas:
            canvas = torch.empty(rows * S + (rows - 1) * gap, cols * S + (cols - 1) * gap, 3, dtype=torch.uint8, device=dev)
        tokens = d.xe.view(B, n + 1, E)
        for k0 in range(0, K, B):
            m = min(B, K - k0)
            # a short last chunk runs at the full row count (one GEMM plan per call); its spare rows hold the previous
            # chunk's tokens and nobody reads their output
            tokens[:m, 1:].copy_(prototypes[k0:k0 + m].detach().view(m, n, E))
            self._decode(d)
            ops.proto_mosaic(d.pred[:m * (n + 1)], n, p, C, k0, (rows, cols), images=images, canvas=canvas, gap=gap)
        return images, canvas

    # -- backward (the streams, events and deferred reductions of a pass: _BackwardSchedule) ---
    def _block_bwd(self, blk: Block, L: _Acts, x_in, gout, a: _Acts, sched: _BackwardSchedule, prefix: str, bufs, parity: int = 0):
        """gout: gradient w.r.t. the block output [T,dim]; returns gradient w.r.t. x_in (in bufs)."""
        T, dim, hid = a.T, blk.dim, blk.hidden
        G = sched.G
        sched._side_join(keep=1)           # side work of the block before the previous one must be done
        g1, g0 = bufs
        dh = a.dh2[parity][:T * hid].view(T, hid)
        da = a.da[:T * dim].view(T, dim)
        dqkv = a.dqkv2[parity][:T * 3 * dim].view(T, 3 * dim)
        sched._dw(gout, L.hact, G(f"{prefix}.mlp.2.weight"), G(f"{prefix}.mlp.2.bias"))
        sched._dx(gout, blk.mlp["2"].weight, dh, gelu_grad=L.hpre)
        sched._dw(dh, L.a2, G(f"{prefix}.mlp.0.weight"), G(f"{prefix}.mlp.0.bias"))
        sched._dx_ln(dh, blk.mlp["0"].weight, da, L.x1, L.mean2, L.rstd2, blk.norm2.weight, gout, g1,
                    G(f"{prefix}.norm2.weight"), G(f"{prefix}.norm2.bias"))
        sched._dw(g1, L.ao, G(f"{prefix}.attn.proj.weight"), G(f"{prefix}.attn.proj.bias"))
        sched._dx(g1, blk.attn.proj.weight, da)
        ops.attention_bwd(L.qkv, L.ao, da, L.lse, dqkv, a.delta, a.B, a.N, blk.heads, dim // blk.heads)
        sched._dw(dqkv, L.a1, G(f"{prefix}.attn.qkv.weight"), G(f"{prefix}.attn.qkv.bias"))
        sched._dx_ln(dqkv, blk.attn.qkv.weight, da, x_in, L.mean1, L.rstd1, blk.norm1.weight, g1, g0,
                    G(f"{prefix}.norm1.weight"), G(f"{prefix}.norm1.bias"))
        sched._side_mark()
        return g0

    def _views(self, a: _Acts, dim: int):
        return [b[:a.T * dim].view(a.T, dim) for b in a.g]

    def _decoder_bwd(self, a: _Acts, sched: _BackwardSchedule, before_dxe=None):
        """a.dpred holds dL/dpred; writes decoder grads and dL/d(xe) into a.d_xe -- overwriting it, or,
        when `before_dxe` is given, calling it and then ADDING to what a.d_xe holds (the SOM input
        gradient written concurrently on another stream; `before_dxe` waits for it)."""
        G, DE = sched.G, self.decoder_embed_dim
        ring = self._views(a, DE)
        gA = ring[0]
        ops.linear_bwd_weight(a.dpred, a.dn, G("decoder_pred.weight"), G("decoder_pred.bias"))
        dn_grad = a.da[:a.T * DE].view(a.T, DE)
        sched._dx(a.dpred, self.decoder_pred.weight, dn_grad)
        x_last = a.dec[-1].x2 if a.dec else a.dec0
        sched._ln_bwd(dn_grad, x_last, a.mean_d, a.rstd_d, self.decoder_norm.weight, None, gA,
                      G("decoder_norm.weight"), G("decoder_norm.bias"))
        gout, pos = gA, 0
        for j, i in enumerate(reversed(range(len(self.decoder_blocks)))):
            x_in = a.dec[i - 1].x2 if i > 0 else a.dec0
            bufs = [ring[(pos + 1) % 5], ring[(pos + 2) % 5]]
            gout = self._block_bwd(self.decoder_blocks[i], a.dec[i], x_in, gout, a, sched, f"decoder_blocks.{i}", bufs, j & 1)
            pos = (pos + 2) % 5
        ops.linear_bwd_weight(gout, a.xe, G("decoder_embed.weight"), G("decoder_embed.bias"))
        if before_dxe is not None:
            before_dxe()
        sched._dx(gout, self.decoder_embed.weight, a.d_xe, accumulate=before_dxe is not None)

    def _encoder_bwd(self, a: _Acts, sched: _BackwardSchedule, on_block=None, depth=None):
        """a.d_xe holds dL/d(xe); writes every encoder gradient.  on_block(i) is called once block i's
        backward (main chain and weight-gradient side work) has been enqueued.  With `depth` given, the caller has
        already run the final norm and blocks [depth, D) and left dL/d(output of block depth - 1) in the first
        [T, E] gradient buffer (self._views(a, E)[0]); only blocks [0, depth) and the patch embedding run."""
        sched._side_join(keep=0)           # the decoder's blocks may still be reading the shared buffers
        G, E = sched.G, self.embed_dim
        ring = self._views(a, E)
        gA = ring[0]
        if depth is None:
            depth = len(self.blocks)
            x_last = a.enc[-1].x2 if a.enc else a.tok0
            sched._ln_bwd(a.d_xe, x_last, a.mean_e, a.rstd_e, self.norm.weight, None, gA, G("norm.weight"), G("norm.bias"))
        gout, pos = gA, 0
        for j, i in enumerate(reversed(range(depth))):
            x_in = a.enc[i - 1].x2 if i > 0 else a.tok0
            bufs = [ring[(pos + 1) % 5], ring[(pos + 2) % 5]]
            gout = self._block_bwd(self.blocks[i], a.enc[i], x_in, gout, a, sched, f"blocks.{i}", bufs, j & 1)
            pos = (pos + 2) % 5
            if on_block is not None:
                on_block(i)
        p = self.patch_embed.patch_size[0]
        ops.patch_embed_bwd(gout, a.xp, G("patch_embed.proj.weight").view(E, -1), G("patch_embed.proj.bias"),
                            G("cls_token").view(E), a.B, self.in_chans, self.img_size, p, E)


# ------------------------------------------------------------------------------------ per-module autograd
def _stale(vit, B, version):
    a = vit._acts.get(B)
    if a is None or a.version != version:
        raise RuntimeError("ViTAutoencoder: backward() after the activation buffers of this batch size were rewritten "
                           "(another forward / training_step / validation_step ran in between); call backward first")
    return a


class _VitForwardFn(torch.autograd.Function):
    """ViTAutoencoder.forward / forward_features for stand-alone use under autograd (models/vit.py:155-179,202-240):
    forward = the HIP forward kernels; backward = the same HIP backward kernels the fused step uses, fed with the
    upstream gradients of (cls, patches, recon) -- or of cls alone in "features" mode.  The gradient w.r.t. the input
    IMAGE is not produced (nothing on the path needs it): an input that requires grad is refused."""

    @staticmethod
    def forward(ctx, x, vit, mode, *params):
        if x.requires_grad:
            raise RuntimeError("ViTAutoencoder: the gradient w.r.t. the input image is not implemented")
        ctx.vit, ctx.B, ctx.mode = vit, x.shape[0], mode
        with torch.no_grad():
            if mode == "features":
                a = vit._buffers_for(x.shape[0], x.device)
                out = vit._encode(x, a).view(a.B, a.N, vit.embed_dim)[:, 0].clone()
            else:
                out = vit._forward_impl(x)
        ctx.version = vit._acts[ctx.B].version
        return out

    @staticmethod
    def backward(ctx, g_cls, g_patches=None, g_recon=None):
        vit = ctx.vit
        a = _stale(vit, ctx.B, ctx.version)
        named = _trainable_order(vit)
        with torch.no_grad():
            grads = {n: torch.zeros_like(p) for n, p in named}
            sched = _BackwardSchedule(grads.__getitem__)          # single stream: this is not the fused step
            E, N, B = vit.embed_dim, a.N, a.B
            if g_recon is not None:
                dp = a.dpred.view(B, N, -1)
                dp[:, 0].zero_()
                dp[:, 1:].copy_(vit.patchify(g_recon.float()))
                vit._decoder_bwd(a, sched)
            else:
                a.d_xe.zero_()
            d = a.d_xe.view(B, N, E)
            if g_cls is not None:
                d[:, 0].add_(g_cls)
            if g_patches is not None:
                d[:, 1:].add_(g_patches)
            vit._encoder_bwd(a, sched)
        return (None, None, None) + tuple(grads[n] for n, _ in named)


class _VitDecoderFn(torch.autograd.Function):
    """ViTAutoencoder.forward_decoder under autograd (models/vit.py:182-200): gradients to the decoder parameters and
    to the token tensor it was fed."""

    @staticmethod
    def forward(ctx, x, vit, *params):
        ctx.vit, ctx.B = vit, x.shape[0]
        with torch.no_grad():
            a = vit._decode_tokens(x)
            out = a.pred.view(a.B, a.N, -1)[:, 1:].clone()
        ctx.version = a.version
        return out

    @staticmethod
    def backward(ctx, g_patches):
        vit = ctx.vit
        a = _stale(vit, ctx.B, ctx.version)
        named = _trainable_order(vit)
        with torch.no_grad():
            grads = {n: torch.zeros_like(p) for n, p in named}
            dp = a.dpred.view(a.B, a.N, -1)
            dp[:, 0].zero_()
            dp[:, 1:].copy_(g_patches.float())
            vit._decoder_bwd(a, _BackwardSchedule(grads.__getitem__))
            gx = a.d_xe.view(a.B, a.N, vit.embed_dim).clone()
        return (gx, None) + tuple(grads[n] for n, _ in named)
