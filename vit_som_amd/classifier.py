"""ViTClassifier (models/vit.py:243-340): the plain ViT baseline the paper measures ViT-SOM against, on the HIP kernels.

The module surface is the reference's: ``model`` (a ViTAutoencoder, decoder included and never run), ``cls_head``,
``state_dict`` keys ``model.*`` / ``cls_head.*``, CrossEntropyLoss WITHOUT label smoothing (vit.py:279: the configs'
``optimizer.smoothing`` is not read for this model), the same optimizer groups and schedule.  Parameters live in one
flat arena (step.py _ArenaOwner), like ViTSOM's.

The training step is encoder-only and prunes the last encoder block: forward_features reads only norm(x)[:, 0]
(vit.py:174-179), so in the last block only the CLS row's output is ever used.  K and V are still projected for every
token, but the query, the attention (one query per image and head: ops.attention_q1_*), proj, norm2, the MLP and the
final LayerNorm run on the B CLS rows only.  ``tuning.hooks.cls_prune = False`` runs the last block in full instead.
There is no CPU path and no launch tape: the step is host-driven.
"""
import math
from typing import Dict, Optional

import torch

from . import ops
from ._base import _HAVE_PL, _Acts, _Base
from ._lib import stream_wait_stream
from .arena import ParamArena
from .model import _LOSS_RING, _STEP_STREAMS, ViTSOM
from .optim import FusedAdamW, param_groups_lrd
from .step import _ArenaOwner, _StepLoss
from .tuning import hooks
from .vit import ViTAutoencoder, _Affine


class ViTClassifier(_ArenaOwner, _Base):
    """Classification module for ViT (models/vit.py:243-340), MI355X-native."""

    def __init__(self, config, device=None):
        super().__init__()
        # like ViTSOM, this does NOT lower torch's float32 matmul precision (vit.py:249): every contraction is fp32
        self.config = config
        if _HAVE_PL:
            self.save_hyperparameters(config)
        hp, data_hp = config["hyperparameters"], config["data"]
        vit_hp = hp["vit"]
        self.model = ViTAutoencoder(
            img_size=data_hp["input_size"], patch_size=vit_hp["patch_size"], in_chans=data_hp["num_channels"],
            embed_dim=vit_hp["emb_dim"], depth=vit_hp["depth"], num_heads=vit_hp["heads"],
            decoder_embed_dim=vit_hp["dec_emb_dim"], decoder_depth=vit_hp["dec_depth"],
            decoder_num_heads=vit_hp["heads"], mlp_ratio=vit_hp["mlp_ratio"], eps=1e-6)
        self.cls_head = _Affine((data_hp["num_classes"], vit_hp["emb_dim"]), (data_hp["num_classes"],))
        with torch.no_grad():
            self.cls_head.weight.normal_(std=0.02)
            bound = 1.0 / math.sqrt(vit_hp["emb_dim"])                  # nn.Linear's default bias init
            self.cls_head.bias.uniform_(-bound, bound)
        self.classification = True          # FusedAdamW: the decoder gets no gradient and no weight decay
        self.smoothing = 0.0                # nn.CrossEntropyLoss() (vit.py:279)
        self._it = 0
        self._n_train: Optional[int] = None
        self._est_steps: Optional[int] = None
        self._last: Dict[str, torch.Tensor] = {}
        self.arena: Optional[ParamArena] = None
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self._pack(torch.device(device))

    # -- arena ----------------------------------------------------------------------------------
    def _default_weight_decay(self, name: str, p) -> float:
        if name.startswith("model."):
            return 0.0 if p.ndim == 1 else 0.05
        return 0.01

    def _after_pack(self):
        self._build_weight_transposes()

    def _decoder_param_names(self):
        return [n for n, _ in self._named_trainable() if n.startswith("model.decoder_")]

    def _build_weight_transposes(self):
        """W^T copies of the encoder Linear weights for the blocks' input-gradient GEMMs (as ViTSOM keeps them)."""
        arena, dev = self.arena, self.arena.device
        rows, views, off = [], {}, 0
        for n, p in self._named_trainable():
            if not (n.startswith("model.blocks.") and p.ndim == 2 and n.endswith(".weight")):
                continue
            N, K = p.shape
            if N % 4 or K % 4:
                continue
            src = (arena.p(n).data_ptr() - arena.params.data_ptr()) // 4
            rows.append((src, off, N, K))
            views[arena.p(n).data_ptr()] = (off, K, N)
            off += -(-N * K // 64) * 64
        self._wt_flat = torch.empty(max(off, 1), dtype=torch.float32, device=dev)
        self._wt_table = torch.tensor(rows, dtype=torch.int64, device=dev).view(-1, 4) if rows else None
        self._wt_views = {k: self._wt_flat[o:o + a * b].view(a, b) for k, (o, a, b) in views.items()}
        self._wt_max = (max(r[2] for r in rows), max(r[3] for r in rows)) if rows else (1, 1)

    def _refresh_weight_transposes(self):
        if self._wt_table is not None and self._wt_flat.is_cuda:
            ops.transpose_many(self.arena.params, self._wt_flat, self._wt_table, *self._wt_max)

    def _WT(self, weight):
        return self._wt_views.get(weight.data_ptr())

    def set_schedule(self, n_train: int, estimated_stepping_batches: int):
        """Trainer-less bookkeeping for train.fit(); this model has no schedule of its own."""
        self._n_train, self._est_steps = int(n_train), int(estimated_stepping_batches)

    def _log(self, *a, **k):
        if _HAVE_PL and getattr(self, "_trainer", None) is not None:
            self.log_dict(*a, **k) if isinstance(a[0], dict) else self.log(*a, **k)

    def _ensure_streams(self, device):
        """The weight-gradient side stream, shared with every ViTSOM of the process (model.py _STEP_STREAMS)."""
        if getattr(self, "_side_stream", None) is None or self._side_stream.device != device:
            key = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
            pair = _STEP_STREAMS.get(key)
            if pair is None:
                pair = _STEP_STREAMS[key] = (torch.cuda.Stream(device=device), torch.cuda.Stream(device=device))
            self._side_stream = pair[0]
        self.model.__dict__["_lent_stream"] = self._side_stream

    # -- buffers ----------------------------------------------------------------------------------
    def _cls_view(self, buf: torch.Tensor, a: _Acts):
        """The B CLS rows of a [B*N, E] buffer, as a strided [B, E] view."""
        E = self.model.embed_dim
        return torch.as_strided(buf, (a.B, E), (a.N * E, 1), buf.storage_offset())

    def _buffers_for(self, B: int, device):
        a = self.model._buffers_for(B, device)
        c = a.__dict__.get("cls")
        if c is None:
            vit, E = self.model, self.model.embed_dim
            hid, H, C = vit.blocks[-1].hidden, vit.num_heads, self.cls_head.weight.shape[0]
            f = lambda *s: torch.empty(*s, dtype=torch.float32, device=device)   # noqa: E731
            c = a.cls = _Acts()
            # the pruned last block: K/V of every token, everything else on the CLS rows
            c.q, c.kv, c.ao, c.lse = f(B, E), f(a.T, 2 * E), f(B, E), f(B, H)
            c.x1, c.a2, c.mean2, c.rstd2 = f(B, E), f(B, E), f(B), f(B)
            c.hpre, c.hact, c.x2 = f(B, hid), f(B, hid), f(B, E)
            c.xe, c.mean_e, c.rstd_e = f(B, E), f(B), f(B)
            c.logits, c.dlogits = f(B, C), f(B, C)
            c.dxe, c.gx2, c.dh, c.da, c.gx1, c.dao, c.dq = f(B, E), f(B, E), f(B, hid), f(B, E), f(B, E), f(B, E), f(B, E)
            c.dkv, c.da1 = f(a.T, 2 * E), f(a.T, E)
            c.main_sum = f(1)
            c.loss_ring = torch.zeros(_LOSS_RING, 4, dtype=torch.float32, device=device)
            c.loss_slot = 0
            c.pruned = False
        return a, c

    # -- forward ----------------------------------------------------------------------------------
    def _last_block_fwd(self, cur, a: _Acts, c: _Acts):
        """The last encoder block on the CLS rows (K/V over all rows) and the final LayerNorm -> c.xe [B, E]."""
        vit = self.model
        blk, L = vit.blocks[-1], a.enc[-1]
        E, B, N, eps = vit.embed_dim, a.B, a.N, vit.eps
        Wqkv, bqkv = blk.attn.qkv.weight, blk.attn.qkv.bias
        ops.layernorm_fwd(cur, blk.norm1.weight, blk.norm1.bias, L.a1, L.mean1, L.rstd1, eps)
        ops.linear_fwd(L.a1, Wqkv[E:], bqkv[E:], c.kv)
        ops.linear_fwd(self._cls_view(L.a1, a), Wqkv[:E], bqkv[:E], c.q)
        ops.attention_q1_fwd(c.q, c.kv, c.ao, c.lse, B, N, blk.heads, E // blk.heads)
        ops.linear_residual_fwd(c.ao, blk.attn.proj.weight, blk.attn.proj.bias, self._cls_view(cur, a), B, c.x1)
        ops.layernorm_fwd(c.x1, blk.norm2.weight, blk.norm2.bias, c.a2, c.mean2, c.rstd2, eps)
        ops.linear_gelu_fwd(c.a2, blk.mlp["0"].weight, blk.mlp["0"].bias, c.hpre, c.hact)
        ops.linear_residual_fwd(c.hact, blk.mlp["2"].weight, blk.mlp["2"].bias, c.x1, B, c.x2)
        ops.layernorm_fwd(c.x2, vit.norm.weight, vit.norm.bias, c.xe, c.mean_e, c.rstd_e, eps)

    @torch.no_grad()
    def _run_forward(self, x):
        x = self.model._check_input(x)
        if not x.is_cuda:
            raise ValueError("ViTClassifier: input must live on the MI355X (there is no CPU path)")
        a, c = self._buffers_for(x.shape[0], x.device)
        self._ensure_streams(x.device)
        vit = self.model
        c.pruned = bool(hooks.cls_prune)
        if c.pruned:
            cur = vit._encode_trunk(x, a, len(vit.blocks) - 1)
            self._last_block_fwd(cur, a, c)
            feat = c.xe
        else:
            vit._encode(x, a)
            feat = self._cls_view(a.xe, a)
        ops.linear_fwd(feat, self.cls_head.weight, self.cls_head.bias, c.logits)
        return x, a, c

    @torch.no_grad()
    def forward(self, x):
        """vit.py:281-284 -> logits [B, C].  Runs under no_grad: the result is not differentiable under torch autograd
        (training goes through training_step / train_step_fused)."""
        return self._run_forward(x)[2].logits.clone()

    @torch.no_grad()
    def predict(self, x):
        """(None, logits [B, C]) as views of internal buffers (valid until the next call): the shape
        evaluation.evaluate_classification reads, the `vit` branch of the reference's evaluation.py:109-110."""
        return None, self._run_forward(x)[2].logits

    @torch.no_grad()
    def _forward_losses(self, x, y, gamma_t=0.0, T=0.0, want_grad=True):
        """Forward + cross-entropy (+ dL/dlogits when want_grad); the mean loss as a 0-dim device tensor (a slot of a
        small ring, like ViTSOM's, so the value stays readable for the next few steps).  gamma_t / T are unused: they
        keep _ArenaOwner._step's call shape."""
        x, a, c = self._run_forward(x)
        B = a.B
        self._ctx = (x, a, c)
        self._forward_id, self._seeds_consumed = self._forward_id + 1, False
        yv = y.view(-1)
        if yv.device != x.device:
            yv = yv.to(x.device)
        if yv.dtype != torch.int64:
            yv = yv.long()
        ops.cross_entropy_ls(c.logits, yv.contiguous(), self.smoothing, c.main_sum,
                             dlogits=c.dlogits if want_grad else None, grad_scale=1.0 / B)
        c.loss_slot = (c.loss_slot + 1) % _LOSS_RING
        parts = c.loss_ring[c.loss_slot]
        ops.loss_parts(parts, c.main_sum, 1.0 / B, c.main_sum, 0.0, 0.0)
        self._last = {"total": parts[0], "main": parts[1]}
        return parts[0]

    # -- backward ---------------------------------------------------------------------------------
    @torch.no_grad()
    def _scale_seeds(self, gout):
        c = self._ctx[2]
        ops.scale_by(c.dlogits, gout.detach().reshape(1).float().contiguous())

    def _exchange_buckets(self):
        """Arena slices reduced early, in the order the backward finishes them: name -> (lo, hi)."""
        b = self.__dict__.get("_bucket_cache")
        if b is not None and b[0] is self.arena:
            return b[1]
        out = {"head": self._arena_span("cls_head.weight", "cls_head.bias")}
        D = len(self.model.blocks)
        step = max(1, int(hooks.bucket_blocks))
        hi_name = "model.norm.bias"
        for i in range(D - step, 0, -step):                 # blocks [i, i + step) (+ the final norm for the top bucket)
            out[f"enc{i}"] = self._arena_span(f"model.blocks.{i}.norm1.weight", hi_name)
            hi_name = f"model.blocks.{i - 1}.mlp.2.bias"
        self.__dict__["_bucket_cache"] = (self.arena, out)
        return out

    def _last_block_bwd(self, a: _Acts, c: _Acts, G):
        """Backward of the pruned last block from c.gx2 = dL/d(its CLS outputs); leaves dL/d(its input) [T, E] in the
        first gradient buffer of the ring, where ViTAutoencoder._encoder_bwd(depth=D-1) starts."""
        vit = self.model
        D = len(vit.blocks)
        blk, L = vit.blocks[-1], a.enc[-1]
        E, B, N = vit.embed_dim, a.B, a.N
        pre = f"blocks.{D - 1}"
        x_in = a.enc[D - 2].x2 if D > 1 else a.tok0
        ops.linear_bwd_weight(c.gx2, c.hact, G(f"{pre}.mlp.2.weight"), G(f"{pre}.mlp.2.bias"))
        ops.linear_bwd_input(c.gx2, blk.mlp["2"].weight, c.dh, gelu_grad=c.hpre)
        ops.linear_bwd_weight(c.dh, c.a2, G(f"{pre}.mlp.0.weight"), G(f"{pre}.mlp.0.bias"))
        ops.linear_bwd_input(c.dh, blk.mlp["0"].weight, c.da)
        ops.layernorm_bwd(c.da, c.x1, c.mean2, c.rstd2, blk.norm2.weight, c.gx2, c.gx1, G(f"{pre}.norm2.weight"),
                          G(f"{pre}.norm2.bias"))
        ops.linear_bwd_weight(c.gx1, c.ao, G(f"{pre}.attn.proj.weight"), G(f"{pre}.attn.proj.bias"))
        ops.linear_bwd_input(c.gx1, blk.attn.proj.weight, c.dao)
        ops.attention_q1_bwd(c.dao, c.ao, c.lse, c.q, c.kv, c.dq, c.dkv, B, N, blk.heads, E // blk.heads)
        # the qkv weight gradient by row slice: Q rows from the B CLS rows, K/V rows from all T rows
        Wqkv, gW, gb = blk.attn.qkv.weight, G(f"{pre}.attn.qkv.weight"), G(f"{pre}.attn.qkv.bias")
        a1_cls = self._cls_view(L.a1, a)
        ops.linear_bwd_weight(c.dq, a1_cls, gW[:E], gb[:E])
        ops.linear_bwd_weight(c.dkv, L.a1, gW[E:], gb[E:])
        # d(norm1 out) = dKV W_kv, plus dQ W_q on the CLS rows
        ops.linear_bwd_input(c.dkv, Wqkv[E:], c.da1)
        ops.linear_bwd_input(c.dq, Wqkv[:E], self._cls_view(c.da1, a), accumulate=True)
        g0 = vit._views(a, E)[0]
        ops.layernorm_bwd(c.da1, x_in, L.mean1, L.rstd1, blk.norm1.weight, None, g0, G(f"{pre}.norm1.weight"),
                          G(f"{pre}.norm1.bias"))
        ops.rows_add(c.gx1, self._cls_view(g0, a))          # the residual path reaches the CLS rows only

    @torch.no_grad()
    def _backward(self):
        """All backward kernels; overwrites the whole gradient arena (no accumulation)."""
        x, a, c = self._ctx
        vit = self.model
        self._grads_reduced = False
        self._exchange_reset()
        if hooks.side_stream:
            self._ensure_streams(x.device)
            vit._side = self._side_stream
        else:
            vit._side = None
        Gv = self._G("model.")
        self._refresh_weight_transposes()
        jobs = None
        if hooks.ln_reduce_batched:
            jobs = a.__dict__.get("ln_jobs")
            if jobs is None:
                jobs = a.ln_jobs = ops.LayerNormJobs(x.device)
            jobs.begin()
        vit.__dict__["_ln_jobs"] = jobs
        try:
            self._backward_body(a, c, Gv, jobs)
        finally:
            vit.__dict__["_ln_jobs"] = None

    def _backward_body(self, a: _Acts, c: _Acts, Gv, jobs):
        vit = self.model
        D = len(vit.blocks)
        buckets = self._exchange_buckets() if self._overlap_enabled() else {}
        main = torch.cuda.current_stream()

        def streams_now():
            return [st for st in (main, vit._side) if st is not None]

        def flush():
            if jobs is not None:
                jobs.flush()

        def on_block(i):
            b = buckets.get(f"enc{i}")
            if b is not None:
                flush()
                self._reduce_early(*b, streams=streams_now())

        # the decoder is never run: its gradients are exactly zero (one fill over its contiguous arena slice)
        dec = self._decoder_param_names()
        if dec:
            lo, hi = self._arena_span(dec[0], dec[-1])
            ops.fill(self.arena.grads[lo:hi], 0.0)
        gw, gb = self._grad_views["cls_head.weight"], self._grad_views["cls_head.bias"]
        if c.pruned:
            ops.linear_bwd_weight(c.dlogits, c.xe, gw, gb)
            if "head" in buckets:
                self._reduce_early(*buckets["head"], streams=[main])
            ops.linear_bwd_input(c.dlogits, self.cls_head.weight, c.dxe)
            ops.layernorm_bwd(c.dxe, c.x2, c.mean_e, c.rstd_e, vit.norm.weight, None, c.gx2, Gv("norm.weight"),
                              Gv("norm.bias"))
            self._last_block_bwd(a, c, Gv)
            on_block(D - 1)
            vit._encoder_bwd(a, Gv, self._WT, on_block, depth=D - 1)
        else:
            ops.fill(a.d_xe, 0.0)
            ops.linear_bwd_weight(c.dlogits, self._cls_view(a.xe, a), gw, gb)
            if "head" in buckets:
                self._reduce_early(*buckets["head"], streams=[main])
            ops.linear_bwd_input(c.dlogits, self.cls_head.weight, self._cls_view(a.d_xe, a), accumulate=True)
            vit._encoder_bwd(a, Gv, self._WT, on_block)
        flush()
        if vit._side is not None:
            stream_wait_stream(None, vit._side)             # every gradient is final from here on
            vit.__dict__.setdefault("_side_pending", []).clear()

    # -- reference API ------------------------------------------------------------------------------
    def training_step(self, batch, batch_idx):
        """vit.py:286-292.  Returns a scalar tensor; ``.backward()`` runs the HIP backward."""
        x, y = batch
        if self._anchor is None:
            self._anchor = torch.zeros((), device=self.arena.device, requires_grad=True)
        loss = _StepLoss.apply(self._anchor, self, x, y, 0.0, 0.0)
        self._it += 1
        self._log("train/cls_loss", self._last["main"], on_step=True, on_epoch=False, prog_bar=True)
        return loss

    def train_step_fused(self, x, y):
        """The same step without the autograd bridge: forward + loss + backward into the gradient arena (the caller
        then runs optimizer.step()).  Returns the loss tensor."""
        total, backward = self._step(x, y, 0.0, 0.0)
        backward()
        self._it += 1
        return total

    def validation_step(self, batch, batch_idx):
        """vit.py:294-302."""
        x, y = batch
        total = self._forward_losses(x, y, want_grad=False)
        c = self._ctx[2]
        self._last["acc"] = (c.logits.argmax(dim=-1) == y.view(-1).to(c.logits.device)).float().mean()
        self._log({"val/cls_loss": self._last["main"], "val/accuracy": self._last["acc"]}, on_step=False, on_epoch=True)
        return total.clone()

    def configure_optimizers(self):
        """vit.py:304-336: layer-decay groups of the ViT plus the head's group (AdamW's default weight decay 0.01),
        lr * batch_size / 256, per-epoch LambdaLR with the warm-up / cosine multiplier floored at min_lr."""
        hp = self.config["hyperparameters"]
        opt_hp = hp["optimizer"]
        groups = param_groups_lrd(self.model, weight_decay=opt_hp["weight_decay"], layer_decay=opt_hp["layer_decay"])
        groups.append({"params": list(self.cls_head.parameters())})
        if opt_hp["type"] not in ("adamw", "adam"):
            raise ValueError(f"unsupported optimizer type {opt_hp['type']!r}")
        optimizer = FusedAdamW(self, groups, lr=opt_hp["lr"] * hp["batch_size"] / 256,
                               betas=(opt_hp["beta_1"], opt_hp["beta_2"]), adamw=(opt_hp["type"] == "adamw"))
        if opt_hp["scheduler"] != "cosine_annealing":
            raise ValueError(f"unsupported scheduler {opt_hp['scheduler']!r}")
        lr_func = lambda epoch: max(opt_hp["min_lr"], min((epoch + 1) / (opt_hp["warmup_epochs"] + 1e-8),   # noqa: E731
                                                           0.5 * (math.cos(epoch / hp["total_epochs"] * math.pi) + 1)))
        scheduler = torch.optim.lr_scheduler.LambdaLR(optimizer, lr_lambda=lr_func)
        return [optimizer], [scheduler]

    # Lightning's .ckpt layout, written and read exactly as ViTSOM does (torch.load(weights_only=True))
    save_checkpoint = ViTSOM.save_checkpoint
    load_from_checkpoint = classmethod(ViTSOM.load_from_checkpoint.__func__)

    def on_train_end(self):                                             # vit.py:338-345
        print(f"Peak GPU memory usage: {torch.cuda.max_memory_allocated() / 1e9:.4f} GB")
