"""ViTClassifier (models/vit.py:243-340): the plain ViT baseline the paper measures ViT-SOM against, on the HIP kernels.

The module surface is the reference's: ``model`` (a ViTAutoencoder, decoder included and never run), ``cls_head``,
``state_dict`` keys ``model.*`` / ``cls_head.*``, CrossEntropyLoss WITHOUT label smoothing (vit.py:279: the configs'
``optimizer.smoothing`` is not read for this model), the same optimizer groups and schedule.  What it shares with ViTSOM
-- parameters in one flat arena, the W^T copies, streams, encoder buckets, the backward's frame, optimizer and
checkpoints -- is vit_owner.py's.

The training step is encoder-only and prunes the last encoder block: forward_features reads only norm(x)[:, 0]
(vit.py:174-179), so in the last block only the CLS row's output is ever used.  K and V are still projected for every
token, but the query, the attention (one query per image and head: ops.attention_q1_*), proj, norm2, the MLP and the
final LayerNorm run on the B CLS rows only.  ``tuning.hooks.cls_prune = False`` runs the last block in full instead.
There is no CPU path and no launch tape: the step is host-driven.
"""
import torch

from . import ops
from ._base import _Acts
from .tuning import hooks
from .vit_owner import _ViTOwner


class ViTClassifier(_ViTOwner):
    """Classification module for ViT (models/vit.py:243-340), MI355X-native."""

    _vit_name = "model"

    def __init__(self, config, device=None):
        super().__init__(config)
        self._add_cls_head()
        self.classification = True          # FusedAdamW: the decoder gets no gradient and no weight decay
        self.smoothing = 0.0                # nn.CrossEntropyLoss() (vit.py:279)
        self._pack(self._default_device(device))

    def set_schedule(self, n_train: int, estimated_stepping_batches: int):
        """Trainer-less bookkeeping for train.fit(); this model has no schedule of its own."""
        self._n_train, self._est_steps = int(n_train), int(estimated_stepping_batches)

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
            self._loss_buffers(c, device)
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
            cur = vit._encode_trunk(x, a, len(vit.blocks) - 1, self._side_stream)
            self._last_block_fwd(cur, a, c)
            feat = c.xe
        else:
            vit._encode(x, a, self._side_stream)
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

    def attention_rollout(self, x, query="cls", head_fusion="mean", residual=0.5, start_layer=0):
        """ViTAutoencoder.attention_rollout of the encoder -> [B, N]: a full encode, whatever hooks.cls_prune says -- the
        CLS-pruned last block keeps no qkv for all queries."""
        return self.model.attention_rollout(x, query, head_fusion, residual, start_layer)

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
        parts = self._next_loss_slot(c)
        ops.loss_parts(parts, c.main_sum, 1.0 / B, c.main_sum, 0.0, 0.0)
        self._last = {"total": parts[0], "main": parts[1]}
        return parts[0]

    # -- backward ---------------------------------------------------------------------------------
    @torch.no_grad()
    def _scale_seeds(self, gout):
        c = self._ctx[2]
        ops.scale_by(c.dlogits, gout.detach().reshape(1).float().contiguous())

    def _head_buckets(self):
        return {"head": self._arena_span("cls_head.weight", "cls_head.bias")}

    def _head_params(self):
        return list(self.cls_head.parameters())

    def _last_block_bwd(self, a: _Acts, c: _Acts, sched):
        """Backward of the pruned last block from c.gx2 = dL/d(its CLS outputs); leaves dL/d(its input) [T, E] in the
        first gradient buffer of the ring, where ViTAutoencoder._encoder_bwd(depth=D-1) starts."""
        vit, G = self.model, sched.G
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

    def _head_backward(self, a: _Acts, c: _Acts, sched, reduce):
        """The cls_head backward, then (pruned) the final LayerNorm and the last block on the CLS rows; returns the
        number of encoder blocks left to run."""
        vit = self.model
        D = len(vit.blocks)
        main = torch.cuda.current_stream()
        self._zero_decoder_grads()
        gw, gb = self._grad_views["cls_head.weight"], self._grad_views["cls_head.bias"]
        if c.pruned:
            ops.linear_bwd_weight(c.dlogits, c.xe, gw, gb)
            reduce("head", [main])
            ops.linear_bwd_input(c.dlogits, self.cls_head.weight, c.dxe)
            ops.layernorm_bwd(c.dxe, c.x2, c.mean_e, c.rstd_e, vit.norm.weight, None, c.gx2, sched.G("norm.weight"),
                              sched.G("norm.bias"))
            self._last_block_bwd(a, c, sched)
            reduce(f"enc{D - 1}")
            return D - 1
        ops.fill(a.d_xe, 0.0)
        ops.linear_bwd_weight(c.dlogits, self._cls_view(a.xe, a), gw, gb)
        reduce("head", [main])
        ops.linear_bwd_input(c.dlogits, self.cls_head.weight, self._cls_view(a.d_xe, a), accumulate=True)
        return None

    # -- reference API ------------------------------------------------------------------------------
    def training_step(self, batch, batch_idx):
        """vit.py:286-292.  Returns a scalar tensor; ``.backward()`` runs the HIP backward."""
        x, y = batch
        loss = self._step_loss(x, y, 0.0, 0.0)
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
