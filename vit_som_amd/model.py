"""Host-side mirror of the reference's module surface for the ViT-SOM training-step hot path.

Classes keep the reference's names, constructor (the YAML-schema ``config`` dict), method
names, positional return tuples / dtypes and ``state_dict`` keys:

  ViTSOM          models/vit_som.py:17-187   forward / training_step / validation_step /
                                             configure_optimizers
  ViTAutoencoder  models/vit.py:66-240       forward / forward_features / patchify / unpatchify
                                             (vit.py)
  SOMLayer        models/som_layer.py:8-152  forward / compute_distances / update_temperature /
                                             compute_weights / som_loss / index_to_position (som.py)

FusedAdamW and param_groups_lrd live in optim.py; the fused step's autograd bridge, launch tape
and arena owner, shared with DESOM, in step.py.  All arithmetic runs in libvitsom_hip.so
(hand-written gfx950 kernels) through ``ops``; these files only own memory (flat parameter
arenas, activation buffers), ordering, schedules and the data-parallel exchange (one RCCL
all-reduce over the gradient arena).  There is no CPU path.
"""
import math
import os
from typing import Dict, Optional

import torch

from . import ops
from ._base import _HAVE_PL, _Acts, _Base
from ._lib import Event, on_stream, stream_wait_stream
from .arena import ParamArena
from .optim import FusedAdamW, param_groups_lrd
from .som import SOMLayer
from .step import _ArenaOwner, _StepLoss, _StepTape
from .tuning import hooks
from .vit import ViTAutoencoder, _Affine

_LOSS_RING = 16     # the loss terms of a step stay readable until this many further steps have run
_STEP_STREAMS: Dict[int, tuple] = {}        # device index -> (side stream, SOM stream), shared by every model of the process


# ------------------------------------------------------------------------------------ ViT-SOM
class ViTSOM(_ArenaOwner, _Base):
    """Vision Transformer Self-Organizing Map (models/vit_som.py:17-187), MI355X-native."""

    def __init__(self, config, device=None):
        super().__init__()
        # NOTE: unlike vit_som.py:23 this does NOT lower torch's global float32 matmul precision:
        # every contraction here is exact fp32 on MFMA.
        self.config = config
        if _HAVE_PL:
            self.save_hyperparameters(config)
        hp, data_hp = config["hyperparameters"], config["data"]
        vit_hp, opt_hp, som_hp = hp["vit"], hp["optimizer"], hp["som"]
        self.gamma = hp["gamma"]
        self.use_reduced = som_hp["use_reduced"]
        self.classification = data_hp["num_classes"] > 0
        self.vit = ViTAutoencoder(
            img_size=data_hp["input_size"], patch_size=vit_hp["patch_size"], in_chans=data_hp["num_channels"],
            embed_dim=vit_hp["emb_dim"], depth=vit_hp["depth"], num_heads=vit_hp["heads"],
            decoder_embed_dim=vit_hp["dec_emb_dim"], decoder_depth=vit_hp["dec_depth"],
            decoder_num_heads=vit_hp["heads"], mlp_ratio=vit_hp["mlp_ratio"], eps=1e-6)
        self.som_layer = SOMLayer(config)
        if self.classification:
            self.cls_head = _Affine((data_hp["num_classes"], vit_hp["emb_dim"]), (data_hp["num_classes"],))
            with torch.no_grad():
                self.cls_head.weight.normal_(std=0.02)
                bound = 1.0 / math.sqrt(vit_hp["emb_dim"])
                self.cls_head.bias.uniform_(-bound, bound)
        self.smoothing = float(opt_hp["smoothing"])
        self.register_buffer("iteration", torch.tensor(0))
        self._it = 0
        self._n_train: Optional[int] = None
        self._est_steps: Optional[int] = None
        self.world_size, self.rank = 1, 0
        self._grads_reduced = False
        self._forward_id, self._seeds_consumed = 0, False
        self._last: Dict[str, torch.Tensor] = {}
        self.arena: Optional[ParamArena] = None
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self._pack(torch.device(device))

    # -- arenas -------------------------------------------------------------------------------
    def _default_weight_decay(self, name: str, p) -> float:
        if name.startswith("vit."):
            return 0.0 if p.ndim == 1 else 0.05
        return 0.01

    def _after_pack(self):
        self._build_weight_transposes()

    def _decoder_param_names(self):
        return [n for n, _ in self._named_trainable() if n.startswith("vit.decoder_")]

    def _build_weight_transposes(self):
        """Transposed copies W^T of the ViT Linear weights whose input gradient is needed, so that
        dX = dY W runs on the forward's kernel family (both operands contiguous along the reduction).
        One flat buffer + a device table; refreshed by ONE batched transpose per backward pass."""
        arena, dev = self.arena, self.arena.device
        rows, views, off = [], {}, 0
        for n, p in self._named_trainable():
            if not (n.startswith("vit.") and p.ndim == 2 and n.endswith(".weight")) or "patch_embed" in n:
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

    # -- schedules ----------------------------------------------------------------------------
    def set_schedule(self, n_train: int, estimated_stepping_batches: int):
        """Trainer-less replacement for len(trainer.train_dataloader.dataset) and
        trainer.estimated_stepping_batches (som_layer.py:131, vit_som.py:89)."""
        self._n_train, self._est_steps = int(n_train), int(estimated_stepping_batches)
        self.som_layer._n_train = int(n_train)

    def _estimated_steps(self) -> int:
        if self._est_steps is not None:
            return self._est_steps
        tr = getattr(self, "_trainer", None) if not _HAVE_PL else getattr(self, "trainer", None)
        if tr is None:
            raise RuntimeError("ViTSOM: call set_schedule(n_train, estimated_stepping_batches) or attach a trainer")
        self.som_layer._trainer_ref = tr
        return int(tr.estimated_stepping_batches)

    def _gamma_t(self) -> float:                                        # vit_som.py:89-90 (host int, no .item() sync)
        ramp_up_end_step = self._estimated_steps() // 2
        return self.config["hyperparameters"]["gamma"] * min(1.0, self._it / ramp_up_end_step)

    def _log(self, *a, **k):
        """self.log / self.log_dict when a Lightning trainer is attached (vit_som.py:95-101); a no-op otherwise.
        Errors raised by Lightning's logger propagate."""
        if _HAVE_PL and getattr(self, "_trainer", None) is not None:
            self.log_dict(*a, **k) if isinstance(a[0], dict) else self.log(*a, **k)

    # -- fused forward + losses ---------------------------------------------------------------
    def _som_input(self, a: _Acts):
        E, N, B = self.vit.embed_dim, a.N, a.B
        if self.use_reduced:
            return torch.as_strided(a.xe, (B, E), (N * E, 1), a.xe.storage_offset())
        return torch.as_strided(a.xe, (B, (N - 1) * E), (N * E, 1), a.xe.storage_offset() + E)

    def _cls_view(self, buf: torch.Tensor, a: _Acts):
        E = self.vit.embed_dim
        return torch.as_strided(buf, (a.B, E), (a.N * E, 1), buf.storage_offset())

    @torch.no_grad()
    def _run_forward(self, x, need_decoder: bool, fresh_w: bool = False):
        x = self.vit._check_input(x)
        if not x.is_cuda:
            raise ValueError("ViTSOM: input must live on the MI355X (there is no CPU path)")
        a = self.vit._buffers_for(x.shape[0], x.device)
        self._ensure_streams(x.device)
        # the prototypes' plane image for the BMU pass: re-split on the SOM stream while the encoder runs
        w_ready = self.som_layer._w_planes_async(self._som_stream, fresh_w) if self.som_layer._planes_shape_ok(a.B) else None
        self.vit._encode(x, a)
        s = self.som_layer._buffers_for(a.B, x.device)
        if need_decoder and hooks.bmu_overlap and hooks.side_stream:
            # The BMU pass and the decoder both start from the encoder output and do not meet before the losses: the pass
            # runs on the SOM stream (behind the prototypes' image, which is written there) under the decoder's
            # latency-bound kernels.
            som = self._som_stream
            Event.pooled().record().wait(som)
            with on_stream(som):
                self.som_layer._distances_into(self._som_input(a), s)
            self.vit._decode(a)
            Event.pooled().record(som).wait()
        else:
            if need_decoder:
                self.vit._decode(a)
            if w_ready is not None:
                w_ready.wait()
            self.som_layer._distances_into(self._som_input(a), s)
        if self.classification:
            if not hasattr(a, "logits"):
                a.logits = torch.empty(a.B, self.cls_head.weight.shape[0], dtype=torch.float32, device=x.device)
                a.dlogits = torch.empty_like(a.logits)
            ops.linear_fwd(self._cls_view(a.xe, a), self.cls_head.weight, self.cls_head.bias, a.logits)
        return x, a, s

    @torch.no_grad()
    def forward(self, x):
        """vit_som.py:67-78 -> (cls_token, recon_img, logits | None, distances, bmu_indices[int64])."""
        x, a, s = self._run_forward(x, need_decoder=True)
        recon = torch.empty_like(x)
        tmp = torch.empty(1, dtype=torch.float32, device=x.device)
        ops.l1_unpatchify(a.pred, x, tmp, recon=recon, p=self.vit.patch_embed.patch_size[0])
        cls = self._cls_view(a.xe, a).clone()
        logits = a.logits.clone() if self.classification else None
        return cls, recon, logits, s.dist.clone(), s.bmu.clone()

    @torch.no_grad()
    def predict(self, x):
        """Inference fast path for tools/evaluation.py: encoder + SOM (+ cls head) only -- the decoder,
        whose output evaluate_clustering / evaluate_classification never read, is skipped.  Returns
        (bmu_indices [B] int64, logits [B,C] | None) as views of internal buffers (valid until the
        next call)."""
        x, a, s = self._run_forward(x, need_decoder=False)
        return s.bmu, (a.logits if self.classification else None)

    # The two calls of the step whose arguments change from step to step (temperature, gamma ramp): the host issues them
    # itself, also when the rest of the step is replayed from a launch tape (tape holes).
    def _call_neigh(self, s: _Acts, gamma_t: float, T: float, B: int, want_grad: bool):
        K = self.som_layer.n_prototypes
        if want_grad:
            ops.som_neigh_loss(s.dist, s.bmu, self.som_layer.grid_positions, T, s.loss_sum, inv_nx=s.inx, inv_nw=s.inw,
                               grad_scale=gamma_t / (B * K), coef=s.coef, row_dot=s.row_dot, col_dot=s.col_dot,
                               distance=self.som_layer._dist_mode)
        else:
            ops.som_neigh_loss(s.dist, s.bmu, self.som_layer.grid_positions, T, s.loss_sum,
                               distance=self.som_layer._dist_mode)

    def _call_parts(self, a: _Acts, s: _Acts, gamma_t: float, T: float, B: int, numel_x: int, want_grad: bool):
        # total = main + gamma_t * som (and the two terms by themselves, for logging) from the two device-side sums, in one
        # tiny kernel that also advances the `iteration` buffer of a training step (vit_som.py:104): no ATen kernel in
        # the step.  The three values land in their own slot of a small ring, so `_last` and the returned loss stay
        # valid for the next _LOSS_RING - 1 steps (plain tensors: .get / `in` / iteration / ** all see them).
        K = self.som_layer.n_prototypes
        main_scale = 1.0 / B if self.classification else 1.0 / numel_x
        a.loss_slot = (a.loss_slot + 1) % _LOSS_RING
        parts = a.loss_ring[a.loss_slot]
        ops.loss_parts(parts, a.main_sum, main_scale, s.loss_sum, gamma_t / (B * K), 1.0 / (B * K),
                       counter=self.iteration if want_grad else None)
        self._last = {"total": parts[0], "main": parts[1], "som": parts[2], "gamma_t": gamma_t, "T": T}
        return parts[0]

    def _loss_buffers(self, a: _Acts, dev):
        if not hasattr(a, "main_sum"):
            a.main_sum = torch.empty(1, dtype=torch.float32, device=dev)
            a.loss_ring = torch.zeros(_LOSS_RING, 4, dtype=torch.float32, device=dev)
            a.loss_slot = 0

    @torch.no_grad()
    def _forward_losses(self, x, y, gamma_t: float, T: float, want_grad: bool):
        """All forward kernels + both losses (+ loss-side gradients when want_grad).  Returns the
        total loss as a 0-dim device tensor; parts land in self._last."""
        # (a training step always re-splits the prototypes unless the optimizer keeps their image: a recorded step must
        # not depend on the state it was recorded in)
        x, a, s = self._run_forward(x, need_decoder=not self.classification, fresh_w=want_grad and not hooks.adamw_planes)
        B = a.B
        self._ctx = (x, a, s)
        self._forward_id, self._seeds_consumed = self._forward_id + 1, False
        self._loss_buffers(a, x.device)
        with ops.tape_hole():
            self._call_neigh(s, gamma_t, T, B, want_grad)
        if self.classification:
            yv = y.view(-1)
            if yv.dtype != torch.int64:
                yv = yv.long()
            ops.cross_entropy_ls(a.logits, yv.contiguous(), self.smoothing, a.main_sum,
                                 dlogits=a.dlogits if want_grad else None, grad_scale=1.0 / B)
        else:
            ops.l1_unpatchify(a.pred, x, a.main_sum, dpred=a.dpred if want_grad else None, grad_scale=1.0 / x.numel(),
                              p=self.vit.patch_embed.patch_size[0])
        with ops.tape_hole():
            total = self._call_parts(a, s, gamma_t, T, B, x.numel(), want_grad)
        return total

    def _ensure_streams(self, device):
        """The two extra HIP streams of the step (kept to two: a process has few hardware queues)."""
        if getattr(self, "_side_stream", None) is None or self._side_stream.device != device:
            # one pair per device for the whole process: which hardware queue a stream lands on depends on how many
            # streams the process has created, and two of a model's streams on one queue serialise (measured: the 3rd, 5th
            # ... model of a process ran its step 1.4x slower at batch 128)
            key = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
            pair = _STEP_STREAMS.get(key)
            if pair is None:
                pair = _STEP_STREAMS[key] = (torch.cuda.Stream(device=device), torch.cuda.Stream(device=device))
            self._side_stream = pair[0]      # weight-gradient GEMMs; second forward chain
            self._som_stream = pair[1]       # SOM backward + early all-reduce; the prototypes' plane image in the forward
        self.vit.__dict__["_lent_stream"] = self._side_stream

    @torch.no_grad()
    def _scale_seeds(self, gout):
        """Multiply the loss-side gradient seeds by the scalar `gout` (a 0-dim device tensor)."""
        _, a, s = self._ctx
        gout = gout.detach().reshape(1).float().contiguous()
        for buf in ((s.coef, s.row_dot, s.col_dot) + ((a.dlogits,) if self.classification else (a.dpred,))):
            ops.scale_by(buf, gout)

    def _exchange_buckets(self):
        """Arena slices reduced early, in the order the backward finishes them: name -> (lo, hi)."""
        b = self.__dict__.get("_bucket_cache")
        if b is not None and b[0] is self.arena:
            return b[1]
        names = [n for n, _ in self._named_trainable()]
        out = {"som": (self.arena.offsets["som_layer.prototypes"][0], self.arena.numel)}
        dec = [n for n in names if n.startswith("vit.decoder_")]
        if dec and not self.classification:
            out["decoder"] = self._arena_span(dec[0], dec[-1])
        D = len(self.vit.blocks)
        step = max(1, int(hooks.bucket_blocks))
        hi_name = "vit.norm.bias"
        for i in range(D - step, 0, -step):                 # blocks [i, i + step) (+ the final norm for the top bucket)
            out[f"enc{i}"] = self._arena_span(f"vit.blocks.{i}.norm1.weight", hi_name)
            hi_name = f"vit.blocks.{i - 1}.mlp.2.bias"
        self.__dict__["_bucket_cache"] = (self.arena, out)
        return out

    @torch.no_grad()
    def _backward(self):
        """All backward kernels; overwrites the whole gradient arena (no accumulation)."""
        x, a, s = self._ctx
        self._grads_reduced = False
        self._exchange_reset()
        if x.is_cuda and hooks.side_stream:
            self._ensure_streams(x.device)
            self.vit._side = self._side_stream
        else:
            self.vit._side = None
        Gv = self._G("vit.")
        self._refresh_weight_transposes()
        # the LayerNorm backwards leave their dgamma / dbeta reductions to one launch per exchange piece (or one in all)
        jobs = None
        if x.is_cuda and hooks.ln_reduce_batched:
            jobs = a.__dict__.get("ln_jobs")
            if jobs is None:
                jobs = a.ln_jobs = ops.LayerNormJobs(x.device)
            jobs.begin()
        self.vit.__dict__["_ln_jobs"] = jobs
        try:
            self._backward_body(x, a, s, Gv, jobs)
        finally:
            self.vit.__dict__["_ln_jobs"] = None

    def _backward_body(self, x, a, s, Gv, jobs):
        X = self._som_input(a)
        E, N = self.vit.embed_dim, a.N
        if self.use_reduced:
            gX = torch.as_strided(a.d_xe, (a.B, E), (N * E, 1), a.d_xe.storage_offset())
        else:
            gX = torch.as_strided(a.d_xe, (a.B, (N - 1) * E), (N * E, 1), a.d_xe.storage_offset() + E)
        buckets = self._exchange_buckets() if self._overlap_enabled() else {}
        main = torch.cuda.current_stream() if x.is_cuda else None

        def som_backward(gx_out, accumulate):
            if self.som_layer._dist_mode == ops.DIST_MANHATTAN:
                ops.som_bwd_manhattan(X, self.som_layer.prototypes, s.coef, self._grad_views["som_layer.prototypes"], gx_out,
                                      accumulate_gx=accumulate)
            else:
                ops.som_bwd(X, self.som_layer.prototypes, s.coef, s.row_dot, s.col_dot,
                            self._grad_views["som_layer.prototypes"], gx_out, accumulate_gx=accumulate)

        def streams_now():
            return [st for st in (main, self.vit._side) if st is not None]

        def flush():
            if jobs is not None:
                jobs.flush()

        side = self._som_stream if self.vit._side is not None else None
        if self.classification or side is None:
            if self.classification:
                ops.fill(a.d_xe, 0.0)
                # decoder is unused by the classification loss: its gradients are exactly zero
                for n in self._decoder_param_names():
                    ops.fill(self._grad_views[n], 0.0)
                ops.linear_bwd_weight(a.dlogits, self._cls_view(a.xe, a), self._grad_views["cls_head.weight"],
                                      self._grad_views["cls_head.bias"])
                ops.linear_bwd_input(a.dlogits, self.cls_head.weight, self._cls_view(a.d_xe, a), accumulate=True)
            else:
                self.vit._decoder_bwd(a, Gv, self._WT)
                if "decoder" in buckets:
                    flush()
                    self._reduce_early(*buckets["decoder"], streams=streams_now())
            som_backward(gX, True)
            if "som" in buckets:
                self._reduce_early(*buckets["som"], streams=streams_now())
        else:
            # The SOM backward depends only on the forward (coef, X, W), so it runs on a stream of its
            # own under the decoder backward and writes its input gradient straight into (the zeroed)
            # d_xe; the decoder's last GEMM waits for it and accumulates on top.  The prototype
            # all-reduce is issued behind it: it starts the moment gW is final, before the decoder
            # backward has finished.
            self.vit._event().record().wait(side)
            with on_stream(side):
                ops.fill(a.d_xe, 0.0)
                som_backward(gX, False)
            if "som" in buckets:
                self._reduce_early(*buckets["som"], streams=[side])
            # a dedicated event: its wait is deferred to the end of the decoder backward, by which time a pooled
            # (round-robin) event could have been re-recorded for something else (deep decoders)
            som_done = self.__dict__.get("_som_done_ev")
            if som_done is None:
                som_done = self.__dict__["_som_done_ev"] = Event()
            som_done.record(side)
            self.vit._decoder_bwd(a, Gv, self._WT, before_dxe=lambda: som_done.wait())
            if "decoder" in buckets:
                flush()
                self._reduce_early(*buckets["decoder"], streams=streams_now())

        def on_block(i):
            b = buckets.get(f"enc{i}")
            if b is not None:
                flush()
                self._reduce_early(*b, streams=streams_now())

        self.vit._encoder_bwd(a, Gv, self._WT, on_block if buckets else None)
        flush()
        if self.vit._side is not None:
            stream_wait_stream(None, self.vit._side)     # every gradient is final from here on
            self.vit.__dict__.setdefault("_side_pending", []).clear()

    # -- data-parallel exchange ----------------------------------------------------------------
    # -- reference API ---------------------------------------------------------------------------
    def _schedules_for_step(self):
        self.som_layer.update_temperature(self._it)                     # vit_som.py:84 (iteration BEFORE increment)
        return self._gamma_t(), float(self.som_layer.current_temperature)

    def _step(self, x, y, gamma_t: float, T: float):
        return _StepTape.step(self, x, y, gamma_t, T)

    def training_step(self, batch, batch_idx):
        """vit_som.py:80-105.  Returns a scalar tensor; ``.backward()`` runs the HIP backward."""
        x, y = batch
        self._estimated_steps()
        gamma_t, T = self._schedules_for_step()
        if self._anchor is None:
            self._anchor = torch.zeros((), device=self.arena.device, requires_grad=True)
        total = _StepLoss.apply(self._anchor, self, x, y, gamma_t, T)
        self._advance()
        if _HAVE_PL and getattr(self, "_trainer", None) is not None:          # vit_som.py:91,95-102
            main = "train/cls_loss" if self.classification else "train/recon_loss"
            self._log("hp/gamma", gamma_t)
            self._log({main: self._last["main"], "train/som_loss": self._last["som"], "train/total_loss": self._last["total"]})
        return total

    def train_step_fused(self, x, y):
        """Same step without the autograd bridge: forward + losses + backward into the gradient
        arena (the caller then runs optimizer.step()).  Returns the loss tensor."""
        self._estimated_steps()
        gamma_t, T = self._schedules_for_step()
        total, backward = self._step(x, y, gamma_t, T)
        backward()
        self._advance()
        return total

    def _advance(self):
        self._it += 1                                                   # the device buffer moved with the loss (_forward_losses)

    def validation_step(self, batch, batch_idx):
        """vit_som.py:107-125 (full gamma, current temperature, no schedule update)."""
        x, y = batch
        total = self._forward_losses(x, y, float(self.gamma), float(self.som_layer.current_temperature), want_grad=False)
        if self.classification:
            a = self._ctx[1]
            self._last["acc"] = (a.logits.argmax(dim=-1) == y.view(-1)).float().mean()
        if _HAVE_PL and getattr(self, "_trainer", None) is not None:          # vit_som.py:116-123
            main = "val/cls_loss" if self.classification else "val/recon_loss"
            logs = {main: self._last["main"], "val/som_loss": self._last["som"], "val/total_loss": self._last["total"]}
            if self.classification:
                logs["val/accuracy"] = self._last["acc"]
            self._log(logs)
        return total.clone()

    def configure_optimizers(self):
        """vit_som.py:127-163: AdamW/Adam (lr * batch_size / 256), reference param groups, per-epoch
        LambdaLR with the warm-up / cosine multiplier floored at min_lr."""
        hp = self.config["hyperparameters"]
        opt_hp = hp["optimizer"]
        groups = param_groups_lrd(self.vit, weight_decay=opt_hp["weight_decay"], layer_decay=opt_hp["layer_decay"])
        other = list(self.som_layer.parameters())
        if self.classification:
            other.extend(list(self.cls_head.parameters()))
        groups.append({"params": other})
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

    # -- checkpoints: Lightning's .ckpt layout --------------------------------------
    def save_checkpoint(self, path, optimizer=None, scheduler=None, epoch=0, global_step=None):
        """Write a file with the keys a Lightning ModelCheckpoint writes (train_vit_som.py:81-84):
        state_dict (reference key names), hyper_parameters (= the config dict, vit_som.py:26),
        optimizer_states / lr_schedulers, epoch, global_step."""
        ckpt = {
            "epoch": int(epoch), "global_step": int(self._it if global_step is None else global_step),
            "pytorch-lightning_version": "2.2.1", "hparams_name": "config",
            "state_dict": {k: v.detach().cpu().clone() for k, v in self.state_dict().items()},
            "hyper_parameters": self.config,
            "optimizer_states": [optimizer.state_dict()] if optimizer is not None else [],
            "lr_schedulers": [scheduler.state_dict()] if scheduler is not None else [],
        }
        for st in ckpt["optimizer_states"]:
            for s in st["state"].values():
                for k2 in ("exp_avg", "exp_avg_sq"):
                    s[k2] = s[k2].cpu()
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        torch.save(ckpt, path)
        return path

    @classmethod
    def load_from_checkpoint(cls, checkpoint_path, config=None, device=None, map_location=None):
        """ViTSOM.load_from_checkpoint(path, config=config) (train_vit_som.py:111).  Only loaders
        that execute nothing from the file are used (torch.load(weights_only=True))."""
        ckpt = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
        if config is None:
            config = ckpt.get("hyper_parameters")
            if config is None:
                raise ValueError("checkpoint carries no hyper_parameters; pass config=")
        model = cls(config, device=device)
        model.load_state_dict(ckpt["state_dict"])
        model._loaded_checkpoint = ckpt
        return model

    def on_train_end(self):                                             # vit_som.py:165-172
        print(f"Peak GPU memory usage: {torch.cuda.max_memory_allocated() / 1e9:.4f} GB")

    def get_latent_representation(self, x):
        """vit_som.py:174-187 (the reference unpacks 4 of 3 values; this returns what it meant)."""
        with torch.no_grad():
            cls_token, patches, _ = self.vit(x)
            return cls_token if self.use_reduced else patches.flatten(start_dim=1)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        key = prefix + "iteration"
        if key in state_dict:
            self._it = int(state_dict[key])
