"""Host-side mirror of the reference's module surface for the ViT-SOM training-step hot path.

Classes keep the reference's names, constructor (the YAML-schema ``config`` dict), method
names, positional return tuples / dtypes and ``state_dict`` keys:

  ViTSOM          models/vit_som.py:17-187   forward / training_step / validation_step /
                                             configure_optimizers
  ViTAutoencoder  models/vit.py:66-240       forward / forward_features / patchify / unpatchify
                                             (vit.py)
  SOMLayer        models/som_layer.py:8-152  forward / compute_distances / update_temperature /
                                             compute_weights / som_loss / index_to_position (som.py)

What ViTSOM shares with ViTClassifier (the ViT, its W^T copies, streams, encoder buckets, the
backward's frame, optimizer and checkpoints) lives in vit_owner.py; FusedAdamW and
param_groups_lrd in optim.py; the fused step's autograd bridge, launch tape and arena owner,
shared with DESOM, in step.py.  All arithmetic runs in libvitsom_hip.so (hand-written gfx950
kernels) through ``ops``; these files only own memory (flat parameter arenas, activation
buffers), ordering, schedules and the data-parallel exchange (one RCCL all-reduce over the
gradient arena).  There is no CPU path.
"""
import torch

from . import ops
from ._base import _HAVE_PL, _Acts
from ._lib import Event, on_stream
from .som import SOMLayer
from .step import _StepTape
from .tuning import hooks
from .vit_owner import _ViTOwner


# ------------------------------------------------------------------------------------ ViT-SOM
class ViTSOM(_ViTOwner):
    """Vision Transformer Self-Organizing Map (models/vit_som.py:17-187), MI355X-native."""

    def __init__(self, config, device=None):
        super().__init__(config)
        hp = config["hyperparameters"]
        self.gamma = hp["gamma"]
        self.use_reduced = hp["som"]["use_reduced"]
        self.classification = config["data"]["num_classes"] > 0
        self.som_layer = SOMLayer(config)
        if self.classification:
            self._add_cls_head()
        self.smoothing = float(hp["optimizer"]["smoothing"])
        self.register_buffer("iteration", torch.tensor(0))
        self._som_done_ev = None    # the SOM backward's completion on its stream (_head_backward)
        self._pack(self._default_device(device))

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

    # -- fused forward + losses ---------------------------------------------------------------
    def _som_input(self, a: _Acts):
        E, N, B = self.vit.embed_dim, a.N, a.B
        if self.use_reduced:
            return torch.as_strided(a.xe, (B, E), (N * E, 1), a.xe.storage_offset())
        return torch.as_strided(a.xe, (B, (N - 1) * E), (N * E, 1), a.xe.storage_offset() + E)

    @torch.no_grad()
    def _run_forward(self, x, need_decoder: bool, fresh_w: bool = False):
        x = self.vit._check_input(x)
        if not x.is_cuda:
            raise ValueError("ViTSOM: input must live on the MI355X (there is no CPU path)")
        a = self.vit._buffers_for(x.shape[0], x.device)
        self._ensure_streams(x.device)
        # the prototypes' plane image for the BMU pass: re-split on the SOM stream while the encoder runs
        w_ready = self.som_layer._w_planes_async(self._som_stream, fresh_w) if self.som_layer._planes_shape_ok(a.B) else None
        self.vit._encode(x, a, self._side_stream)
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
        # the step.  The three values land in their own slot of the loss ring.
        K = self.som_layer.n_prototypes
        main_scale = 1.0 / B if self.classification else 1.0 / numel_x
        parts = self._next_loss_slot(a)
        ops.loss_parts(parts, a.main_sum, main_scale, s.loss_sum, gamma_t / (B * K), 1.0 / (B * K),
                       counter=self.iteration if want_grad else None)
        self._last = {"total": parts[0], "main": parts[1], "som": parts[2], "gamma_t": gamma_t, "T": T}
        return parts[0]

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

    @torch.no_grad()
    def _scale_seeds(self, gout):
        """Multiply the loss-side gradient seeds by the scalar `gout` (a 0-dim device tensor)."""
        _, a, s = self._ctx
        gout = gout.detach().reshape(1).float().contiguous()
        for buf in ((s.coef, s.row_dot, s.col_dot) + ((a.dlogits,) if self.classification else (a.dpred,))):
            ops.scale_by(buf, gout)

    def _head_buckets(self):
        """The prototypes, then (clustering only: in classification mode its gradients are zero) the decoder."""
        out = {"som": (self.arena.offsets["som_layer.prototypes"][0], self.arena.numel)}
        dec = self._decoder_param_names()
        if dec and not self.classification:
            out["decoder"] = self._arena_span(dec[0], dec[-1])
        return out

    def _head_params(self):
        return list(self.som_layer.parameters()) + (list(self.cls_head.parameters()) if self.classification else [])

    def _head_backward(self, a, s, sched, reduce):
        """The SOM, decoder and cls_head backwards; leaves dL/d(xe) in a.d_xe for the whole encoder."""
        X = self._som_input(a)
        E, N = self.vit.embed_dim, a.N
        if self.use_reduced:
            gX = torch.as_strided(a.d_xe, (a.B, E), (N * E, 1), a.d_xe.storage_offset())
        else:
            gX = torch.as_strided(a.d_xe, (a.B, (N - 1) * E), (N * E, 1), a.d_xe.storage_offset() + E)

        def som_backward(gx_out, accumulate):
            if self.som_layer._dist_mode == ops.DIST_MANHATTAN:
                ops.som_bwd_manhattan(X, self.som_layer.prototypes, s.coef, self._grad_views["som_layer.prototypes"], gx_out,
                                      accumulate_gx=accumulate)
            else:
                ops.som_bwd(X, self.som_layer.prototypes, s.coef, s.row_dot, s.col_dot,
                            self._grad_views["som_layer.prototypes"], gx_out, accumulate_gx=accumulate)

        side = self._som_stream if sched.side is not None else None
        if self.classification or side is None:
            if self.classification:
                ops.fill(a.d_xe, 0.0)
                self._zero_decoder_grads()
                ops.linear_bwd_weight(a.dlogits, self._cls_view(a.xe, a), self._grad_views["cls_head.weight"],
                                      self._grad_views["cls_head.bias"])
                ops.linear_bwd_input(a.dlogits, self.cls_head.weight, self._cls_view(a.d_xe, a), accumulate=True)
            else:
                self.vit._decoder_bwd(a, sched)
                reduce("decoder")
            som_backward(gX, True)
            reduce("som")
        else:
            # The SOM backward depends only on the forward (coef, X, W), so it runs on a stream of its
            # own under the decoder backward and writes its input gradient straight into (the zeroed)
            # d_xe; the decoder's last GEMM waits for it and accumulates on top.  The prototype
            # all-reduce is issued behind it: it starts the moment gW is final, before the decoder
            # backward has finished.
            sched._event().record().wait(side)
            with on_stream(side):
                ops.fill(a.d_xe, 0.0)
                som_backward(gX, False)
            reduce("som", [side])
            # a dedicated event: its wait is deferred to the end of the decoder backward, by which time a pooled
            # (round-robin) event could have been re-recorded for something else (deep decoders)
            if self._som_done_ev is None:
                self._som_done_ev = Event()
            som_done = self._som_done_ev.record(side)
            self.vit._decoder_bwd(a, sched, before_dxe=lambda: som_done.wait())
            reduce("decoder")
        return None

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
        total = self._step_loss(x, y, gamma_t, T)
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

    def attention_rollout(self, x, query=None, head_fusion="mean", residual=0.5, start_layer=0):
        """ViTAutoencoder.attention_rollout of the encoder -> [B, N].  query None: what the SOM is fed -- 'patches', or 'cls'
        when use_reduced is set."""
        if query is None:
            query = "cls" if self.use_reduced else "patches"
        return self.vit.attention_rollout(x, query, head_fusion, residual, start_layer)

    def get_latent_representation(self, x):
        """vit_som.py:174-187 (the reference unpacks 4 of 3 values; this returns what it meant)."""
        with torch.no_grad():
            cls_token, patches, _ = self.vit(x)
            return cls_token if self.use_reduced else patches.flatten(start_dim=1)
