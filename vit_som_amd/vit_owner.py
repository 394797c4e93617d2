"""What the two models built on ViTAutoencoder share (ViTSOM in model.py, ViTClassifier in classifier.py): the ViT and
cls_head built from the config, the transposed weight copies of the encoder's backward, the per-device stream pair, the
encoder buckets of the data-parallel exchange, the backward pass's frame, the loss ring, the optimizer and schedule,
and checkpoints.  What sits above the encoder -- the SOM and the decoder, or the pruned last block -- is the
subclass's: its forward, its losses, its part of the backward and its exchange buckets."""
import math
import os
from typing import Dict, Optional

import torch

from . import ops
from ._base import _HAVE_PL, _Acts, _Base
from ._lib import stream_wait_stream
from .optim import FusedAdamW, param_groups_lrd
from .step import _ArenaOwner
from .tuning import hooks
from .vit import ViTAutoencoder, _Affine, _BackwardSchedule

_LOSS_RING = 16     # the loss terms of a step stay readable until this many further steps have run
_STEP_STREAMS: Dict[int, tuple] = {}        # device index -> (side stream, SOM stream), shared by every model of the process


class _ViTOwner(_ArenaOwner, _Base):
    """A model whose trunk is a ViTAutoencoder, registered as the submodule `_vit_name` (also the reference's
    state_dict prefix).  Subclasses provide the forward and losses, `_head_buckets`, `_head_backward` and
    `_head_params`."""

    _vit_name = "vit"

    def __init__(self, config):
        super().__init__()
        # NOTE: unlike vit_som.py:23 / vit.py:249 this does NOT lower torch's global float32 matmul precision: every
        # contraction here is exact fp32 on MFMA.
        self.config = config
        if _HAVE_PL:
            self.save_hyperparameters(config)
        vit_hp, data_hp = config["hyperparameters"]["vit"], config["data"]
        setattr(self, self._vit_name, ViTAutoencoder(
            img_size=data_hp["input_size"], patch_size=vit_hp["patch_size"], in_chans=data_hp["num_channels"],
            embed_dim=vit_hp["emb_dim"], depth=vit_hp["depth"], num_heads=vit_hp["heads"],
            decoder_embed_dim=vit_hp["dec_emb_dim"], decoder_depth=vit_hp["dec_depth"],
            decoder_num_heads=vit_hp["heads"], mlp_ratio=vit_hp["mlp_ratio"], eps=1e-6))
        self._it = 0
        self._n_train: Optional[int] = None
        self._est_steps: Optional[int] = None
        self._last: Dict[str, torch.Tensor] = {}
        self._side_stream = self._som_stream = None
        self._sched: Optional[_BackwardSchedule] = None     # what the last host-driven backward pass ran with

    @property
    def _vit(self) -> ViTAutoencoder:
        return self._modules[self._vit_name]

    def _add_cls_head(self):
        """cls_head = nn.Linear(emb_dim, num_classes) with the reference's initialisation."""
        E, C = self._vit.embed_dim, self.config["data"]["num_classes"]
        self.cls_head = _Affine((C, E), (C,))
        with torch.no_grad():
            self.cls_head.weight.normal_(std=0.02)
            bound = 1.0 / math.sqrt(E)                                  # nn.Linear's default bias init
            self.cls_head.bias.uniform_(-bound, bound)

    # -- arenas -------------------------------------------------------------------------------
    def _default_weight_decay(self, name: str, p) -> float:
        if name.startswith(self._vit_name + "."):
            return 0.0 if p.ndim == 1 else 0.05
        return 0.01

    def _after_pack(self):
        self._build_weight_transposes()

    def _decoder_param_names(self):
        return [n for n, _ in self._named_trainable() if n.startswith(self._vit_name + ".decoder_")]

    def _build_weight_transposes(self):
        """Transposed copies W^T of the ViT Linear weights whose input gradient is needed, so that
        dX = dY W runs on the forward's kernel family (both operands contiguous along the reduction).
        One flat buffer + a device table; refreshed by ONE batched transpose per backward pass.  The
        decoder gets no gradient in classification mode and no copies either."""
        arena, dev = self.arena, self.arena.device
        unused = set(self._decoder_param_names()) if self.classification else set()
        rows, views, off = [], {}, 0
        for n, p in self._named_trainable():
            if not (n.startswith(self._vit_name + ".") and p.ndim == 2 and n.endswith(".weight")) or n in unused:
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

    # -- buffers and streams --------------------------------------------------------------------
    def _cls_view(self, buf: torch.Tensor, a: _Acts):
        """The B CLS rows of a [B*N, E] buffer, as a strided [B, E] view."""
        E = self._vit.embed_dim
        return torch.as_strided(buf, (a.B, E), (a.N * E, 1), buf.storage_offset())

    @staticmethod
    def _loss_buffers(buf: _Acts, device):
        """The main loss's device-side sum and the ring the step's loss terms land in, once per buffer set."""
        if not hasattr(buf, "main_sum"):
            buf.main_sum = torch.empty(1, dtype=torch.float32, device=device)
            buf.loss_ring = torch.zeros(_LOSS_RING, 4, dtype=torch.float32, device=device)
            buf.loss_slot = 0

    @staticmethod
    def _next_loss_slot(buf: _Acts):
        """The ring row for this step's loss terms: `_last` and the returned loss stay valid for the next
        _LOSS_RING - 1 steps (plain tensors: .get / `in` / ** all see them)."""
        buf.loss_slot = (buf.loss_slot + 1) % _LOSS_RING
        return buf.loss_ring[buf.loss_slot]

    def _ensure_streams(self, device):
        """The two extra HIP streams of the step (kept to two: a process has few hardware queues)."""
        if self._side_stream is None or self._side_stream.device != device:
            # one pair per device for the whole process: which hardware queue a stream lands on depends on how many
            # streams the process has created, and two of a model's streams on one queue serialise (measured: the 3rd, 5th
            # ... model of a process ran its step 1.4x slower at batch 128)
            key = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
            pair = _STEP_STREAMS.get(key)
            if pair is None:
                pair = _STEP_STREAMS[key] = (torch.cuda.Stream(device=device), torch.cuda.Stream(device=device))
            self._side_stream = pair[0]      # weight-gradient GEMMs; second forward chain
            self._som_stream = pair[1]       # SOM backward + early all-reduce; the prototypes' plane image in the forward

    def _log(self, *a, **k):
        """self.log / self.log_dict when a Lightning trainer is attached (vit_som.py:95-101); a no-op otherwise.
        Errors raised by Lightning's logger propagate."""
        if _HAVE_PL and getattr(self, "_trainer", None) is not None:
            self.log_dict(*a, **k) if isinstance(a[0], dict) else self.log(*a, **k)

    # -- backward ---------------------------------------------------------------------------------
    def _exchange_buckets(self):
        """Arena slices reduced early, in the order the backward finishes them: name -> (lo, hi)."""
        b = self.__dict__.get("_bucket_cache")
        if b is not None and b[0] is self.arena:
            return b[1]
        out = self._head_buckets()
        pre = self._vit_name
        D = len(self._vit.blocks)
        step = max(1, int(hooks.bucket_blocks))
        hi_name = f"{pre}.norm.bias"
        for i in range(D - step, 0, -step):                 # blocks [i, i + step) (+ the final norm for the top bucket)
            out[f"enc{i}"] = self._arena_span(f"{pre}.blocks.{i}.norm1.weight", hi_name)
            hi_name = f"{pre}.blocks.{i - 1}.mlp.2.bias"
        self.__dict__["_bucket_cache"] = (self.arena, out)
        return out

    def _zero_decoder_grads(self):
        """The decoder is not run in classification mode: its gradients are exactly zero (one fill over its contiguous
        arena slice)."""
        dec = self._decoder_param_names()
        if dec:
            lo, hi = self._arena_span(dec[0], dec[-1])
            ops.fill(self.arena.grads[lo:hi], 0.0)

    @torch.no_grad()
    def _backward(self):
        """All backward kernels; overwrites the whole gradient arena (no accumulation).  The pass's streams, deferred
        LayerNorm reductions, W^T copies and gradient views travel in one _BackwardSchedule.  The subclass's
        _head_backward(a, extra, sched, reduce) runs the part above the encoder, starting each of its buckets with
        reduce(name[, streams]), and returns the `depth` of ViTAutoencoder._encoder_bwd that is left: None for the
        whole encoder from dL/d(xe) in a.d_xe."""
        x, a, extra = self._ctx
        self._grads_reduced = False
        self._exchange_reset()
        side = None
        if hooks.side_stream:
            self._ensure_streams(x.device)
            side = self._side_stream
        Gv = self._G(self._vit_name + ".")
        self._refresh_weight_transposes()
        # the LayerNorm backwards leave their dgamma / dbeta reductions to one launch per exchange piece (or one in all)
        jobs = None
        if hooks.ln_reduce_batched:
            jobs = getattr(a, "ln_jobs", None)
            if jobs is None:
                jobs = a.ln_jobs = ops.LayerNormJobs(x.device)
            jobs.begin()
        buckets = self._exchange_buckets() if self._overlap_enabled() else {}
        main = torch.cuda.current_stream()
        sched = self._sched = _BackwardSchedule(Gv, side, jobs, self._WT)

        def flush():
            if jobs is not None:
                jobs.flush()

        def reduce(name, streams=None):
            """Start the early all-reduce of bucket `name`, if the exchange has one, once its gradients are final on
            `streams` (default: the main and the side stream)."""
            b = buckets.get(name)
            if b is not None:
                flush()
                if streams is None:
                    streams = [st for st in (main, side) if st is not None]
                self._reduce_early(*b, streams=streams)

        depth = self._head_backward(a, extra, sched, reduce)
        self._vit._encoder_bwd(a, sched, lambda i: reduce(f"enc{i}"), depth=depth)
        flush()
        if side is not None:
            stream_wait_stream(None, side)              # every gradient is final from here on
            sched.pending.clear()

    # -- reference API ----------------------------------------------------------------------------
    def configure_optimizers(self):
        """vit_som.py:127-163 / vit.py:304-336: AdamW/Adam (lr * batch_size / 256), the ViT's layer-decay groups plus one
        group of `_head_params()` (AdamW's default weight decay 0.01), per-epoch LambdaLR with the warm-up / cosine
        multiplier floored at min_lr."""
        hp = self.config["hyperparameters"]
        opt_hp = hp["optimizer"]
        groups = param_groups_lrd(self._vit, weight_decay=opt_hp["weight_decay"], layer_decay=opt_hp["layer_decay"])
        groups.append({"params": self._head_params()})
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
        if "iteration" not in model._buffers:
            model._it = int(ckpt.get("global_step", 0))          # no `iteration` buffer to restore the step count from
        model._loaded_checkpoint = ckpt
        return model

    def on_train_end(self):                                             # vit_som.py:165-172, vit.py:338-345
        print(f"Peak GPU memory usage: {torch.cuda.max_memory_allocated() / 1e9:.4f} GB")
