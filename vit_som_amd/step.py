"""The fused training step's machinery, shared by every arena-owning model (ViTSOM, DESOM): the autograd bridge, the
launch tape, the library's RCCL communicator and the arena owner with its data-parallel exchange."""
import weakref
from typing import Optional

import torch

from . import ops
from ._lib import Event, on_stream, stream_wait_stream
from .arena import ParamArena
from .tuning import hooks


# ------------------------------------------------------------------------------------ autograd bridge
class _StepLoss(torch.autograd.Function):
    """Makes the fused step look like one differentiable scalar to torch / Lightning:
    forward = all HIP forward kernels + losses, backward = all HIP backward kernels writing the
    gradient arena.  The incoming scalar gradient multiplies the three loss-side seeds (dL/dpred,
    dL/dlogits, the SOM coefficients) BEFORE the backward kernels run -- the backward is linear in
    them -- so nothing touches the arena after the overlapped all-reduces have started."""

    @staticmethod
    def forward(ctx, anchor, model, x, y, gamma_t, T):
        ctx.model = model
        out, ctx.run_backward = model._step(x, y, gamma_t, T)
        ctx.forward_id = model._forward_id
        return out.clone()

    @staticmethod
    def backward(ctx, gout):
        m = ctx.model
        if ctx.forward_id != m._forward_id or m._seeds_consumed:
            raise RuntimeError("ViTSOM: backward() called twice for one training_step (or after a later forward): the "
                               "step's buffers and gradient seeds are single-use; gradient accumulation is not supported")
        m._seeds_consumed = True
        ctx.run_backward(gout)             # the seeds scaled by gout (1.0 under a plain loss.backward()), then the backward
        m._expose_grads()
        return None, None, None, None, None, None


class _StepTape:
    """A training step recorded on a launch tape (vsom_tape_*) while it runs; later steps re-issue its ~420 launches from C.
    Segments: 0 = forward up to the distances, 1 = main loss, 2 = loss-seed scaling (autograd bridge only), 3 = the whole
    backward.  The host issues the neighbourhood kernel and the loss combination in the holes between 0 | 1 | 2, with each
    step's temperature and gamma.  The third step of a batch size is recorded; inputs are staged into fixed buffers.

    The tape points into: the ViT activations `a`, which own it; the SOM buffers `s`; the arenas, the weight transposes and
    the frozen parameters, which only _apply / _pack move or rebuild, always with a new arena; the prototypes' plane image;
    ops.scratch blocks, grow-only with retired blocks kept alive, so they need no check.  `valid` compares the others by
    identity -- weak references, never id(), which CPython reuses -- and the switches, exchange and launch stream of the
    recording.  A tape that fails it is closed and the step recorded again."""

    @staticmethod
    def _key(m):
        return (ops.get_gemm_mode(), ops.get_attention_fused(), ops.get_wgrad_tiles(), ops.get_ln_tiles(), hooks.signature(), m.world_size, m._use_vsom_comm, ops.stream())

    @classmethod
    @torch.no_grad()
    def step(cls, m, x, y, gamma_t: float, T: float):
        """A training step's forward through the tape of its batch size -> (total, backward), like _ArenaOwner._step."""
        if not (hooks.launch_tape and x.is_cuda and (m.world_size == 1 or m._use_vsom_comm) and ops.tape_recording() == 0):
            return _ArenaOwner._step(m, x, y, gamma_t, T)
        x = m.vit._check_input(x)
        a = m.vit._buffers_for(x.shape[0], x.device)
        if not hasattr(a, "x_in"):
            a.x_in = torch.empty(a.B, m.vit.in_chans, m.vit.img_size, m.vit.img_size, dtype=torch.float32, device=a.device)
            a.y_in = torch.zeros(a.B, dtype=torch.int64, device=a.device)
            a.gout_in = torch.ones(1, dtype=torch.float32, device=a.device)
            a.steps_seen = 0
        xs, ys = a.x_in.copy_(x), a.y_in
        if m.classification:
            ys.copy_(y.view(-1))
        tape = a.__dict__.get("tape")
        if tape is not None and not tape.valid(m, a):
            tape.close()
            tape = a.tape = None
        if hooks.adamw_planes and m.som_layer._planes_shape_ok(a.B):
            m.som_layer._w_planes()                   # outside the tape: launches only when the optimizer-kept image is stale
        if tape is None:
            a.steps_seen += 1
            if a.steps_seen <= 2:                     # host-driven: scratch buffers and lazily built tables settle first
                return _ArenaOwner._step(m, xs, ys, gamma_t, T)
            tid = ops.tape_begin()
            try:
                total = m._forward_losses(xs, ys, gamma_t, T, want_grad=True)      # segments 0 | hole | 1 | hole | 2 ...
                a.gout_in.fill_(1.0)
                m._scale_seeds(a.gout_in)                                          # ... segment 2 (x 1.0: exact no-op)
                ops.tape_cut()
                m._backward()                                                      # segment 3
            except BaseException:
                ops.tape_end()
                ops.tape_destroy(tid)
                raise
            tape = a.tape = cls(tid, ops.tape_end(), m, a)
            # the recording ran the backward (seed 1); the autograd bridge replays it with its own seed
            return total, lambda gout=None: gout is not None and tape.backward(m, gout)
        # the host-side state a host-driven step leaves behind, then segment | hole | segment | hole
        s = tape.som_bufs
        a.version += 1
        m._ctx = (xs, a, s)
        m._forward_id, m._seeds_consumed = m._forward_id + 1, False
        total = tape.forward(lambda: m._call_neigh(s, gamma_t, T, a.B, True),
                             lambda: m._call_parts(a, s, gamma_t, T, a.B, xs.numel(), True))
        return total, lambda gout=None: tape.backward(m, gout)

    def __init__(self, tid, nseg, m, a):
        if nseg != 4:
            ops.tape_destroy(tid)
            raise RuntimeError(f"launch tape: expected 4 segments, recorded {nseg}")
        w = m.som_layer._wplanes
        self.id, self.key, self.gout_in, self.som_bufs = tid, self._key(m), a.gout_in, m._ctx[2]
        self.arena, self.planes = weakref.ref(m.arena), (lambda: None) if w is None else weakref.ref(w)
        self.started, self.comm_dirty = list(m._started), m._comm_dirty

    def valid(self, m, a) -> bool:
        return (self.key == self._key(m) and self.arena() is m.arena and self.planes() is m.som_layer._wplanes
                and self.som_bufs is m.som_layer._bufs.get(a.B))

    def forward(self, neigh, parts):
        """Segments 0 and 1, each followed by its host-issued call; returns what `parts` returns (the total loss)."""
        ops.tape_replay(self.id, 0)
        neigh()
        ops.tape_replay(self.id, 1)
        return parts()

    @torch.no_grad()
    def backward(self, m, gout=None):
        """Segment 3 (segment 2 first when a loss seed comes in), then the host-side state the recorded backward left."""
        m._grads_reduced = False
        m._exchange_reset()
        if gout is not None:
            self.gout_in.copy_(gout.detach().reshape(1))
            ops.tape_replay(self.id, 2)
        ops.tape_replay(self.id, 3)
        m._started, m._comm_dirty = list(self.started), self.comm_dirty

    def close(self):
        if self.id:
            ops.tape_destroy(self.id)
            self.id = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def init_vsom_comm(world_size: int, rank: int, unique_id: Optional[bytes] = None):
    """One RCCL communicator per process behind the C-ABI (vsom_comm_init).  The unique id comes from rank 0; with no
    `unique_id` given it travels over the torch.distributed process group the launcher set up (host-side plumbing)."""
    w, r = ops.comm_info()
    if w == world_size and r == rank:
        return
    if w != 0:
        ops.comm_destroy()
    if unique_id is None:
        if world_size == 1:
            unique_id = ops.comm_unique_id()
        else:
            import torch.distributed as dist
            box = [ops.comm_unique_id() if rank == 0 else None]
            dist.broadcast_object_list(box, src=0)
            unique_id = box[0]
    ops.comm_init(unique_id, world_size, rank)


def _vsom_comm_selftest(world_size: int, device) -> bool:
    """One small sum all-reduce through the library's communicator, checked against the closed form: rank r contributes
    r + 1 in every element, the sum is world (world + 1) / 2."""
    _, rank = ops.comm_info()
    buf = torch.full((1024,), float(rank + 1), dtype=torch.float32, device=device)
    ops.comm_allreduce_sum(buf)
    torch.cuda.synchronize(device)
    return bool((buf == world_size * (world_size + 1) / 2).all().item())


# ------------------------------------------------------------------------------------ arena owner
class _ArenaOwner:
    """What every model on this path shares: trainable tensors packed into flat arenas
    (arena.py), gradients exposed as views, and the data-parallel exchange over the gradient
    arena.  Subclasses may provide ``som_layer`` and override the two hooks."""

    arena: Optional[ParamArena] = None
    world_size, rank = 1, 0
    current_epoch = 0                            # Lightning's attribute; train.fit sets it (the plots' file names carry it)
    _grads_reduced = False
    _forward_id, _seeds_consumed = 0, False      # one backward per forward of the fused step (_StepLoss)

    def _default_weight_decay(self, name: str, p) -> float:
        return 0.0

    def _after_pack(self):
        pass

    @staticmethod
    def _default_device(device=None) -> torch.device:
        """`device`, else the current GPU when there is one, else the CPU."""
        if device is not None:
            return torch.device(device)
        return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")

    def _step_loss(self, x, y, gamma_t: float, T: float):
        """A training step through the autograd bridge: its loss as a scalar whose .backward() runs the HIP backward."""
        if self._anchor is None:
            self._anchor = torch.zeros((), device=self.arena.device, requires_grad=True)
        return _StepLoss.apply(self._anchor, self, x, y, gamma_t, T)

    def _step(self, x, y, gamma_t: float, T: float):
        """Forward + losses of a training step -> (total, backward); backward(gout=None) fills the gradient arena."""
        def backward(gout=None):
            if gout is not None:
                self._scale_seeds(gout)
            self._backward()
        return self._forward_losses(x, y, gamma_t, T, want_grad=True), backward

    def _named_trainable(self):
        return [(n, p) for n, p in self.named_parameters() if p.requires_grad]

    def _pack(self, device):
        """(Re)build the flat arenas on `device` and re-point every Parameter at its view."""
        old_wd = self.arena.wd_by_name if self.arena is not None else {}
        named = self._named_trainable()
        specs = []
        for n, p in named:
            wd = old_wd[n] if n in old_wd else self._default_weight_decay(n, p)
            specs.append((n, tuple(p.shape), wd))
        arena = ParamArena(specs, device)
        with torch.no_grad():
            for n, p in named:
                v = arena.p(n)
                v.copy_(p.detach().to(device))
                p.data = v
            for n, b in list(self.named_buffers()) + [(n, p) for n, p in self.named_parameters() if not p.requires_grad]:
                if b.device != device:
                    b.data = b.data.to(device)
        if self.arena is not None and self.arena.device == device:
            arena.exp_avg.copy_(self.arena.exp_avg)
            arena.exp_avg_sq.copy_(self.arena.exp_avg_sq)
        self.arena = arena
        self._anchor = None
        self._grad_views = {n: arena.g(n) for n, _ in named}
        self._after_pack()

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        dev = next(self.parameters()).device
        aliased = all(p.data_ptr() == self.arena.p(n).data_ptr() for n, p in self._named_trainable())
        if not aliased or dev != self.arena.device:
            self._pack(dev)
        return self

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        """The host counter `_it` (temperature, gamma ramp) follows a loaded `iteration` buffer, for every model that has one:
        the reference reads the buffer itself (vit_som.py:84, desom.py:113-118)."""
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        key = prefix + "iteration"
        if key in state_dict and "iteration" in self._buffers:
            self._it = int(state_dict[key])

    def _G(self, prefix: str):
        return lambda name: self._grad_views[prefix + name]

    def _expose_grads(self):
        for n, p in self._named_trainable():
            p.grad = self._grad_views[n]

    _use_vsom_comm = False

    def set_distributed(self, world_size: int, rank: int = 0, backend: Optional[str] = None):
        """backend: "rccl" = the library's own communicator (vsom_comm_*; the default on the GPU unless torch.distributed
        runs on gloo), "torch" = torch.distributed's all_reduce (gloo on CPU tensors, or its "nccl" = RCCL)."""
        self.world_size, self.rank = int(world_size), int(rank)
        som = getattr(self, "som_layer", None)          # ViTClassifier has none
        if som is not None:
            som._world_size = int(world_size)
        self._backend_defaulted = backend is None
        if backend is None:
            backend = "torch"
            if self.world_size > 1 and self.arena is not None and self.arena.grads.is_cuda:
                import torch.distributed as dist
                if dist.is_available() and dist.is_initialized() and dist.get_backend() != "gloo":
                    backend = "rccl"
        if backend not in ("rccl", "torch"):
            raise ValueError(f"set_distributed: unknown backend {backend!r}")
        self._use_vsom_comm = backend == "rccl"
        if self._use_vsom_comm:
            chosen_by_default = getattr(self, "_backend_defaulted", False)
            try:
                init_vsom_comm(self.world_size, self.rank)
                ok = self.world_size == 1 or _vsom_comm_selftest(self.world_size, self.arena.grads.device)
                err = None if ok else "self-test all-reduce gave a wrong sum"
            except Exception as e:                       # noqa: BLE001 -- a collective backend that does not come up
                if not chosen_by_default:
                    raise
                ok, err = False, repr(e)
            if chosen_by_default and self.world_size > 1:
                # every rank takes the same path: agree on it through the process group that is known to work
                import torch.distributed as dist
                flag = torch.tensor([1.0 if ok else 0.0], device=self.arena.grads.device)
                dist.all_reduce(flag, op=dist.ReduceOp.MIN)
                all_ok = bool(flag.item() > 0.5)
                if not all_ok:
                    import warnings
                    warnings.warn(f"vit_som_amd: the library's RCCL communicator did not come up on every rank ({err}); "
                                  f"the gradient exchange uses torch.distributed instead")
                    self._use_vsom_comm = False
                    if ops.comm_info()[0] != 0:
                        ops.comm_destroy()
            elif not ok:
                raise RuntimeError(f"set_distributed: vsom_comm {err}")

    # -- data-parallel exchange: sum all-reduce over the gradient arena, in pieces -----------------
    # Each piece is a contiguous arena slice whose gradients are final at a known point of the backward
    # pass: the [K, L] prototype accumulator right after the SOM backward (79 of 100 MB at CIFAR shapes),
    # the decoder after the decoder backward, the encoder in buckets of a few blocks in reverse layer
    # order.  A piece is issued from a stream of its own that first waits for the events of the streams
    # that wrote it (main chain + weight-gradient side stream), so the collective (RCCL runs it on its
    # own stream) overlaps the rest of the backward; allreduce_gradients() reduces what is left and
    # makes the consumer stream wait for every piece.  Under torch.distributed "nccl" == RCCL over xGMI.
    def _overlap_enabled(self) -> bool:
        return self.world_size > 1 and hooks.overlap_allreduce

    def _exchange_reset(self):
        """Forget the pieces of the previous exchange.  Pieces still in flight (a backward pass whose gradients were
        never consumed by allreduce_gradients() / optimizer.step()) are waited for first: the new backward is about
        to overwrite the arena slices they are reducing."""
        for w in getattr(self, "_works", ()):
            w.wait()
        if getattr(self, "_comm_dirty", False) and self.arena is not None and self.arena.grads.is_cuda:
            stream_wait_stream(None, self._comm)
        self._works, self._started, self._comm_dirty = [], [], False

    def _arena_span(self, first: str, last: str):
        """[lo, hi) of the arena slice from parameter `first` through parameter `last` (padded)."""
        lo = self.arena.offsets[first][0]
        off, n, _ = self.arena.offsets[last]
        return lo, off + (n + 255) // 256 * 256

    def _reduce_async(self, lo: int, hi: int, after=()):
        """Start the sum all-reduce of grads[lo:hi]; `after` = events the piece must wait for."""
        import torch.distributed as dist
        g = self.arena.grads
        if hi <= lo:
            return
        if g.is_cuda:
            comm = getattr(self, "_comm", None)
            if comm is None or comm.device != g.device:
                comm = self._comm = torch.cuda.Stream(device=g.device)
            for ev in after:
                ev.wait(comm)
            if self._use_vsom_comm:
                # the library's own RCCL communicator (vsom_comm_*): the collective is enqueued on `comm` like a kernel
                with on_stream(comm):
                    ops.comm_allreduce_sum(g[lo:hi])
                self._comm_dirty = True
            else:
                with torch.cuda.stream(comm):
                    self._works.append(dist.all_reduce(g[lo:hi], op=dist.ReduceOp.SUM, async_op=True))
        else:
            self._works.append(dist.all_reduce(g[lo:hi], op=dist.ReduceOp.SUM, async_op=True))
        self._started.append((lo, hi))

    def _reduce_early(self, lo: int, hi: int, streams=()):
        """Called inside the backward pass once grads[lo:hi] is final on the given streams."""
        if not self._overlap_enabled():
            return
        evs = []
        if self.arena.grads.is_cuda:
            for st in streams:
                evs.append(Event.pooled().record(st))
        self._reduce_async(lo, hi, evs)

    def allreduce_gradients(self):
        """Reduce every arena slice not yet in flight, then make the current stream wait for all pieces.
        Idempotent until the next backward pass; AdamW divides by world_size."""
        if self.world_size <= 1 or self._grads_reduced:
            return
        self._grads_reduced = True
        g = self.arena.grads
        if not hasattr(self, "_works"):
            self._exchange_reset()
        evs = []
        if g.is_cuda:
            evs.append(Event.pooled().record())     # current stream: every gradient is final here
        pos = 0
        for lo, hi in sorted(self._started) + [(g.numel(), g.numel())]:
            if lo > pos:
                self._reduce_async(pos, lo, evs)
            pos = max(pos, hi)
        self._exchange_reset()                  # torch "nccl" / vsom_comm: the current stream waits; gloo: the host does

    def broadcast_parameters(self, src: int = 0):
        """Replicas are built from the same seed; this makes it explicit (DDP broadcasts at construction)."""
        if self.world_size > 1:
            import torch.distributed as dist
            dist.broadcast(self.arena.params, src=src)
