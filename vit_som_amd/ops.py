"""Tensor-level wrappers over the C-ABI (one per entry point of include/vitsom_hip.h).

Every wrapper passes raw device pointers, row strides and torch's current HIP stream, and raises
``VsomError`` on a non-zero status.  Nothing here computes: there is no eager fallback.

This module is the only place that can tell a device pointer from a host pointer.  The training
step's wrappers (above the `evaluation` banner) check device, dtype and inner stride of their
matrices with ``_f32`` and the rest with ``assert``: the model owns every buffer it hands them.  The
evaluation wrappers (from that banner to the RCCL section) take tensors from callers: every tensor
whose address crosses into the library is checked there for device, dtype, layout and size by
``_matrix`` / ``_dense`` / ``_buffer``, None passes only where the docstring says optional, and a
refusal is a ``ValueError`` naming the argument, raised before anything is launched, ``python -O``
or not.  A buffer whose element count goes to the entry (a workspace, ``zpart``, ``part``) is sized
by the entry, which refuses a short one before it launches.  The agglomerative-clustering and DBSCAN
wrappers at the end of the module are evaluation wrappers under the same contract.
"""
from contextlib import contextmanager
from typing import Optional

import torch

from . import _lib as _lib_mod
from ._lib import check, lib, ptr, stream

_scratch = {}
_retired = []

# Optional per-op HIP-event timing (bench.py): name -> list of (start_event, end_event) recorded
# on torch's current stream, which is the stream every kernel here is launched on.
_timers = {}


def enable_timer(name: str):
    _timers[name] = []


def disable_timers():
    _timers.clear()


def timer_ms(name: str):
    """Average milliseconds per timed call (synchronises)."""
    ev = _timers.get(name, [])
    if not ev:
        return None
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in ev) / len(ev), len(ev)


def reset_timer(name: str):
    if name in _timers:
        _timers[name] = []


@contextmanager
def _timed(name: str):
    """An event pair around the launches of the block, on the stream they go to, when timer `name` is enabled."""
    rec = _timers.get(name)
    if rec is None:
        yield
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(_lib_mod.launch_torch_stream())
    yield
    e1.record(_lib_mod.launch_torch_stream())
    rec.append((e0, e1))


def scratch(nbytes: int, device) -> torch.Tensor:
    """Grow-only byte scratch per (device, stream): reuse is ordered by the stream the kernels run on
    (256-byte aligned by the allocator)."""
    key = (torch.device(device).index or 0, stream() if torch.device(device).type == "cuda" else 0)
    buf = _scratch.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is not None:
            # The old block may still be read by kernels queued on a side stream the caching allocator knows nothing
            # about (launches go to raw stream handles): never hand it back while the process lives (grow-only, a few
            # blocks per stream at most).
            _retired.append(buf)
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _scratch[key] = buf
    return buf


def _f32(t: torch.Tensor, name: str, inner_contig: bool = True):
    if not t.is_cuda:
        raise ValueError(f"{name}: expected a HIP device tensor (vit_som_amd has no CPU path)")
    if t.dtype != torch.float32:
        raise ValueError(f"{name}: expected float32, got {t.dtype}")
    if inner_contig and t.dim() >= 1 and t.numel() > 0 and t.stride(-1) != 1:
        raise ValueError(f"{name}: innermost stride must be 1")
    return t


def _rows(t: torch.Tensor) -> int:
    return t.stride(0) if t.dim() == 2 and t.shape[0] > 1 else t.shape[-1]


# The argument checks of the evaluation wrappers (everything below the `evaluation` banner): each tensor whose address goes
# to the library passes one of _matrix / _dense / _buffer first.  They raise ValueError, so they hold under `python -O`.
_Tensor, _I32, _I64, _F32, _F64, _U8 = torch.Tensor, torch.int32, torch.int64, torch.float32, torch.float64, torch.uint8


def _device(t, name, dtype):
    """Refuses what is not a tensor, not on the device or not of `dtype` (None: any): the first half of every refusal
    below, which test everything in one expression first because a loop of an estimator calls them every iteration."""
    if not isinstance(t, _Tensor):
        raise ValueError(f"{name}: expected a tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise ValueError(f"{name}: expected a HIP device tensor (vit_som_amd has no CPU path)")
    if dtype is not None and t.dtype != dtype:
        raise ValueError(f"{name}: expected {str(dtype)[6:]}, got {t.dtype}")


def _matrix(t, name, rows=None, cols=None, optional=False):
    """A row matrix: float32 on the device, 2-D, innermost stride 1, any row stride (a padded or guarded view passes), with
    `rows` / `cols` rows and columns where given -> (rows, cols, row stride); (0, 0, 0) for an optional None."""
    if t is None and optional:
        return 0, 0, 0
    if isinstance(t, _Tensor) and t.is_cuda and t.dtype == _F32 and t.dim() == 2:
        r, c = t.shape
        if (t.stride(1) == 1 or not t.numel()) and (rows is None or rows == r) and (cols is None or cols == c):
            return r, c, (t.stride(0) if r > 1 else c)
    _device(t, name, _F32)
    raise ValueError(f"{name}: expected a [{'any' if rows is None else rows}, {'any' if cols is None else cols}] matrix with "
                     f"innermost stride 1, got shape {tuple(t.shape)} with strides {t.stride()}")


def _dense(t, name, dtype, shape, optional=False):
    """A dense tensor: `dtype` on the device, contiguous (a storage offset is fine), of exactly `shape`: a tuple, None in it
    for an extent the tensor itself sets, or an int for that many elements in any shape.  -> t."""
    if t is None and optional:
        return t
    if isinstance(t, _Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous():
        if isinstance(shape, int):
            if t.numel() == shape:
                return t
        elif t.shape == shape:
            return t
        elif t.dim() == len(shape):
            for want, got in zip(shape, t.shape):
                if want is not None and want != got:
                    break
            else:
                return t
    _device(t, name, dtype)
    want = f"{shape} elements" if isinstance(shape, int) else f"shape {shape}"
    raise ValueError(f"{name}: expected a contiguous tensor of {want}, got shape {tuple(t.shape)} with strides {t.stride()}")


def _buffer(t, name, dtype, n=0, optional=False):
    """A buffer: `dtype` (None: any) on the device, contiguous, at least n elements (a longer one passes).  -> t."""
    if t is None and optional:
        return t
    if isinstance(t, _Tensor) and t.is_cuda and (dtype is None or t.dtype == dtype) and t.is_contiguous() and t.numel() >= n:
        return t
    _device(t, name, dtype)
    raise ValueError(f"{name}: expected a contiguous buffer of at least {n} elements, got shape {tuple(t.shape)} with strides "
                     f"{t.stride()}")


# ---------------------------------------------------------------- linear
def linear_fwd(x, W, bias, out):
    M, K = x.shape
    N = W.shape[0]
    _f32(x, "x"); _f32(W, "W"); _f32(out, "out")
    assert W.shape[1] == K and W.is_contiguous() and out.shape == (M, N)
    check(lib.vsom_linear_fwd(ptr(x), _rows(x), ptr(W), ptr(bias), ptr(out), _rows(out), M, N, K, stream()), "vsom_linear_fwd")
    return out


def linear_gelu_fwd(x, W, bias, grad, act):
    """grad <- gelu'(x W^T + b), act <- gelu(x W^T + b)."""
    pre = grad
    M, K = x.shape
    N = W.shape[0]
    _f32(x, "x"); _f32(W, "W")
    assert W.is_contiguous() and pre.is_contiguous() and act.is_contiguous() and pre.shape == (M, N) == act.shape
    check(lib.vsom_linear_gelu_fwd(ptr(x), _rows(x), ptr(W), ptr(bias), ptr(pre), ptr(act), M, N, K, stream()), "vsom_linear_gelu_fwd")
    return pre, act


def linear_relu_fwd(x, W, bias, ygrad, yact):
    """yact = relu(x W^T + b); ygrad = 1.0 where the pre-activation is positive (its derivative)."""
    M, K = x.shape
    N = W.shape[0]
    _f32(x, "x"); _f32(W, "W"); _f32(ygrad, "ygrad"); _f32(yact, "yact")
    assert W.is_contiguous() and W.shape[1] == K and ygrad.is_contiguous() and yact.is_contiguous()
    assert ygrad.shape == (M, N) and yact.shape == (M, N)
    check(lib.vsom_linear_relu_fwd(ptr(x), _rows(x), ptr(W), ptr(bias), ptr(ygrad), ptr(yact), M, N, K, stream()),
          "vsom_linear_relu_fwd")
    return yact


def l1_loss(pred, target, loss_sum, dpred=None, grad_scale=0.0):
    """loss_sum[0] = sum |pred - target|; dpred = grad_scale * sign(pred - target)."""
    assert pred.is_contiguous() and target.is_contiguous() and pred.numel() == target.numel()
    _f32(pred, "pred"); _f32(target, "target")
    n = pred.numel()
    ws = scratch(lib.vsom_l1_loss_workspace_bytes(n), pred.device)
    check(lib.vsom_l1_loss(ptr(pred), ptr(target), ptr(loss_sum), ptr(dpred), float(grad_scale), n, ptr(ws), ws.numel(),
                           stream()), "vsom_l1_loss")
    return loss_sum


def linear_residual_fwd(x, W, bias, R, r_mod, out):
    M, K = x.shape
    N = W.shape[0]
    _f32(x, "x"); _f32(W, "W"); _f32(R, "R"); _f32(out, "out")
    assert W.is_contiguous() and out.shape == (M, N) and R.shape[-1] == N
    check(lib.vsom_linear_residual_fwd(ptr(x), _rows(x), ptr(W), ptr(bias), ptr(R), _rows(R), int(r_mod), ptr(out),
                                       _rows(out), M, N, K, stream()), "vsom_linear_residual_fwd")
    return out


def linear_bwd_input(dy, W, dx, accumulate=False, gelu_grad=None):
    gelu_pre = gelu_grad
    M, N = dy.shape
    K = W.shape[1]
    _f32(dy, "dy"); _f32(W, "W"); _f32(dx, "dx")
    assert W.shape[0] == N and W.is_contiguous() and dx.shape == (M, K)
    if gelu_pre is not None:
        assert gelu_pre.is_contiguous() and gelu_pre.shape == (M, K)
    check(lib.vsom_linear_bwd_input(ptr(dy), _rows(dy), ptr(W), ptr(dx), _rows(dx), M, N, K, int(accumulate),
                                    ptr(gelu_pre), stream()), "vsom_linear_bwd_input")
    return dx


def linear_bwd_input_t(dy, Wt, dx, accumulate=False, gelu_grad=None):
    """dX (+)= dY * W from the transposed copy Wt[K,N] (see transpose_many)."""
    M, N = dy.shape
    K = Wt.shape[0]
    _f32(dy, "dy"); _f32(Wt, "Wt"); _f32(dx, "dx")
    assert Wt.shape[1] == N and Wt.is_contiguous() and dx.shape == (M, K)
    if gelu_grad is not None:
        assert gelu_grad.is_contiguous() and gelu_grad.shape == (M, K)
    check(lib.vsom_linear_bwd_input_t(ptr(dy), _rows(dy), ptr(Wt), ptr(dx), _rows(dx), M, N, K, int(accumulate),
                                      ptr(gelu_grad), stream()), "vsom_linear_bwd_input_t")
    return dx


def transpose_many(src_base, dst_base, table, max_rows, max_cols):
    """table: device int64 [count,4] rows {src_off, dst_off, rows, cols} (offsets in floats)."""
    _f32(src_base, "src_base"); _f32(dst_base, "dst_base")
    assert table.dtype == torch.int64 and table.is_contiguous() and table.ndim == 2 and table.shape[1] == 4
    assert table.device == src_base.device == dst_base.device
    check(lib.vsom_transpose_many(ptr(src_base), ptr(dst_base), table.data_ptr(), table.shape[0], int(max_rows),
                                  int(max_cols), stream()), "vsom_transpose_many")
    return dst_base


GEMM_F32, GEMM_SPLIT_BF16, GEMM_SPLIT_BF16_GRAD3 = 0, 1, 2      # include/vitsom_hip.h: VSOM_GEMM_*


def set_gemm_mode(mode: int):
    check(lib.vsom_set_gemm_mode(int(mode)), "vsom_set_gemm_mode")


def get_gemm_mode() -> int:
    return int(lib.vsom_get_gemm_mode())


def set_wgrad_tiles(mode):
    """Test / measurement hook (include/vitsom_hip.h, vsom_set_wgrad_tiles): 0 = 192 x 64 weight-gradient tiles, 1 = 192 x 192
    tiles at the 192 x 64 plan's split count (bitwise the same result), 2 = 192 x 192 tiles with their own plan (default)."""
    global _wgrad_tiles
    check(lib.vsom_set_wgrad_tiles(int(mode)), "vsom_set_wgrad_tiles")
    _wgrad_tiles = int(mode)


_wgrad_tiles = 2


def get_wgrad_tiles() -> int:
    """The value last set through set_wgrad_tiles (the library's default otherwise)."""
    return _wgrad_tiles


def set_ln_tiles(mode):
    """Test / measurement hook (include/vitsom_hip.h, vsom_set_ln_tiles) of the LayerNorm-fused input-gradient GEMM at the
    encoder width: 0 = 64 x 192 tiles, 1 = 192 x 192 tiles (default; bitwise the same dX and partials)."""
    global _ln_tiles
    check(lib.vsom_set_ln_tiles(int(mode)), "vsom_set_ln_tiles")
    _ln_tiles = int(mode)


_ln_tiles = 1


def get_ln_tiles() -> int:
    """The value last set through set_ln_tiles (the library's default otherwise)."""
    return _ln_tiles


def linear_bwd_weight(dy, x, dW, db):
    M, N = dy.shape
    K = x.shape[1]
    _f32(dy, "dy"); _f32(x, "x"); _f32(dW, "dW")
    assert x.shape[0] == M and dW.is_contiguous() and dW.numel() == N * K
    nbytes = lib.vsom_linear_bwd_weight_workspace_bytes(M, N, K)
    ws = scratch(nbytes, dy.device)
    check(lib.vsom_linear_bwd_weight(ptr(dy), _rows(dy), ptr(x), _rows(x), ptr(dW), ptr(db), M, N, K, ptr(ws), ws.numel(),
                                     stream()), "vsom_linear_bwd_weight")
    return dW, db


# ---------------------------------------------------------------- patch embedding
def patch_embed_fwd(img, Wpe, bpe, pos, cls_token, tokens, xp_ws, p):
    B, Cc, S, _ = img.shape
    E = Wpe.shape[0]
    for n_, t in (("img", img), ("Wpe", Wpe), ("tokens", tokens), ("xp_ws", xp_ws)):
        _f32(t, n_)
        assert t.is_contiguous(), n_
    check(lib.vsom_patch_embed_fwd(ptr(img), ptr(Wpe), ptr(bpe), ptr(pos), ptr(cls_token), ptr(tokens), ptr(xp_ws), B, Cc, S,
                                   p, E, stream()), "vsom_patch_embed_fwd")
    return tokens


def patch_embed_bwd(dtokens, xp_ws, dWpe, dbpe, dcls, B, Cc, S, p, E):
    assert dtokens.is_contiguous() and xp_ws.is_contiguous()
    nbytes = lib.vsom_patch_embed_bwd_workspace_bytes(B, Cc, S, p, E)
    ws = scratch(nbytes, dtokens.device)
    check(lib.vsom_patch_embed_bwd(ptr(dtokens), ptr(xp_ws), ptr(dWpe), ptr(dbpe), ptr(dcls), B, Cc, S, p, E, ptr(ws),
                                   ws.numel(), stream()), "vsom_patch_embed_bwd")


# ---------------------------------------------------------------- layernorm
def layernorm_fwd(x, gamma, beta, y, mean, rstd, eps=1e-6):
    rows, cols = x.shape
    assert x.is_contiguous() and y.is_contiguous()
    _f32(x, "x")
    check(lib.vsom_layernorm_fwd(ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd), rows, cols, float(eps), stream()),
          "vsom_layernorm_fwd")
    return y


def layernorm_bwd(dy, x, mean, rstd, gamma, resid, dx, dgamma, dbeta):
    rows, cols = x.shape
    assert dy.is_contiguous() and x.is_contiguous() and dx.is_contiguous() and (resid is None or resid.is_contiguous())
    nbytes = lib.vsom_layernorm_bwd_workspace_bytes(rows, cols)
    ws = scratch(nbytes, x.device)
    check(lib.vsom_layernorm_bwd(ptr(dy), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(resid), ptr(dx), ptr(dgamma),
                                 ptr(dbeta), rows, cols, ptr(ws), ws.numel(), stream()), "vsom_layernorm_bwd")
    return dx


class LayerNormJobs:
    """The LayerNorm backwards of one pass in deferred form: `bwd` computes dX and leaves the column partials in a buffer
    of its own, `flush` produces dgamma / dbeta for everything since the last flush in ONE launch (bit for bit what
    layernorm_bwd writes).  The job table is fixed after the first pass (same calls in the same order, same buffers);
    a call that does not match it (other shape, other order) starts a new table."""

    def __init__(self, device):
        self.device = device
        self.keys, self.rows_host, self.parts = [], [], []
        self.table = None               # int64 [njobs, 4] on the device, built once the first pass is complete
        self.n = self.flushed = 0
        self.max_cols = 0

    def begin(self):
        self.n = self.flushed = 0

    def _slot(self, key, dgamma, dbeta, cols, partial_bytes):
        """The partial buffer of the pass's next job: the table's when `key` matches it; else the table is forgotten
        from here on and a buffer of partial_bytes() bytes joins it."""
        i = self.n
        if i < len(self.keys) and self.keys[i] != key:           # the pass changed
            del self.keys[i:], self.rows_host[i:], self.parts[i:]
            self.table = None
        if i == len(self.keys):
            nbytes = partial_bytes()
            part = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self.keys.append(key); self.parts.append(part)
            self.rows_host.append([ptr(part), ptr(dgamma), ptr(dbeta), ((nbytes // (8 * cols)) << 32) | cols])
            self.max_cols = max(self.max_cols, cols)
            self.table = None
        self.n += 1
        return self.parts[i]

    def bwd(self, dy, x, mean, rstd, gamma, resid, dx, dgamma, dbeta):
        rows, cols = x.shape
        part = self._slot((ptr(dgamma), ptr(dbeta), rows, cols), dgamma, dbeta, cols,
                          lambda: lib.vsom_layernorm_bwd_workspace_bytes(rows, cols))
        check(lib.vsom_layernorm_bwd_partial(ptr(dy), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(resid), ptr(dx), rows, cols,
                                             ptr(part), part.numel(), stream()), "vsom_layernorm_bwd_partial")
        return dx

    def bwd_linear_fused(self, dy, Wt, x, mean, rstd, gamma, resid, dx, dgamma, dbeta):
        """dX of the Linear whose input-gradient GEMM (dy, Wt) feeds this LayerNorm's dY, in one launch
        (linear_bwd_input_ln_partial); one job of the table, like `bwd`."""
        rows, cols = x.shape
        part = self._slot((ptr(dgamma), ptr(dbeta), rows, cols, "fused"), dgamma, dbeta, cols,
                          lambda: lib.vsom_linear_bwd_input_ln_partial_bytes(rows, cols))
        linear_bwd_input_ln_partial(dy, Wt, x, mean, rstd, gamma, resid, dx, part)
        return dx

    def flush(self):
        if self.n == self.flushed:
            return
        if self.table is None or self.table.shape[0] < self.n:
            self.table = torch.tensor(self.rows_host, dtype=torch.int64, device=self.device)
        check(lib.vsom_layernorm_bwd_finish_many(ptr(self.table), self.flushed, self.n - self.flushed, self.max_cols, stream()),
              "vsom_layernorm_bwd_finish_many")
        self.flushed = self.n


def layernorm_bwd_deferrable(rows: int, cols: int) -> bool:
    return bool(lib.vsom_layernorm_bwd_deferrable(int(rows), int(cols)))


# ---------------------------------------------------------------- input-gradient GEMM + LayerNorm backward
def linear_bwd_input_ln_supported(rows: int, n: int, cols: int) -> bool:
    """Whether linear_bwd_input_ln takes dY[rows, n] -> LayerNorm width `cols` in the current GEMM mode."""
    return bool(lib.vsom_linear_bwd_input_ln_supported(int(rows), int(n), int(cols)))


def _ln_fused_args(dy, Wt, x, mean, rstd, gamma, resid, dx):
    M, N = dy.shape
    K = Wt.shape[0]
    for n_, t in (("dy", dy), ("Wt", Wt), ("x", x), ("dx", dx)):
        _f32(t, n_)
    assert Wt.shape[1] == N and Wt.is_contiguous() and x.shape == (M, K) == dx.shape and x.is_contiguous() and dx.is_contiguous()
    assert resid is None or (resid.is_contiguous() and resid.shape == (M, K))
    return (ptr(dy), _rows(dy), ptr(Wt), M, N, K, ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(resid), ptr(dx))


def linear_bwd_input_ln(dy, Wt, x, mean, rstd, gamma, resid, dx, dgamma, dbeta):
    """dx = resid + LayerNorm_bwd(dy Wt^T) with dgamma / dbeta, in one GEMM launch plus the column reduction: bit for bit
    linear_bwd_input_t into scratch followed by layernorm_bwd for dx; dgamma / dbeta to rounding."""
    args = _ln_fused_args(dy, Wt, x, mean, rstd, gamma, resid, dx)
    ws = scratch(lib.vsom_linear_bwd_input_ln_partial_bytes(x.shape[0], x.shape[1]), x.device)
    check(lib.vsom_linear_bwd_input_ln(*args, ptr(dgamma), ptr(dbeta), ptr(ws), ws.numel(), stream()), "vsom_linear_bwd_input_ln")
    return dx


def linear_bwd_input_ln_partial(dy, Wt, x, mean, rstd, gamma, resid, dx, part):
    """The same leaving the dgamma / dbeta partials in `part` for layernorm_bwd_finish_many (LayerNormJobs)."""
    args = _ln_fused_args(dy, Wt, x, mean, rstd, gamma, resid, dx)
    check(lib.vsom_linear_bwd_input_ln_partial(*args, ptr(part), part.numel(), stream()), "vsom_linear_bwd_input_ln_partial")
    return dx


# ---------------------------------------------------------------- attention
def attention_fwd(qkv, out, lse, B, N, H, hd):
    assert qkv.is_contiguous() and out.is_contiguous() and lse.is_contiguous()
    _f32(qkv, "qkv")
    check(lib.vsom_attention_fwd(ptr(qkv), ptr(out), ptr(lse), B, N, H, hd, stream()), "vsom_attention_fwd")
    return out


def attention_bwd(qkv, out, dout, lse, dqkv, delta, B, N, H, hd):
    assert all(t.is_contiguous() for t in (qkv, out, dout, lse, dqkv, delta))
    check(lib.vsom_attention_bwd(ptr(qkv), ptr(out), ptr(dout), ptr(lse), ptr(dqkv), ptr(delta), B, N, H, hd, stream()),
          "vsom_attention_bwd")
    return dqkv


def attention_probs(qkv, lse, probs, B, N, H, hd):
    """probs[B,H,N,N] = softmax(q k^T / sqrt(hd)) from qkv, each row normalised by its own scores (attention maps,
    vit.py:41-42); `lse` is kept in the signature and must be a device tensor, but is no longer read."""
    assert qkv.is_contiguous() and lse.is_contiguous() and probs.is_contiguous() and probs.shape == (B, H, N, N)
    _f32(qkv, "qkv"); _f32(probs, "probs")
    check(lib.vsom_attention_probs(ptr(qkv), ptr(lse), ptr(probs), B, N, H, hd, stream()), "vsom_attention_probs")
    return probs


def attention_q1_fwd(q, kv, out, lse, B, N, H, hd):
    """Single-query attention (the CLS row): q[B,E], kv[B*N,2E] (K then V) -> out[B,E], lse[B,H]."""
    assert all(t.is_contiguous() for t in (q, kv, out, lse))
    _f32(q, "q"); _f32(kv, "kv"); _f32(out, "out"); _f32(lse, "lse")
    check(lib.vsom_attention_q1_fwd(ptr(q), ptr(kv), ptr(out), ptr(lse), B, N, H, hd, stream()), "vsom_attention_q1_fwd")
    return out


def attention_q1_bwd(dout, out, lse, q, kv, dq, dkv, B, N, H, hd):
    """dq[B,E], dkv[B*N,2E] of attention_q1_fwd; every element written."""
    assert all(t.is_contiguous() for t in (dout, out, lse, q, kv, dq, dkv))
    _f32(dout, "dout"); _f32(q, "q"); _f32(kv, "kv"); _f32(dq, "dq"); _f32(dkv, "dkv")
    check(lib.vsom_attention_q1_bwd(ptr(dout), ptr(out), ptr(lse), ptr(q), ptr(kv), ptr(dq), ptr(dkv), B, N, H, hd, stream()),
          "vsom_attention_q1_bwd")
    return dq, dkv


def rows_add(src, dst):
    """dst += src over [rows, cols] views with any row stride (e.g. the CLS rows of a [B*N, E] buffer)."""
    rows, cols = src.shape
    _f32(src, "src"); _f32(dst, "dst")
    assert dst.shape == (rows, cols)
    check(lib.vsom_rows_add(ptr(src), _rows(src), ptr(dst), _rows(dst), rows, cols, stream()), "vsom_rows_add")
    return dst


# ---------------------------------------------------------------- SOM
def row_inv_norm(x, out, eps=1e-12):
    rows, cols = x.shape
    _f32(x, "x")
    check(lib.vsom_row_inv_norm(ptr(x), _rows(x), rows, cols, float(eps), ptr(out), stream()), "vsom_row_inv_norm")
    return out


DIST_COSINE, DIST_EUCLIDEAN, DIST_MANHATTAN = 0, 1, 2


def row_sqnorm(x, out):
    rows, cols = x.shape
    _f32(x, "x")
    check(lib.vsom_row_sqnorm(ptr(x), _rows(x), rows, cols, ptr(out), stream()), "vsom_row_sqnorm")
    return out


def _bmu_args(x, W, dist, bmu, inv_nx=None, inv_nw=None, reranked=None):
    """The argument checks every BMU wrapper shares -> (B, K, L).  inv_nx / inv_nw / reranked: what the three-product forms
    write beside dist and bmu."""
    B, L = x.shape
    K = W.shape[0]
    _f32(x, "x"); _f32(W, "W")
    assert W.is_contiguous() and W.shape[1] == L and bmu.dtype == torch.int64 and (dist is None or dist.is_contiguous())
    if inv_nx is not None:
        _f32(inv_nx, "inv_nx"); _f32(inv_nw, "inv_nw")
        assert reranked is None or (reranked.dtype == torch.int32 and reranked.is_cuda)
    return B, K, L


def bmu_euclid_fwd(x, W, sq_x, sq_w, dist: Optional[torch.Tensor], bmu):
    B, K, L = _bmu_args(x, W, dist, bmu)
    nbytes = lib.vsom_bmu_cosine_workspace_bytes(B, K, L)
    ws = scratch(nbytes, x.device)
    check(lib.vsom_bmu_euclid_fwd(ptr(x), _rows(x), ptr(W), ptr(sq_x), ptr(sq_w), ptr(dist), ptr(bmu), B, K, L, ptr(ws),
                                  ws.numel(), stream()), "vsom_bmu_euclid_fwd")
    return dist, bmu


def bmu_manhattan_fwd(x, W, dist: Optional[torch.Tensor], bmu):
    B, K, L = _bmu_args(x, W, dist, bmu)
    ws = scratch(lib.vsom_bmu_manhattan_workspace_bytes(B, K, L), x.device)
    check(lib.vsom_bmu_manhattan_fwd(ptr(x), _rows(x), ptr(W), ptr(dist), ptr(bmu), B, K, L, ptr(ws), ws.numel(), stream()),
          "vsom_bmu_manhattan_fwd")
    return dist, bmu


def som_bwd_manhattan(x, W, coef, gW, gX, accumulate_gx=True):
    B, L = x.shape
    K = W.shape[0]
    assert W.is_contiguous() and coef.is_contiguous() and gW.is_contiguous()
    check(lib.vsom_som_bwd_manhattan(ptr(x), _rows(x), ptr(W), ptr(coef), ptr(gW), ptr(gX), _rows(gX), int(accumulate_gx),
                                     B, K, L, stream()), "vsom_som_bwd_manhattan")


# The cosine BMU pass has three forms (include/vitsom_hip.h: VSOM_BMU_*); vsom_bmu_cosine_form names the one the library's
# launch plan chooses for a shape (SOMLayer._bmu_form asks), the three wrappers below run one each.
BMU_EXACT, BMU_X3, BMU_X3_PLANES = 0, 1, 2


def bmu_cosine_x3_fwd(x, W, dist: Optional[torch.Tensor], bmu, inv_nx, inv_nw, reranked: Optional[torch.Tensor] = None):
    """Cosine BMU pass (norms + three-product bf16 contraction + exact re-rank) -> dist, bmu, inv_nx, inv_nw.
    `reranked`: optional int32 device scalar counting the rows whose minimum had to be re-ranked."""
    B, K, L = _bmu_args(x, W, dist, bmu, inv_nx, inv_nw, reranked)
    nbytes = lib.vsom_bmu_cosine_x3_workspace_bytes(B, K, L)
    ws = scratch(nbytes, x.device)
    with _timed("bmu_cosine_dots"):
        check(lib.vsom_bmu_cosine_x3_dots(ptr(x), _rows(x), ptr(W), B, K, L, ptr(ws), ws.numel(), stream()), "vsom_bmu_cosine_x3_dots")
    check(lib.vsom_bmu_cosine_x3_finalize(ptr(x), _rows(x), ptr(W), ptr(ws), ws.numel(), ptr(dist), ptr(bmu), ptr(inv_nx),
                                          ptr(inv_nw), ptr(reranked), B, K, L, stream()), "vsom_bmu_cosine_x3_finalize")
    return dist, bmu


def bmu_planes_supported(B: int, K: int, L: int) -> bool:
    """Does the pre-split ("planes") form of the cosine BMU pass cover this shape?"""
    return bool(lib.vsom_bmu_cosine_x3_planes_supported(int(B), int(K), int(L)))


def bmu_planes_alloc(R: int, L: int, device) -> torch.Tensor:
    """Plane buffer of an operand [R, L] (fragment image + squared-norm partials)."""
    return torch.empty(lib.vsom_bmu_planes_bytes(int(R), int(L)), dtype=torch.uint8, device=device)


def bmu_planes_from(src, planes):
    """Split the fp32 operand `src` [R, L] (rows 16-byte aligned) into its plane buffer."""
    R, L = src.shape
    _f32(src, "src")
    assert src.stride(1) == 1 and planes.dtype == torch.uint8
    check(lib.vsom_bmu_planes_from(ptr(src), _rows(src), R, L, ptr(planes), planes.numel(), stream()), "vsom_bmu_planes_from")
    return planes


def bmu_cosine_x3_planes_fwd(x, W, xplanes, wplanes, dist: Optional[torch.Tensor], bmu, inv_nx, inv_nw,
                             reranked: Optional[torch.Tensor] = None):
    """bmu_cosine_x3_fwd on pre-split operands: `xplanes` / `wplanes` must describe `x` / `W` as they are now (x and W
    themselves feed the exact re-rank)."""
    B, K, L = _bmu_args(x, W, dist, bmu, inv_nx, inv_nw, reranked)
    nbytes = lib.vsom_bmu_cosine_x3_planes_workspace_bytes(B, K, L)
    if nbytes == 0:
        raise ValueError(f"bmu_cosine_x3_planes_fwd: shape B={B} K={K} L={L} is not covered by the planes form")
    ws = scratch(nbytes, x.device)
    with _timed("bmu_cosine_dots"):
        check(lib.vsom_bmu_cosine_x3_planes_dots(ptr(xplanes), ptr(wplanes), B, K, L, ptr(ws), ws.numel(), stream()),
              "vsom_bmu_cosine_x3_planes_dots")
    check(lib.vsom_bmu_cosine_x3_planes_finalize(ptr(x), _rows(x), ptr(W), ptr(xplanes), ptr(wplanes), ptr(ws), ws.numel(),
                                                 ptr(dist), ptr(bmu), ptr(inv_nx), ptr(inv_nw), ptr(reranked), B, K, L, stream()),
          "vsom_bmu_cosine_x3_planes_finalize")
    return dist, bmu


def bmu_cosine_fwd(x, W, inv_nx, inv_nw, dist: Optional[torch.Tensor], bmu):
    B, K, L = _bmu_args(x, W, dist, bmu)
    nbytes = lib.vsom_bmu_cosine_workspace_bytes(B, K, L)
    ws = scratch(nbytes, x.device)
    with _timed("bmu_cosine_dots"):
        check(lib.vsom_bmu_cosine_dots(ptr(x), _rows(x), ptr(W), B, K, L, ptr(ws), ws.numel(), stream()), "vsom_bmu_cosine_dots")
    check(lib.vsom_bmu_cosine_finalize(ptr(ws), ws.numel(), ptr(inv_nx), ptr(inv_nw), ptr(dist), ptr(bmu), B, K, L, stream()),
          "vsom_bmu_cosine_finalize")
    return dist, bmu


def som_neigh_loss(dist, bmu, grid, T, loss_sum, h=None, inv_nx=None, inv_nw=None, grad_scale=0.0, coef=None,
                   row_dot=None, col_dot=None, distance=DIST_COSINE):
    B, K = dist.shape
    assert dist.is_contiguous() and grid.is_contiguous() and bmu.dtype == torch.int64
    nbytes = lib.vsom_som_neigh_workspace_bytes(B, K)
    ws = scratch(nbytes, dist.device)
    check(lib.vsom_som_neigh_loss(ptr(dist), ptr(bmu), ptr(grid), float(T), ptr(inv_nx), ptr(inv_nw), float(grad_scale),
                                  ptr(h), ptr(loss_sum), ptr(coef), ptr(row_dot), ptr(col_dot), B, K, int(distance), ptr(ws), ws.numel(),
                                  stream()), "vsom_som_neigh_loss")
    return loss_sum


def som_bwd(x, W, coef, row_dot, col_dot, gW, gX, accumulate_gx=True):
    B, L = x.shape
    K = W.shape[0]
    assert W.is_contiguous() and coef.is_contiguous() and gW.is_contiguous()
    check(lib.vsom_som_bwd(ptr(x), _rows(x), ptr(W), ptr(coef), ptr(row_dot), ptr(col_dot), ptr(gW), ptr(gX), _rows(gX),
                           int(accumulate_gx), B, K, L, stream()), "vsom_som_bwd")


# ---------------------------------------------------------------- losses
def l1_unpatchify(pred, img, loss_sum, recon=None, dpred=None, grad_scale=0.0, p=1):
    B, Cc, S, _ = img.shape
    assert pred.is_contiguous() and img.is_contiguous()
    nbytes = lib.vsom_l1_unpatchify_workspace_bytes(B, Cc, S, p)
    ws = scratch(nbytes, img.device)
    check(lib.vsom_l1_unpatchify(ptr(pred), ptr(img), ptr(recon), ptr(loss_sum), ptr(dpred), float(grad_scale), B, Cc, S, p,
                                 ptr(ws), ws.numel(), stream()), "vsom_l1_unpatchify")
    return loss_sum


def cross_entropy_ls(logits, y, smoothing, loss_sum, dlogits=None, grad_scale=0.0):
    B, Cn = logits.shape
    assert logits.is_contiguous() and y.dtype == torch.int64
    nbytes = lib.vsom_cross_entropy_ls_workspace_bytes(B)
    ws = scratch(nbytes, logits.device)
    check(lib.vsom_cross_entropy_ls(ptr(logits), ptr(y), float(smoothing), ptr(loss_sum), ptr(dlogits), float(grad_scale), B,
                                    Cn, ptr(ws), ws.numel(), stream()), "vsom_cross_entropy_ls")
    return loss_sum


# ---------------------------------------------------------------- optimiser / utilities
def adamw_step(p, g, m, v, wd_chunk, lr, beta1, beta2, eps, step, grad_scale=1.0, adamw=True, planes=None):
    """One AdamW / Adam step over the flat arena.  `planes` = (element offset, R, L, plane buffer) of a [R, L] parameter
    whose BMU plane image is rewritten from the updated values in the same pass."""
    n = p.numel()
    if planes is not None:
        off, R, L, buf = planes
        check(lib.vsom_adamw_step_planes(ptr(p), ptr(g), ptr(m), ptr(v), ptr(wd_chunk), n, float(lr), float(beta1), float(beta2),
                                         float(eps), int(step), float(grad_scale), int(adamw), int(off), int(R), int(L), ptr(buf),
                                         buf.numel(), stream()), "vsom_adamw_step_planes")
        return
    check(lib.vsom_adamw_step(ptr(p), ptr(g), ptr(m), ptr(v), ptr(wd_chunk), n, float(lr), float(beta1), float(beta2),
                              float(eps), int(step), float(grad_scale), int(adamw), stream()), "vsom_adamw_step")


def fill(t, value):
    check(lib.vsom_fill(ptr(t), t.numel(), float(value), stream()), "vsom_fill")
    return t


def set_attention_fused(fused):
    """Test / measurement hook (include/vitsom_hip.h, vsom_set_attention_fused): False (0) runs the short-sequence attention
    backward as two launches, True (1) is the default (one launch, scores shared between its phases where the shape allows;
    at hd = 64 in the default GEMM mode its products run on the two-piece bf16 split), 2 = one launch with recomputed
    scores, 3 = 1 with fp32 products in every GEMM mode."""
    global _attention_fused
    check(lib.vsom_set_attention_fused(int(fused)), "vsom_set_attention_fused")
    _attention_fused = int(fused)


_attention_fused = 1


def get_attention_fused() -> int:
    """The value last set through set_attention_fused (the library's default otherwise)."""
    return _attention_fused


def scaled_mul(out, a, b=None, scale_dev=None, factor=1.0):
    """out = factor * scale_dev[0] * a * b  (b / scale_dev optional)."""
    _f32(out, "out"); _f32(a, "a")
    assert out.is_contiguous() and a.is_contiguous() and out.numel() == a.numel() and (b is None or (b.is_contiguous() and b.numel() == a.numel()))
    check(lib.vsom_scaled_mul(ptr(out), ptr(a), ptr(b), a.numel(), ptr(scale_dev), float(factor), stream()), "vsom_scaled_mul")
    return out


def som_weighted_loss(dist, weights, loss_sum, inv_nx=None, inv_nw=None, grad_scale=0.0, coef=None, row_dot=None, col_dot=None,
                      distance=0):
    """loss_sum <- sum(weights * dist) (+ backward coefficients of grad_scale * that sum when coef etc. are given)."""
    B, K = dist.shape
    _f32(dist, "dist"); _f32(weights, "weights")
    assert dist.is_contiguous() and weights.is_contiguous() and weights.shape == dist.shape
    nbytes = lib.vsom_som_neigh_workspace_bytes(B, K)
    ws = scratch(nbytes, dist.device)
    check(lib.vsom_som_weighted_loss(ptr(dist), ptr(weights), ptr(inv_nx), ptr(inv_nw), float(grad_scale), ptr(loss_sum), ptr(coef),
                                     ptr(row_dot), ptr(col_dot), B, K, int(distance), ptr(ws), ws.numel(), stream()),
          "vsom_som_weighted_loss")
    return loss_sum


def lincomb2(out, a, ca, b, cb, counter=None):
    """out[0] = ca * a[0] + cb * b[0] (device scalars); `counter` (a 0-dim int64 device tensor) += 1 in the same launch."""
    if counter is not None:
        assert counter.dtype == torch.int64 and counter.is_cuda and counter.numel() == 1
    check(lib.vsom_lincomb2(ptr(out), ptr(a), float(ca), ptr(b), float(cb), None if counter is None else counter.data_ptr(), stream()),
          "vsom_lincomb2")
    return out


def loss_parts(parts, main_sum, main_scale, som_sum, som_coef, som_scale, counter=None):
    """parts[0:3] = (total, main term, SOM term) of the step; `counter` += 1 in the same launch (see lincomb2)."""
    if counter is not None:
        assert counter.dtype == torch.int64 and counter.is_cuda and counter.numel() == 1
    _f32(parts, "parts")
    assert parts.numel() >= 3 and parts.is_contiguous()
    check(lib.vsom_loss_parts(ptr(parts), ptr(main_sum), float(main_scale), ptr(som_sum), float(som_coef), float(som_scale),
                              None if counter is None else counter.data_ptr(), stream()), "vsom_loss_parts")
    return parts


def scale_by(t, scale_dev):
    """t *= scale_dev[0] (device scalar, no host sync)."""
    _f32(t, "t"); _f32(scale_dev, "scale")
    assert t.is_contiguous() and scale_dev.numel() == 1
    check(lib.vsom_scale_by(ptr(t), t.numel(), ptr(scale_dev), stream()), "vsom_scale_by")
    return t


def reduce_slabs(slabs, out):
    nslabs, n = slabs.shape
    check(lib.vsom_reduce_slabs(ptr(slabs), slabs.stride(0), nslabs, ptr(out), n, stream()), "vsom_reduce_slabs")
    return out


# ---------------------------------------------------------------- evaluation
def contingency(a, b, table, bad):
    """table[a[i], b[i]] += 1 (a, b: contiguous int64 device tensors of one size; table is [na, nb] int64, accumulated;
    bad int32 [1] counts the pairs outside it)."""
    n = _buffer(a, "a", _I64).numel()
    _dense(b, "b", _I64, n)
    na, nb = _dense(table, "table", _I64, (None, None)).shape
    _dense(bad, "bad", _I32, 1)
    check(lib.vsom_contingency(ptr(a), ptr(b), n, na, nb, ptr(table), ptr(bad), stream()), "vsom_contingency")
    return table


def argmax_rows(x, out):
    """out int64 [rows] = the first argmax of every row of x f32 [rows, cols] (any row stride)."""
    rows, cols, ldx = _matrix(x, "x")
    _dense(out, "out", _I64, rows)
    check(lib.vsom_argmax_rows(ptr(x), ldx, rows, cols, ptr(out), stream()), "vsom_argmax_rows")
    return out


def proto_mosaic(pred, n, p, C, k0, map_size, images=None, canvas=None, gap=1):
    """Decoder output `pred` [chunk * (n + 1), p*p*C] -> images[k0 : k0 + chunk] ([K, C, S, S] float32) and / or the cells
    k0 .. k0 + chunk - 1 of the uint8 RGB `canvas` of the rows x cols map (see vsom_proto_mosaic); both optional."""
    rows, cols = int(map_size[0]), int(map_size[1])
    K, pd = rows * cols, p * p * C
    _dense(pred, "pred", _F32, (None, pd))
    if pred.shape[0] % (n + 1):
        raise ValueError(f"pred: {pred.shape[0]} rows are not a whole number of images of {n} + 1 rows")
    chunk, S = pred.shape[0] // (n + 1), int(round(n ** 0.5)) * p
    _dense(images, "images", _F32, (K, C, S, S), optional=True)
    _dense(canvas, "canvas", _U8, (rows * S + (rows - 1) * gap, cols * S + (cols - 1) * gap, 3), optional=True)
    check(lib.vsom_proto_mosaic(ptr(pred), chunk, int(n), int(p), int(C), ptr(images), ptr(canvas), int(k0), K, rows, cols,
                                int(gap), stream()), "vsom_proto_mosaic")


def last_label(bmu, label, first_ordinal, cells, bad):
    """cells[bmu[i]] = max(cells[bmu[i]], (first_ordinal + i + 1) << 32 | label[i]) (bmu, label: contiguous int64 of one
    size; cells: [K] int64, zeroed by the caller; bad int32 [1])."""
    n = _buffer(bmu, "bmu", _I64).numel()
    _dense(label, "label", _I64, n)
    _buffer(cells, "cells", _I64)
    _dense(bad, "bad", _I32, 1)
    check(lib.vsom_last_label(ptr(bmu), ptr(label), n, int(first_ordinal), cells.numel(), ptr(cells), ptr(bad),
                              stream()), "vsom_last_label")
    return cells


def map_stats(dist, bmu, grid_positions, adj_r2, first_ordinal, hits, qe_fix, te, nearest, bad, second=None):
    """One batch folded into the map-quality accumulators (see vsom_map_stats): dist f32 [B, K] contiguous, bmu int64 [B],
    hits / qe_fix [K] and te [1] int64 zeroed by the caller, nearest [K] int64 set to -1 (all-ones), bad [1] int32;
    `second` [B] int64 (optional) receives the runner-up units."""
    B, K = _dense(dist, "dist", _F32, (None, None)).shape
    _dense(grid_positions, "grid_positions", _F32, (K, 2))
    _dense(bmu, "bmu", _I64, B)
    _dense(hits, "hits", _I64, K); _dense(qe_fix, "qe_fix", _I64, K); _dense(te, "te", _I64, 1); _dense(nearest, "nearest", _I64, K)
    _dense(bad, "bad", _I32, 1)
    _dense(second, "second", _I64, B, optional=True)
    check(lib.vsom_map_stats(ptr(dist), ptr(bmu), B, K, ptr(grid_positions), float(adj_r2), int(first_ordinal), ptr(hits),
                             ptr(qe_fix), ptr(te), ptr(nearest), ptr(bad), ptr(second), stream()), "vsom_map_stats")


def umatrix(W, grid_positions, adj_r2, distance):
    """-> (u [K] f32, nbr_idx [K, 8] int32, nbr_dist [K, 8] f32) on the device (see vsom_umatrix) of W f32 [K, L] contiguous
    and grid_positions f32 [K, 2].  The status word is read here, after the launch: a unit with more than 8 units within
    adj_r2 raises VsomError (VSOM_EUNSUPPORTED)."""
    K, L = _dense(W, "W", _F32, (None, None)).shape
    _dense(grid_positions, "grid_positions", _F32, (K, 2))
    u = torch.empty(K, dtype=torch.float32, device=W.device)
    nbr_idx = torch.empty(K, 8, dtype=torch.int32, device=W.device)
    nbr_dist = torch.empty(K, 8, dtype=torch.float32, device=W.device)
    status = torch.zeros(1, dtype=torch.int32, device=W.device)
    check(lib.vsom_umatrix(ptr(W), K, L, ptr(grid_positions), float(adj_r2), int(distance), ptr(nbr_idx), ptr(nbr_dist), ptr(u),
                           ptr(status), stream()), "vsom_umatrix")
    most = int(status.item())
    if most:
        raise _lib_mod.VsomError(f"vsom_umatrix failed with status -3: a unit has {most} units within adj_r2={adj_r2} (8 are kept)")
    return u, nbr_idx, nbr_dist


# ---------------------------------------------------------------- data pipeline (vit_som_amd.data)
AUGMENT_PARAMS = 16


def _crops(scale, log_ratio, scale2, log_ratio2):
    """The crop-box arguments of the two plan entries; scale2 = None: one crop."""
    s2, l2 = (scale2, log_ratio2) if scale2 is not None else ((0.0, 0.0), (0.0, 0.0))
    return (float(scale[0]), float(scale[1]), float(log_ratio[0]), float(log_ratio[1]), int(scale2 is not None), float(s2[0]),
            float(s2[1]), float(l2[0]), float(l2[1]))


def augment_plan(index, params, N, H, S, scale, log_ratio, scale2, log_ratio2, flip_p, erase_p, seed, epoch):
    """params[b] <- the augmentation plan of row index[b] (int64 [B]) of a data set of N rows in `epoch` (see
    vsom_augment_plan); params int32 [>= B, AUGMENT_PARAMS] (a longer buffer passes); scale2 = None: one crop."""
    B = _dense(index, "index", _I64, (None,)).numel()
    _buffer(params, "params", _I32, B * AUGMENT_PARAMS)
    check(lib.vsom_augment_plan(ptr(index), int(N), B, int(H), int(S), *_crops(scale, log_ratio, scale2, log_ratio2),
                                float(flip_p), float(erase_p), int(seed), int(epoch), ptr(params), stream()), "vsom_augment_plan")
    return params


def augment_batch(src, index, params, out, S, R, off, mean, std, seed, epoch, out_u8=None):
    """out[b] <- the transformed row index[b] of the uint8 set `src` [N, C, H, W] (see vsom_augment_batch); params = None: the
    whole image, no flip, no erase; out_u8 optional.  out, out_u8 and params may be longer than the batch needs."""
    N, C, H, W = _dense(src, "src", _U8, (None,) * 4).shape
    B = _dense(index, "index", _I64, (None,)).numel()
    _buffer(params, "params", _I32, B * AUGMENT_PARAMS, optional=True)
    _buffer(out, "out", _F32, B * C * S * S); _buffer(out_u8, "out_u8", _U8, B * C * S * S, optional=True)
    _dense(mean, "mean", _F32, C); _dense(std, "std", _F32, C)
    check(lib.vsom_augment_batch(ptr(src), N, C, H, W, ptr(index), ptr(params), B, int(S), int(R), int(off), ptr(mean), ptr(std),
                                 int(seed), int(epoch), ptr(out), ptr(out_u8), stream()), "vsom_augment_batch")
    return out


RANDAUG_PARAMS = 72


def _pack_fill(fill):
    fill = tuple(int(v) for v in fill) + (0,) * (3 - len(fill))
    if len(fill) != 3 or not all(0 <= v <= 255 for v in fill):
        raise ValueError(f"fill: expected up to three levels in [0, 255], got {fill}")
    return fill[0] | fill[1] << 8 | fill[2] << 16


def randaug_plan(index, ra, N, S, randaug_n, autoaugment, flip1_p, fill_tv, fill_timm, seed, epoch):
    """ra[b] <- the RandAugment / rand-m9 record of row index[b] in `epoch` (see vsom_randaug_plan); ra int32
    [>= B, RANDAUG_PARAMS] (a longer buffer passes); fills: one level per channel."""
    B = _dense(index, "index", _I64, (None,)).numel()
    _buffer(ra, "ra", _I32, B * RANDAUG_PARAMS)
    check(lib.vsom_randaug_plan(ptr(index), int(N), B, int(S), int(randaug_n), int(bool(autoaugment)), float(flip1_p),
                                _pack_fill(fill_tv), _pack_fill(fill_timm), int(seed), int(epoch), ptr(ra), stream()), "vsom_randaug_plan")
    return ra


def augment_batch_ra(src, index, params, ra, out, S, mean, std, seed, epoch, out_u8=None):
    """out[b] <- the training transform of row index[b] with the op slots of `ra` between the crops (see vsom_augment_batch_ra);
    params and ra are both needed, out_u8 is optional."""
    N, C, H, W = _dense(src, "src", _U8, (None,) * 4).shape
    B = _dense(index, "index", _I64, (None,)).numel()
    _buffer(params, "params", _I32, B * AUGMENT_PARAMS); _buffer(ra, "ra", _I32, B * RANDAUG_PARAMS)
    _buffer(out, "out", _F32, B * C * S * S); _buffer(out_u8, "out_u8", _U8, B * C * S * S, optional=True)
    _dense(mean, "mean", _F32, C); _dense(std, "std", _F32, C)
    check(lib.vsom_augment_batch_ra(ptr(src), N, C, H, W, ptr(index), ptr(params), ptr(ra), B, int(S), ptr(mean), ptr(std), int(seed),
                                    int(epoch), ptr(out), ptr(out_u8), stream()), "vsom_augment_batch_ra")
    return out


# ---------------------------------------------------------------- data pipeline, image sets of varying size
def augment_plan_ragged(index, shapes, params, S, scale, log_ratio, scale2, log_ratio2, flip_p, erase_p, seed, epoch):
    """augment_plan with box 1 drawn on each sample's own (H_n, W_n) = shapes[index[b]], shapes int32 [N, 2] (see
    vsom_augment_plan_ragged)."""
    B = _dense(index, "index", _I64, (None,)).numel()
    _dense(shapes, "shapes", _I32, (None, 2))
    _buffer(params, "params", _I32, B * AUGMENT_PARAMS)
    check(lib.vsom_augment_plan_ragged(ptr(index), ptr(shapes), shapes.shape[0], B, int(S), *_crops(scale, log_ratio, scale2, log_ratio2),
                                       float(flip_p), float(erase_p), int(seed), int(epoch), ptr(params), stream()),
          "vsom_augment_plan_ragged")
    return params


def augment_ragged_scratch_bytes(B: int, C: int, S: int) -> int:
    return lib.vsom_augment_ragged_scratch_bytes(int(B), int(C), int(S))


def augment_batch_ragged(data, offsets, shapes, C, max_h, max_w, index, params, out, S, R, mean, std, seed, epoch, scratch=None,
                         out_u8=None):
    """out[b] <- the transformed image index[b] of the ragged uint8 set (data [bytes], offsets int64 [N], shapes int32 [N, 2])
    (see vsom_augment_batch_ragged); params = None: the evaluation transform Resize(R) -> CenterCrop(S), and `scratch` is
    optional; otherwise `scratch` (uint8, augment_ragged_scratch_bytes(B, C, S); the entry checks its size) holds the image
    between the two crops.  out_u8 optional."""
    _dense(data, "data", _U8, (None,))
    N = _dense(offsets, "offsets", _I64, (None,)).numel()
    _dense(shapes, "shapes", _I32, (N, 2))
    B = _dense(index, "index", _I64, (None,)).numel()
    _buffer(params, "params", _I32, B * AUGMENT_PARAMS, optional=True); _buffer(scratch, "scratch", _U8, optional=params is None)
    _buffer(out, "out", _F32, B * C * S * S); _buffer(out_u8, "out_u8", _U8, B * C * S * S, optional=True)
    _dense(mean, "mean", _F32, C); _dense(std, "std", _F32, C)
    check(lib.vsom_augment_batch_ragged(ptr(data), data.numel(), ptr(offsets), ptr(shapes), N, int(C), int(max_h), int(max_w),
                                        ptr(index), ptr(params), B, int(S), int(R), ptr(mean), ptr(std), int(seed), int(epoch),
                                        ptr(scratch), 0 if scratch is None else scratch.numel(), ptr(out), ptr(out_u8), stream()),
          "vsom_augment_batch_ragged")
    return out


# ---------------------------------------------------------------- k-means (evaluate_kmeans)
def kmeans_workspace_bytes(N: int, D: int, k: int) -> int:
    return lib.vsom_kmeans_workspace_bytes(N, D, k)


def kmeans_assign(X, centers, labels, prev_labels, mind, ws):
    """One Lloyd E-step + partial M-step on X f32 [N, D] (any row stride) and centers f32 [k, D]: labels int64 [N] (from
    prev_labels, likewise) and mind f32 [N] written, cluster partials into ws (kmeans_workspace_bytes(N, D, k) bytes)."""
    N, D, ldx = _matrix(X, "X")
    k = _dense(centers, "centers", _F32, (None, D)).shape[0]
    _dense(labels, "labels", _I64, N); _dense(prev_labels, "prev_labels", _I64, N); _dense(mind, "mind", _F32, N)
    _buffer(ws, "ws", None)
    check(lib.vsom_kmeans_assign(ptr(X), ldx, N, D, ptr(centers), k, ptr(labels), ptr(prev_labels), ptr(mind), ptr(ws),
                                 ws.numel() * ws.element_size(), stream()), "vsom_kmeans_assign")


def kmeans_update(centers_old, centers_new, N, mind, counts, status, ws):
    """centers_new f32 [k, D], counts [k] int64 and status [4] fp64 = (changed, center_shift_tot, empty, inertia) from
    centers_old, mind f32 [N] and the ws kmeans_assign left."""
    k, D = _dense(centers_old, "centers_old", _F32, (None, None)).shape
    _dense(centers_new, "centers_new", _F32, (k, D)); _dense(mind, "mind", _F32, int(N))
    _dense(counts, "counts", _I64, k); _dense(status, "status", _F64, 4); _buffer(ws, "ws", None)
    check(lib.vsom_kmeans_update(ptr(centers_old), ptr(centers_new), N, D, k, ptr(mind), ptr(counts), ptr(status), ptr(ws),
                                 ws.numel() * ws.element_size(), stream()), "vsom_kmeans_update")


def kmeans_relocate(X, labels, moves, centers_old, centers_new, counts, status, ws):
    """Apply the empty-cluster moves (int64 [m, 2] device tensor of (cluster, sample)) in order, then the centres again
    (labels int64 [N], centres f32 [k, D], counts int64 [k], status fp64 [4] as in kmeans_update)."""
    N, D, ldx = _matrix(X, "X")
    k = _dense(centers_old, "centers_old", _F32, (None, D)).shape[0]
    _dense(centers_new, "centers_new", _F32, (k, D)); _dense(labels, "labels", _I64, N)
    _dense(moves, "moves", _I64, (None, 2)); _dense(counts, "counts", _I64, k); _dense(status, "status", _F64, 4)
    _buffer(ws, "ws", None)
    check(lib.vsom_kmeans_relocate(ptr(X), ldx, N, D, k, ptr(labels), ptr(moves), moves.shape[0], ptr(centers_old),
                                   ptr(centers_new), ptr(counts), ptr(status), ptr(ws), ws.numel() * ws.element_size(),
                                   stream()), "vsom_kmeans_relocate")


def kmeanspp_dist(X, candidates, closest, dist, pots):
    """dist f32 [T, N] = min(closest, squared distance to each candidate row) for candidates int64 [T]; closest f32 [N] is
    optional (None: no minimum); pots fp64 [>= T] = row sums of dist."""
    N, D, ldx = _matrix(X, "X")
    T = _buffer(candidates, "candidates", _I64).numel()
    _dense(closest, "closest", _F32, N, optional=True)
    _dense(dist, "dist", _F32, (T, N)); _buffer(pots, "pots", _F64, T)
    check(lib.vsom_kmeanspp_dist(ptr(X), ldx, N, D, ptr(candidates), T, ptr(closest), ptr(dist), ptr(pots), stream()),
          "vsom_kmeanspp_dist")


def kmeans_colvar(X, k, out, ws):
    """out fp64 [1] = mean(var(X, axis=0)) in fp64; ws as for kmeans_assign."""
    N, D, ldx = _matrix(X, "X")
    _dense(out, "out", _F64, 1); _buffer(ws, "ws", None)
    check(lib.vsom_kmeans_colvar(ptr(X), ldx, N, D, k, ptr(out), ptr(ws), ws.numel() * ws.element_size(), stream()),
          "vsom_kmeans_colvar")


# ---------------------------------------------------------------- UMAP (visualize_umap_progression)
UMAP_MAX_K = 64                                                  # csrc/knn.hip (KNN_MAX_K): one list entry per lane


def umap_knn(X, k, metric, knn_idx, knn_dist):
    """knn_idx int64 [N, k] / knn_dist f32 [N, k]: the exact k nearest rows of X (row itself first), ascending by
    (distance, index); metric DIST_EUCLIDEAN or DIST_COSINE."""
    N, D, ldx = _matrix(X, "X")
    _dense(knn_idx, "knn_idx", _I64, (N, k)); _dense(knn_dist, "knn_dist", _F32, (N, k))
    ws = scratch(lib.vsom_umap_knn_workspace_bytes(N, k), X.device)
    check(lib.vsom_umap_knn(ptr(X), ldx, N, D, int(k), int(metric), ptr(knn_idx), ptr(knn_dist), ptr(ws), ws.numel(),
                            stream()), "vsom_umap_knn")
    return knn_idx, knn_dist


def umap_neg_sample(seed, epoch, edge, p, N) -> int:
    """The negative sample vsom_umap_epoch draws (host arithmetic)."""
    return int(lib.vsom_umap_neg_sample(int(seed), int(epoch), int(edge), int(p), int(N)))


def umap_epoch(indptr, indices, eps, next_s, eps_neg, next_neg, Y_in, Y_out, a, b, gamma, alpha, epoch, seed):
    """One synchronous layout epoch: Y_out from Y_in (f32 [N, dim]) over the CSR graph (indptr int64 [N + 1], indices int64
    [nnz]); eps, next_s, eps_neg, next_neg fp64 [nnz], next_s / next_neg updated in place."""
    N, dim = _dense(Y_in, "Y_in", _F32, (None, None)).shape
    _dense(Y_out, "Y_out", _F32, (N, dim)); _dense(indptr, "indptr", _I64, N + 1)
    nnz = _buffer(indices, "indices", _I64).numel()
    _dense(eps, "eps", _F64, nnz); _dense(next_s, "next_s", _F64, nnz)
    _dense(eps_neg, "eps_neg", _F64, nnz); _dense(next_neg, "next_neg", _F64, nnz)
    check(lib.vsom_umap_epoch(ptr(indptr), ptr(indices), ptr(eps), ptr(next_s), ptr(eps_neg), ptr(next_neg), ptr(Y_in),
                              ptr(Y_out), N, dim, float(a), float(b), float(gamma), float(alpha), int(epoch), int(seed),
                              stream()), "vsom_umap_epoch")
    return Y_out


def umap_transform_workspace(M, k, device) -> torch.Tensor:
    """The byte buffer that holds the schedule state of one transform layout (it persists between sliced calls)."""
    return torch.empty(max(int(lib.vsom_umap_transform_workspace_bytes(int(M), int(k))), 16), dtype=torch.uint8, device=device)


def umap_transform_state(ws, M, k):
    """(epoch_of_next_sample, epoch_of_next_negative_sample): fp64 [k, M] views of such a buffer."""
    n = 8 * int(M) * int(k)
    off = (n + 255) // 256 * 256
    return ws[:n].view(torch.float64).view(k, M), ws[off:off + n].view(torch.float64).view(k, M)


def umap_transform_layout(knn_idx, weights, eps, Y_train, Y, a, b, gamma, initial_alpha, n_epochs, epoch_begin, epoch_end,
                          negative_sample_rate, seed, status, ws):
    """Epochs [epoch_begin, epoch_end) of the transform layout of Y [M, dim] against the fixed Y_train [N, dim] in one launch
    (epoch_begin == 0 writes the weighted-mean init first); knn_idx int64 / weights fp64 / eps fp64 [M, k]; status int32 [1]
    (zeroed by the caller) counts refused edges; ws uint8 from umap_transform_workspace(M, k) (the entry checks its size)."""
    M, k = _dense(knn_idx, "knn_idx", _I64, (None, None)).shape
    N, dim = _dense(Y_train, "Y_train", _F32, (None, None)).shape
    _dense(Y, "Y", _F32, (M, dim)); _dense(weights, "weights", _F64, (M, k)); _dense(eps, "eps", _F64, (M, k))
    _dense(status, "status", _I32, 1); _buffer(ws, "ws", _U8)
    check(lib.vsom_umap_transform_layout(ptr(knn_idx), ptr(weights), ptr(eps), ptr(Y_train), N, ptr(Y), M, k, dim, float(a),
                                         float(b), float(gamma), float(initial_alpha), int(n_epochs), int(epoch_begin),
                                         int(epoch_end), int(negative_sample_rate), int(seed), ptr(status), ptr(ws), ws.numel(),
                                         stream()), "vsom_umap_transform_layout")
    return Y


# ---------------------------------------------------------------- kNN probe (evaluate_knn)
KNN_MAX_K = UMAP_MAX_K                                           # the same search (csrc/knn.hip), the same limit
KNN_MAX_CLASSES = 1024                                           # csrc/knn.hip: the vote's LDS score table
KNN_UNIFORM, KNN_DISTANCE, KNN_SOFTMAX = 0, 1, 2                 # VSOM_KNN_*


def knn_query(Q, X, k, metric, idx, dist, index_base=0, accumulate=False, exclude=None):
    """idx int64 [Nq, k] / dist f32 [Nq, k]: the exact k nearest rows of the bank chunk X for every row of Q, as
    index_base + row, ascending by (distance, index); with accumulate the lists already in idx / dist (from other index
    ranges) are folded with this chunk.  exclude int64 [Nq] (optional): a global bank ordinal each query never receives."""
    Nq, D, ldq = _matrix(Q, "Q")
    Nb, _, ldx = _matrix(X, "X", cols=D)
    _dense(idx, "idx", _I64, (Nq, k)); _dense(dist, "dist", _F32, (Nq, k)); _dense(exclude, "exclude", _I64, Nq, optional=True)
    ws = scratch(lib.vsom_knn_query_workspace_bytes(Nq, Nb, k), Q.device)
    check(lib.vsom_knn_query(ptr(Q), ldq, Nq, ptr(X), ldx, Nb, D, int(k), int(metric), int(index_base), int(bool(accumulate)),
                             ptr(exclude), ptr(idx), ptr(dist), ptr(ws), ws.numel(), stream()), "vsom_knn_query")
    return idx, dist


def knn_ranks(A, nbr, metric, less, tied):
    """less / tied int32 [N, k]: for every row i of A [N, D] and every slot n = nbr[i, j] (int64 [N, k]; rows of A, -1 = an
    empty slot) the number of rows other than i and n that lie closer to i than n does / exactly as far, in the distances
    of umap_knn (same contraction, same order); -1 in both for an empty slot and for n == i.  An index outside [0, N) other
    than -1 is refused HERE, on the host (one device reduction and one synchronisation): the C entry has no status word
    and would treat it as an empty slot."""
    N, D, lda = _matrix(A, "A")
    k = _dense(nbr, "nbr", _I64, (N, None)).shape[1]
    _dense(less, "less", _I32, (N, k)); _dense(tied, "tied", _I32, (N, k))
    n_bad = int(((nbr < -1) | (nbr >= N)).sum())
    if n_bad:
        raise ValueError(f"knn_ranks: {n_bad} neighbour indices outside [0, {N}) (-1 marks an empty slot)")
    ws = scratch(lib.vsom_knn_ranks_workspace_bytes(N, k), A.device)
    check(lib.vsom_knn_ranks(ptr(A), lda, N, D, int(metric), ptr(nbr), int(k), ptr(less), ptr(tied), ptr(ws), ws.numel(),
                             stream()), "vsom_knn_ranks")
    return less, tied


SILHOUETTE_MAX_N = (1 << 22) - 1                                 # csrc/knn.hip: a row's fixed-point sum stays below 2^63


class Silhouette:
    """What one vsom_silhouette call wrote: device tensors, except `status`, the four counts on the host."""
    __slots__ = ("sil", "a", "b", "nearest", "counts", "cluster_mean", "score", "status", "sums")


def silhouette_workspace(N, C, device) -> torch.Tensor:
    """A workspace of the caller's own for `silhouette`; afterwards `silhouette(...).sums` is a view of it."""
    return torch.empty(max(lib.vsom_silhouette_workspace_bytes(int(N), int(C)), 1), dtype=torch.uint8, device=device)


def silhouette(X, labels, metric, n_clusters, ws=None, details=True):
    """Silhouette coefficient of the rows of X [N, D] (f32) under labels int64 [N] in [0, n_clusters) -> Silhouette:
    sil f64 [N], a / b f64 [N] and nearest int64 [N] (None without `details`), counts int64 [C], cluster_mean f64 [C],
    score f64 [1], status (host ints: rows with a label out of range, refused distances, non-empty clusters, singleton
    clusters) and, with a workspace (optional, uint8) from silhouette_workspace, sums int64 [N, C]: the fixed-point distance
    sums.  One synchronisation, to read status.  A NaN or infinite input (status[1] != 0) raises ValueError; a label outside
    the range does not: that row gets NaN, counts for nothing and is reported in status[0]."""
    N, D, ldx = _matrix(X, "X")
    C = int(n_clusters)
    _dense(labels, "labels", _I64, (N,))
    dev = X.device
    r = Silhouette()
    f64 = lambda n: torch.empty(n, dtype=torch.float64, device=dev)      # noqa: E731
    r.sil, r.a, r.b = f64(N), f64(N) if details else None, f64(N) if details else None
    r.nearest = torch.empty(N, dtype=torch.int64, device=dev) if details else None
    r.counts = torch.empty(max(C, 0), dtype=torch.int64, device=dev)
    r.cluster_mean, r.score = f64(max(C, 0)), f64(1)
    status = torch.empty(4, dtype=torch.int64, device=dev)
    need = lib.vsom_silhouette_workspace_bytes(N, C)
    own = ws is not None
    if own:
        _buffer(ws, "ws", _U8, need)
    else:
        ws = scratch(need, dev)
    check(lib.vsom_silhouette(ptr(X), ldx, N, D, int(metric), ptr(labels), C, ptr(r.sil), ptr(r.a), ptr(r.b), ptr(r.nearest),
                              ptr(r.counts), ptr(r.cluster_mean), ptr(r.score), ptr(status), ptr(ws), ws.numel(), stream()),
          "vsom_silhouette")
    r.sums = ws[:N * C * 8].view(torch.int64).view(N, C) if own else None
    r.status = [int(v) for v in status.cpu()]
    if r.status[1]:
        raise ValueError(f"silhouette: {r.status[1]} distances were not finite: the input contains NaN or infinity, or a "
                         f"row's squared norm overflows float32")
    return r


def knn_vote(idx, dist, bank_labels, n_classes, weights, temperature, pred, status, scores=None):
    """pred int64 [Nq] = first argmax of the fp64 class scores of each query's neighbour list (idx int64 / dist f32 [Nq, k],
    bank_labels int64 [n_bank]; weights KNN_UNIFORM / KNN_DISTANCE / KNN_SOFTMAX); scores fp64 [Nq, n_classes] optionally;
    status int32 [2] (zeroed by the caller) counts refused neighbours and queries left without one (pred -1)."""
    Nq, k = _dense(idx, "idx", _I64, (None, None)).shape
    _dense(dist, "dist", _F32, (Nq, k)); _buffer(bank_labels, "bank_labels", _I64)
    _dense(pred, "pred", _I64, Nq); _dense(status, "status", _I32, 2)
    _dense(scores, "scores", _F64, (Nq, int(n_classes)), optional=True)
    check(lib.vsom_knn_vote(ptr(idx), ptr(dist), Nq, k, ptr(bank_labels), bank_labels.numel(), int(n_classes), int(weights),
                            float(temperature), ptr(pred), ptr(scores), ptr(status), stream()), "vsom_knn_vote")
    return pred


# ---------------------------------------------------------------- principal component analysis (pca.py)
PCA_MAX_WIDTH = 256                                              # csrc/pca.hip: PCA_MAX_L
PCA_PROJECT, PCA_BACKPROJECT = 0, 1                              # `which` of vsom_pca_slabs


def pca_slabs(N, D, l, which) -> int:
    """Floats of slab space pca_project (which = PCA_PROJECT) / pca_backproject (PCA_BACKPROJECT) take: host arithmetic."""
    return int(lib.vsom_pca_slabs(int(N), int(D), int(l), int(which)))


def pca_colstats(X, mean=None, var=None):
    """(mean f32 [D], var f64 [D]) of the columns of X [N, D]: fp64 sums in a fixed order, the mean rounded once, the
    unbiased variance about that rounded mean.  mean / var optional: allocated here when None."""
    N, D, ldx = _matrix(X, "X")
    mean = torch.empty(D, dtype=torch.float32, device=X.device) if mean is None else _dense(mean, "mean", _F32, (D,))
    var = torch.empty(D, dtype=torch.float64, device=X.device) if var is None else _dense(var, "var", _F64, (D,))
    n_part = int(lib.vsom_pca_colstats_parts(N, D))
    part = scratch(8 * n_part, X.device)
    check(lib.vsom_pca_colstats(ptr(X), ldx, N, D, ptr(mean), ptr(var), ptr(part), part.numel() // 8, stream()), "vsom_pca_colstats")
    return mean, var


def pca_project(X, mean, B, scale, Y):
    """Y [N, l] = (X - mean) B^T diag(scale); X [N, D], B [l, D] and Y with any row stride; mean [D] and scale [l] optional."""
    N, D, ldx = _matrix(X, "X")
    l, _, ldb = _matrix(B, "B", cols=D)
    _, _, ldy = _matrix(Y, "Y", N, l)
    _dense(mean, "mean", _F32, (D,), optional=True); _dense(scale, "scale", _F32, (l,), optional=True)
    slabs = scratch(4 * pca_slabs(N, D, l, PCA_PROJECT), X.device)
    check(lib.vsom_pca_project(ptr(X), ldx, N, D, ptr(mean), ptr(B), ldb, l, ptr(scale), ptr(Y), ldy, ptr(slabs),
                               slabs.numel() // 4, stream()), "vsom_pca_project")
    return Y


def pca_backproject(Y, X, mean, Zt):
    """Zt [l, D] = Y^T (X - mean); Y [N, l], X [N, D] and Zt with any row stride; mean [D] optional."""
    N, D, ldx = _matrix(X, "X")
    _, l, ldy = _matrix(Y, "Y", rows=N)
    _, _, ldz = _matrix(Zt, "Zt", l, D)
    _dense(mean, "mean", _F32, (D,), optional=True)
    slabs = scratch(4 * pca_slabs(N, D, l, PCA_BACKPROJECT), X.device)
    check(lib.vsom_pca_backproject(ptr(Y), ldy, ptr(X), ldx, N, D, ptr(mean), l, ptr(Zt), ldz, ptr(slabs),
                                   slabs.numel() // 4, stream()), "vsom_pca_backproject")
    return Zt


def pca_gram(Zt, G, B=None, H=None):
    """G f64 [l, l] = Zt Zt^T and, with B [l, D] and H f64 [l, l] (optional, together), H = B Zt^T: fp64 products and sums."""
    l, D, ldz = _matrix(Zt, "Zt")
    _dense(G, "G", _F64, (l, l))
    if (B is None) != (H is None):
        raise ValueError("B and H go together")
    _, _, ldb = _matrix(B, "B", l, D, optional=True)
    _dense(H, "H", _F64, (l, l), optional=True)
    check(lib.vsom_pca_gram(ptr(Zt), ldz, ptr(B), ldb, l, D, ptr(G), ptr(H), stream()), "vsom_pca_gram")
    return G, H


def pca_rotate(T, Zt, Bout):
    """Bout [l_out, D] = T Zt, T f64 [l_out, l_in] on the device: fp64 accumulation, one rounding.  Bout may not overlap Zt."""
    l_in, D, ldz = _matrix(Zt, "Zt")
    l_out = _dense(T, "T", _F64, (None, l_in)).shape[0]
    _, _, ldo = _matrix(Bout, "Bout", l_out, D)
    check(lib.vsom_pca_rotate(ptr(T), l_out, l_in, ptr(Zt), ldz, D, ptr(Bout), ldo, stream()), "vsom_pca_rotate")
    return Bout


def pca_reconstruct(Y, scale, B, mean, Xout):
    """Xout [M, D] = (Y diag(scale)) B + mean; Y [M, l], B [l, D], Xout with any row stride; scale [l] and mean [D] optional."""
    M, l, ldy = _matrix(Y, "Y")
    _, D, ldb = _matrix(B, "B", rows=l)
    _, _, ldo = _matrix(Xout, "Xout", M, D)
    _dense(scale, "scale", _F32, (l,), optional=True); _dense(mean, "mean", _F32, (D,), optional=True)
    check(lib.vsom_pca_reconstruct(ptr(Y), ldy, M, l, ptr(scale), ptr(B), ldb, D, ptr(mean), ptr(Xout), ldo, stream()),
          "vsom_pca_reconstruct")
    return Xout


# ---------------------------------------------------------------- Kohonen's batch map (SOMLayer.fit_batch)
def som_batch_accumulate(X, bmu, sums, counts, inv_norm=None, accumulate=False, bad=None):
    """counts [K] int64 = rows per unit, sums [K, D] float64 = per unit the sum of its rows of X [N, D] (times inv_norm f32
    [N] when given) under bmu int64 [N], every (unit, column) one fp64 chain in ascending row index (see
    vsom_som_batch_accumulate).  accumulate=True continues from what sums / counts hold: a row set cut into several calls
    gives the same bits as one call.  bad: an int32 [1] device counter of BMUs outside [0, K) the caller zeroes and reads
    later; None: checked here (one host read) and raised as VsomError."""
    N, D, ldx = _matrix(X, "X")
    K = _dense(counts, "counts", _I64, (None,)).numel()
    _dense(bmu, "bmu", _I64, (N,)); _dense(sums, "sums", _F64, (K, D)); _dense(inv_norm, "inv_norm", _F32, (N,), optional=True)
    own = bad is None
    if own:
        bad = torch.zeros(1, dtype=torch.int32, device=X.device)
    _dense(bad, "bad", _I32, 1)
    order = torch.sort(bmu, stable=True).indices              # the rows of a unit, ascending: what fixes every chain's order
    n_seg = int(lib.vsom_som_batch_accumulate_parts(K))
    seg = scratch(8 * n_seg, X.device)
    check(lib.vsom_som_batch_accumulate(ptr(X), ldx, N, D, ptr(bmu), ptr(order), ptr(inv_norm), K, ptr(sums), ptr(counts),
                                        int(bool(accumulate)), ptr(bad), ptr(seg), seg.numel() // 8, stream()),
          "vsom_som_batch_accumulate")
    if own:
        n_bad = int(bad.item())
        if n_bad:
            raise _lib_mod.VsomError(f"vsom_som_batch_accumulate failed with status -1: {n_bad} rows have a BMU outside [0, {K})")
    return sums, counts


def som_batch_update(sums, counts, grid_positions, sigma, W_out, normalize=False):
    """W_out [K, D] f32 (any row stride) = the batch-map update at radius sigma from sums [K, D] float64, counts [K] int64
    and grid_positions f32 [K, 2] (see vsom_som_batch_update); normalize=True L2-normalises every row afterwards (the
    cosine map)."""
    K = _dense(counts, "counts", _I64, (None,)).numel()
    D = _dense(sums, "sums", _F64, (K, None)).shape[1]
    _dense(grid_positions, "grid_positions", _F32, (K, 2))
    _, _, ldw = _matrix(W_out, "W_out", K, D)
    n_part = int(lib.vsom_som_batch_update_parts(K))
    part = scratch(8 * n_part, sums.device)
    check(lib.vsom_som_batch_update(ptr(sums), ptr(counts), ptr(grid_positions), K, D, float(sigma), int(bool(normalize)), ptr(W_out),
                                    ldw, ptr(part), part.numel() // 8, stream()), "vsom_som_batch_update")
    return W_out


# ---------------------------------------------------------------- linear probe (linear_probe.py)
PROBE_MAX_CLASSES = 256                                          # csrc/linear_probe.hip: PROBE_MAX_C
PROBE_MAX_STEPS = 16                                             # the line search's ladder
LBFGS_MAX_MEMORY = 16
# the L-BFGS state record (state[:16]): indices
LBFGS_ALPHA0, LBFGS_GTP, LBFGS_GG, LBFGS_GMAX, LBFGS_COUNT, LBFGS_SKIPPED, LBFGS_ACCEPTED, LBFGS_SLOT, LBFGS_HEAD = range(9)
PROBE_STEP, PROBE_LS_STATUS, PROBE_F, PROBE_J = 12, 13, 14, 15
LBFGS_RECORD = 16


def probe_parts(N, C) -> int:
    """Doubles of scratch probe_residual / probe_linesearch take: host arithmetic."""
    return int(lib.vsom_probe_parts(int(N), int(C)))


def probe_fold(A, invstd, B, W=None, pen=None):
    """B f32 [C, D] (any row stride) = A o invstd (A fp64 [C, D], invstd fp64 [D]; one rounding); with W fp64 [C, D] and pen
    fp64 [3] (optional, together) also pen = (W.W, W.A, A.A)."""
    C, D = _dense(A, "A", _F64, (None, None)).shape
    _dense(invstd, "invstd", _F64, D)
    _, _, ldb = _matrix(B, "B", C, D)
    if (W is None) != (pen is None):
        raise ValueError("W and pen go together")
    _dense(W, "W", _F64, C * D, optional=True); _dense(pen, "pen", _F64, 3, optional=True)
    n_part = int(lib.vsom_probe_fold_parts(C, D)) if W is not None else 0
    part = scratch(8 * n_part, A.device)
    check(lib.vsom_probe_fold(ptr(A), ptr(invstd), C, D, ptr(B), ldb, ptr(W), ptr(pen), ptr(part), part.numel() // 8, stream()),
          "vsom_probe_fold")
    return B


def probe_residual(Z, b, y, R, loss, gb, status, pred=None, prob=None):
    """R f32 [N, C] = softmax(Z + b) - onehot(y) (Z, R with any row stride; b fp64 [C] optional: no intercept; y int64 [N]),
    loss fp64 [1] = the summed cross-entropy, gb fp64 [C] = the column sums of R; pred int64 [N] and prob fp64 [N, C]
    optionally; status int32 [1] (zeroed by the caller) counts labels outside [0, C)."""
    N, C, ldz = _matrix(Z, "Z")
    _, _, ldr = _matrix(R, "R", N, C)
    _dense(b, "b", _F64, C, optional=True); _dense(loss, "loss", _F64, 1); _dense(gb, "gb", _F64, C)
    _dense(y, "y", _I64, (N,)); _dense(pred, "pred", _I64, (N,), optional=True); _dense(prob, "prob", _F64, N * C, optional=True)
    _dense(status, "status", _I32, 1)
    part = scratch(8 * probe_parts(N, C), Z.device)
    check(lib.vsom_probe_residual(ptr(Z), ldz, N, C, ptr(b), ptr(y), ptr(R), ldr, ptr(loss), ptr(gb), ptr(pred), ptr(prob),
                                  ptr(status), ptr(part), part.numel() // 8, stream()), "vsom_probe_residual")
    return R


def probe_linesearch(Z, Zp, b, pb, y, alpha0, nsteps, phi):
    """phi fp64 [nsteps]: the summed cross-entropy at Z + a_j Zp, b + a_j pb for a_j = alpha0 2^-j (alpha0 fp64 [1] on the
    device), in one launch; Zp has the shape and row stride of Z; b and pb (fp64 [C]) optional, together."""
    N, C, ldz = _matrix(Z, "Z")
    if _matrix(Zp, "Zp", N, C)[2] != ldz:
        raise ValueError("Zp must have the shape and row stride of Z")
    if (b is None) != (pb is None):
        raise ValueError("b and pb go together")
    _dense(b, "b", _F64, C, optional=True); _dense(pb, "pb", _F64, C, optional=True)
    _dense(alpha0, "alpha0", _F64, 1); _dense(phi, "phi", _F64, int(nsteps)); _dense(y, "y", _I64, (N,))
    part = scratch(8 * probe_parts(N, C), Z.device)
    check(lib.vsom_probe_linesearch(ptr(Z), ptr(Zp), ldz, N, C, ptr(b), ptr(pb), ptr(y), ptr(alpha0), int(nsteps), ptr(phi), ptr(part),
                                    part.numel() // 8, stream()), "vsom_probe_linesearch")
    return phi


def probe_step(phi, alpha0, f0, pen, gtp, lam, c1, Z, Zp, theta, p, s_new, rec):
    """The Armijo choice from the ladder phi, then Z += alpha Zp, theta += alpha p, s_new = alpha p; rec[12:16] =
    (alpha, status, F(alpha), j).  alpha0, f0, gtp fp64 [1], pen fp64 [3], theta, p, s_new fp64 [n], rec fp64 [>= 16]: all
    on the device."""
    N, C, ldz = _matrix(Z, "Z")
    if _matrix(Zp, "Zp", N, C)[2] != ldz:
        raise ValueError("Zp must have the shape and row stride of Z")
    nsteps, n = _buffer(phi, "phi", _F64).numel(), _buffer(theta, "theta", _F64).numel()
    _dense(alpha0, "alpha0", _F64, 1); _dense(f0, "f0", _F64, 1); _dense(pen, "pen", _F64, 3); _dense(gtp, "gtp", _F64, 1)
    _dense(p, "p", _F64, n); _dense(s_new, "s_new", _F64, n); _buffer(rec, "rec", _F64, LBFGS_RECORD)
    check(lib.vsom_probe_step(ptr(phi), nsteps, ptr(alpha0), ptr(f0), ptr(pen), ptr(gtp), float(lam), float(c1), ptr(Z), ptr(Zp),
                              ldz, N, C, ptr(theta), ptr(p), ptr(s_new), n, ptr(rec), stream()), "vsom_probe_step")
    return rec


def probe_gradient(Zt, invstd, theta, gb, N, lam, g, g_prev=None, y_new=None):
    """g fp64 [n] = (Zt o invstd) / N + lam W, then gb / N when theta holds an intercept (n = C D + C; gb fp64 [C] is optional
    without one); y_new = g - g_prev (optional, together)."""
    C, D, ldz = _matrix(Zt, "Zt")
    n = _buffer(theta, "theta", _F64).numel()
    if n not in (C * D, C * D + C):
        raise ValueError("theta must hold C D or C D + C elements")
    intercept = n > C * D
    if (g_prev is None) != (y_new is None):
        raise ValueError("g_prev and y_new go together")
    if intercept and gb is None:
        raise ValueError("gb: an intercept needs gb")
    _dense(invstd, "invstd", _F64, D); _dense(g, "g", _F64, n); _dense(gb, "gb", _F64, C, optional=True)
    _dense(g_prev, "g_prev", _F64, n, optional=True); _dense(y_new, "y_new", _F64, n, optional=True)
    check(lib.vsom_probe_gradient(ptr(Zt), ldz, ptr(invstd), ptr(theta), ptr(gb), C, D, int(intercept), int(N), float(lam), ptr(g_prev),
                                  ptr(g), ptr(y_new), stream()), "vsom_probe_gradient")
    return g


def lbfgs_state(m, device):
    """A zeroed state of the L-BFGS pieces for memory m: the record, the Gram matrix and the coefficients."""
    n = int(lib.vsom_lbfgs_state_doubles(int(m)))
    if n <= 0:
        raise ValueError(f"L-BFGS memory must be between 1 and {LBFGS_MAX_MEMORY}, got {m}")
    return torch.zeros(n, dtype=torch.float64, device=device)


def lbfgs_dots(S, Y, g, s_new, y_new, state, dots):
    """dots fp64 [3 (2 m + 3) + 1]: the products of (s_new, y_new, g) with every vector held (S, Y fp64 [m, n]; g fp64 [n];
    state from lbfgs_state(m)), and max |g|, in one pass.  s_new = y_new = None: there is no new pair."""
    m, n = _dense(S, "S", _F64, (None, None)).shape
    _dense(Y, "Y", _F64, (m, n)); _dense(g, "g", _F64, n); _dense(state, "state", _F64, int(lib.vsom_lbfgs_state_doubles(m)))
    if (s_new is None) != (y_new is None):
        raise ValueError("s_new and y_new go together")
    _dense(s_new, "s_new", _F64, n, optional=True); _dense(y_new, "y_new", _F64, n, optional=True)
    _dense(dots, "dots", _F64, 3 * (2 * m + 3) + 1)
    part = scratch(8 * int(lib.vsom_lbfgs_parts(n, m)), g.device)
    check(lib.vsom_lbfgs_dots(ptr(S), ptr(Y), ptr(g), ptr(s_new), ptr(y_new), n, m, int(s_new is not None), ptr(state), ptr(dots),
                              ptr(part), part.numel() // 8, stream()), "vsom_lbfgs_dots")
    return dots


def lbfgs_coeff(dots, m, has_new, state):
    """Takes the new pair in (or skips it), then the two-loop recursion on coefficients; has_new=False empties the history."""
    _dense(dots, "dots", _F64, 3 * (2 * m + 3) + 1); _dense(state, "state", _F64, int(lib.vsom_lbfgs_state_doubles(m)))
    check(lib.vsom_lbfgs_coeff(ptr(dots), int(m), int(bool(has_new)), ptr(state), stream()), "vsom_lbfgs_coeff")
    return state


def lbfgs_combine(S, Y, g, s_new, y_new, state, p):
    """p fp64 [n] = the direction; an accepted pair (s_new, y_new fp64 [n]) is copied into its ring slot of S and Y first."""
    m, n = _dense(S, "S", _F64, (None, None)).shape
    _dense(Y, "Y", _F64, (m, n)); _dense(g, "g", _F64, n); _dense(state, "state", _F64, int(lib.vsom_lbfgs_state_doubles(m)))
    _dense(s_new, "s_new", _F64, n); _dense(y_new, "y_new", _F64, n); _dense(p, "p", _F64, n)
    check(lib.vsom_lbfgs_combine(ptr(S), ptr(Y), ptr(g), ptr(s_new), ptr(y_new), n, m, ptr(state), ptr(p), stream()),
          "vsom_lbfgs_combine")
    return p


# ---------------------------------------------------------------- t-SNE (tsne.py)
TSNE_MAX_K = 63                                                  # csrc/tsne.hip (AFF_MAX_K): the search's 64 less the row itself


def tsne_repulsion_parts(N) -> int:
    """Doubles of zpart at N rows (one per block of 64 rows): host arithmetic."""
    return int(lib.vsom_tsne_repulsion_parts(int(N)))


def tsne_step_parts(N) -> int:
    """Doubles of the step's record at N rows (KL and |grad|^2 per block of 16 rows): host arithmetic."""
    return int(lib.vsom_tsne_step_parts(int(N)))


def tsne_affinities(knn_dist, perplexity, P, beta, status, knn_idx=None, first=1, square=True):
    """P fp64 [N, k_eff] and beta fp64 [N]: the conditional affinities of columns [first, first + k_eff) of knn_dist f32
    [N, k] (any row stride) at this perplexity; status int32 [1] (zeroed by the caller) counts the rows refused, which are
    not written.  knn_idx (optional): int64, laid out as knn_dist; a row with an empty slot in it is refused too."""
    N, k, ldk = _matrix(knn_dist, "knn_dist")
    k_eff = _dense(P, "P", _F64, (N, None)).shape[1]
    _dense(beta, "beta", _F64, (N,)); _dense(status, "status", _I32, 1)
    if first < 0 or first + k_eff > k:
        raise ValueError("columns [first, first + k_eff) must lie inside knn_dist")
    if knn_idx is not None:
        _device(knn_idx, "knn_idx", _I64)
        if knn_idx.shape != knn_dist.shape or knn_idx.stride() != knn_dist.stride():
            raise ValueError("knn_idx must be an int64 device tensor laid out as knn_dist")
    check(lib.vsom_tsne_affinities(ptr(knn_dist), ptr(knn_idx), ldk, N, k_eff, int(first), int(bool(square)), float(perplexity),
                                   ptr(P), ptr(beta), ptr(status), stream()), "vsom_tsne_affinities")
    return P, beta


def tsne_repulsion(Y, rep, sumq, zpart):
    """rep fp64 [N, 2] = sum_j q^2 (y_i - y_j), sumq fp64 [N] = sum_j q over all j != i, q = 1 / (1 + |y_i - y_j|^2) for Y f32
    [N, 2] contiguous, and zpart fp64 [>= tsne_repulsion_parts(N)] (the entry checks its size): the sums of sumq over blocks
    of 64 rows (their sum is Z)."""
    N = _dense(Y, "Y", _F32, (None, 2)).shape[0]
    _dense(rep, "rep", _F64, (N, 2)); _dense(sumq, "sumq", _F64, (N,)); _buffer(zpart, "zpart", _F64)
    check(lib.vsom_tsne_repulsion(ptr(Y), N, ptr(rep), ptr(sumq), ptr(zpart), zpart.numel(), stream()), "vsom_tsne_repulsion")
    return rep, sumq, zpart


def tsne_step(indptr, indices, data, Y_in, Y_out, update, gains, rep, zpart, exaggeration, momentum, learning_rate, part,
              record=False):
    """One iteration: Y_out from Y_in, update and gains (f32 [N, 2] contiguous) in place, from tsne_repulsion's rep and zpart
    at Y_in and the joint P (CSR: indptr int64 [N + 1], indices int64 [nnz], data fp64 [nnz]).  record: part fp64
    [>= tsne_step_parts(N)] receives the (KL, |grad|^2) pairs of the row blocks; add them.  The entry checks the sizes of
    zpart and part."""
    N = _dense(Y_in, "Y_in", _F32, (None, 2)).shape[0]
    _dense(Y_out, "Y_out", _F32, (N, 2)); _dense(update, "update", _F32, (N, 2)); _dense(gains, "gains", _F32, (N, 2))
    _dense(indptr, "indptr", _I64, N + 1); _dense(data, "data", _F64, _buffer(indices, "indices", _I64).numel())
    _dense(rep, "rep", _F64, (N, 2)); _buffer(zpart, "zpart", _F64); _buffer(part, "part", _F64)
    check(lib.vsom_tsne_step(ptr(indptr), ptr(indices), ptr(data), ptr(Y_in), ptr(Y_out), ptr(update), ptr(gains), N, ptr(rep),
                             ptr(zpart), zpart.numel(), float(exaggeration), float(momentum), float(learning_rate),
                             int(bool(record)), ptr(part), part.numel(), stream()), "vsom_tsne_step")
    return Y_out


# ---------------------------------------------------------------- Gaussian mixtures (gmm.py)
GMM_MAX_K = 1024                                                 # csrc/gmm.hip: GM_MAX_K
GMM_ESTEP, GMM_MSTEP, GMM_SET = 0, 1, 2                          # `which` of vsom_gmm_parts
GMM_RECORD = 8                                                   # doubles of the status record
GMM_LOWER_BOUND, GMM_MIN_NK, GMM_MIN_COV, GMM_BAD_COV, GMM_REFUSED = 0, 1, 2, 3, 4


def gmm_parts(N, D, K, which) -> int:
    """Doubles of scratch gmm_estep (GMM_ESTEP), gmm_mstep + gmm_params (GMM_MSTEP) and gmm_set_params (GMM_SET) take: host
    arithmetic, 0 for an empty shape."""
    return int(lib.vsom_gmm_parts(int(N), int(D), int(K), int(which)))


def gmm_slab_rows(N, D, K) -> int:
    """Rows of one M-step slab at this shape: host arithmetic."""
    return int(lib.vsom_gmm_slab_rows(int(N), int(D), int(K)))


def gmm_scratch(N, D, K, which, device):
    """A float64 view of exactly gmm_parts(...) doubles of the shared scratch."""
    n = gmm_parts(N, D, K, which)
    return scratch(8 * n, device)[:8 * n].view(torch.float64)


def gmm_estep(X, means, prec, logc, resp, log_prob_norm, labels, estat, part=None):
    """log_prob_norm fp64 [N], resp f32 [N, K] (any row stride; None: not wanted), labels int64 [N] (None likewise) of the
    mixture (means, prec f32 [K, D] contiguous, logc fp64 [K]) in the direct form; estat fp64 [2] = (sum of log_prob_norm
    over the accepted rows, rows refused for a NaN or an infinity: theirs are NaN / -1).  part (optional): fp64, at least
    gmm_parts(N, D, K, GMM_ESTEP) doubles (the entry checks its size); None: the shared scratch."""
    N, D, ldx = _matrix(X, "X")
    K = _dense(means, "means", _F32, (None, D)).shape[0]
    _dense(prec, "prec", _F32, (K, D)); _dense(logc, "logc", _F64, (K,))
    _dense(log_prob_norm, "log_prob_norm", _F64, (N,)); _dense(estat, "estat", _F64, (2,))
    ldr = _matrix(resp, "resp", N, K, optional=True)[2] or K
    _dense(labels, "labels", _I64, N, optional=True)
    part = gmm_scratch(N, D, K, GMM_ESTEP, X.device) if part is None else _buffer(part, "part", _F64)
    check(lib.vsom_gmm_estep(ptr(X), ldx, N, D, ptr(means), ptr(prec), ptr(logc), K, ptr(resp), ldr, ptr(log_prob_norm),
                             ptr(labels), ptr(estat), ptr(part), part.numel(), stream()), "vsom_gmm_estep")
    return log_prob_norm


def gmm_mstep(X, resp, means_old, part):
    """The M-step's per-slab partial sums (nk, S1, S2 shifted at means_old f32 [K, D]) of X [N, D] under resp f32 [N, K]
    (both with any row stride) into part, fp64 [>= gmm_parts(N, D, K, GMM_MSTEP)] (the entry checks its size); gmm_params
    turns them into parameters."""
    N, D, ldx = _matrix(X, "X")
    K = _dense(means_old, "means_old", _F32, (None, D)).shape[0]
    _, _, ldr = _matrix(resp, "resp", N, K)
    _buffer(part, "part", _F64)
    check(lib.vsom_gmm_mstep(ptr(X), ldx, N, D, ptr(resp), ldr, ptr(means_old), K, ptr(part), part.numel(), stream()),
          "vsom_gmm_mstep")
    return part


def gmm_params(part, N, means_old, reg_covar, spherical, n_norm, estat, means, cov, prec, weights, logc, record):
    """New means f32 [K, D], cov fp64 ([K, D]; spherical: [K]), prec f32 [K, D], weights and logc fp64 [K] from gmm_mstep's
    part; weights = nk / n_norm, or nk / sum(nk) when n_norm == 0.  record fp64 [GMM_RECORD]: the lower bound estat[0] / N
    (estat fp64 [2], optional; None: NaN), the smallest nk, the smallest covariance, the covariances <= 0 or not finite, the
    refused rows."""
    K, D = _dense(means_old, "means_old", _F32, (None, None)).shape
    _dense(means, "means", _F32, (K, D)); _dense(prec, "prec", _F32, (K, D))
    _dense(cov, "cov", _F64, (K,) if spherical else (K, D))
    _dense(weights, "weights", _F64, (K,)); _dense(logc, "logc", _F64, (K,)); _dense(record, "record", _F64, (GMM_RECORD,))
    _dense(estat, "estat", _F64, (2,), optional=True); _buffer(part, "part", _F64)
    check(lib.vsom_gmm_params(ptr(part), part.numel(), int(N), D, K, ptr(means_old), float(reg_covar), int(bool(spherical)),
                              int(n_norm), ptr(estat), ptr(means), ptr(cov), ptr(prec), ptr(weights), ptr(logc), ptr(record),
                              stream()), "vsom_gmm_params")
    return record


def gmm_set_params(weights, cov, D, spherical, prec, logc, record, part=None):
    """prec f32 [K, D], logc fp64 [K] and record[GMM_MIN_COV], record[GMM_BAD_COV] from given weights fp64 [K] and
    covariances fp64 ([K, D]; spherical: [K]).  part (optional): fp64, at least gmm_parts(1, D, K, GMM_SET) doubles (the
    entry checks its size); None: the shared scratch."""
    K = _dense(weights, "weights", _F64, (None,)).numel()
    _dense(cov, "cov", _F64, (K,) if spherical else (K, D))
    _dense(prec, "prec", _F32, (K, D)); _dense(logc, "logc", _F64, (K,)); _dense(record, "record", _F64, (GMM_RECORD,))
    part = gmm_scratch(1, D, K, GMM_SET, weights.device) if part is None else _buffer(part, "part", _F64)
    check(lib.vsom_gmm_set_params(ptr(weights), ptr(cov), int(D), K, int(bool(spherical)), ptr(prec), ptr(logc), ptr(record),
                                  ptr(part), part.numel(), stream()), "vsom_gmm_set_params")
    return prec, logc


# ---------------------------------------------------------------- data-parallel exchange (RCCL)
COMM_ID_BYTES = 128


def comm_unique_id() -> bytes:
    """Rank 0: a fresh RCCL unique id (host bytes) to hand to every rank's comm_init."""
    import ctypes
    buf = ctypes.create_string_buffer(COMM_ID_BYTES)
    check(lib.vsom_comm_unique_id(buf), "vsom_comm_unique_id")
    return buf.raw


def comm_init(unique_id: bytes, world_size: int, rank: int):
    """Collective: build this process's communicator (the current HIP device is this rank's GPU)."""
    import ctypes
    assert len(unique_id) == COMM_ID_BYTES
    buf = ctypes.create_string_buffer(unique_id, COMM_ID_BYTES)
    check(lib.vsom_comm_init(buf, int(world_size), int(rank)), "vsom_comm_init")


def comm_info():
    import ctypes
    w, r = ctypes.c_int(), ctypes.c_int()
    check(lib.vsom_comm_info(ctypes.byref(w), ctypes.byref(r)), "vsom_comm_info")
    return w.value, r.value


def comm_allreduce_sum(t):
    """In-place sum of `t` over the ranks, enqueued on the launch stream (no host sync)."""
    _f32(t, "t")
    assert t.is_contiguous()
    check(lib.vsom_comm_allreduce_sum(ptr(t), t.numel(), stream()), "vsom_comm_allreduce_sum")
    return t


def comm_destroy():
    check(lib.vsom_comm_destroy(), "vsom_comm_destroy")


# ---------------------------------------------------------------- launch tape
def tape_begin() -> int:
    tid = int(lib.vsom_tape_begin())
    if tid <= 0:
        check(tid, "vsom_tape_begin")
    return tid


def tape_cut() -> int:
    seg = int(lib.vsom_tape_cut())
    if seg < 0:
        check(seg, "vsom_tape_cut")
    return seg


def tape_end() -> int:
    return int(lib.vsom_tape_end())


def tape_recording() -> int:
    """0 = not recording, 1 = recording, 2 = recording but paused."""
    return int(lib.vsom_tape_recording())


class tape_hole:
    """A call whose arguments change from step to step: executed but kept OFF the tape, which is cut around it (the host
    re-issues it between two replayed segments).  A no-op when no tape is being recorded."""

    def __enter__(self):
        self.active = tape_recording() == 1
        if self.active:
            tape_cut()
            check(lib.vsom_tape_pause(1), "vsom_tape_pause")

    def __exit__(self, *exc):
        if self.active:
            check(lib.vsom_tape_pause(0), "vsom_tape_pause")


def tape_replay(tape: int, segment: int):
    check(lib.vsom_tape_replay(int(tape), int(segment)), "vsom_tape_replay")


def tape_segment_ops(tape: int, segment: int) -> int:
    return int(lib.vsom_tape_segment_ops(int(tape), int(segment)))


def tape_destroy(tape: int):
    check(lib.vsom_tape_destroy(int(tape)), "vsom_tape_destroy")


# ---------------------------------------------------------------- agglomerative clustering (agglomerative.py)
# Evaluation wrappers like those between the `evaluation` banner and the RCCL section, under the same contract: every tensor
# passes _matrix / _dense / _buffer before its address goes to the library, and a refusal is a ValueError.
AGGLO_MAX_N = 16384                                              # csrc/agglomerative.hip: AG_MAX_N
AGGLO_EUCLIDEAN, AGGLO_MANHATTAN, AGGLO_COSINE = 0, 1, 2
AGGLO_WARD, AGGLO_AVERAGE, AGGLO_COMPLETE, AGGLO_SINGLE = 0, 1, 2, 3
AGGLO_STATUS = 4                                                 # int32 words of agglo_merge's status
AGGLO_MISSING, AGGLO_RESCANNED, AGGLO_RESCAN_STEPS = 0, 1, 2


def agglo_workspace_bytes(N, connectivity) -> int:
    """Bytes of agglo_merge's workspace: host arithmetic, 0 for N < 1 or N > AGGLO_MAX_N."""
    return int(lib.vsom_agglo_workspace_bytes(int(N), int(bool(connectivity))))


def agglo_matrix(ws, N):
    """The fp64 [N, N] matrix at the head of an agglo_merge workspace, as a view."""
    _buffer(ws, "ws", _U8, 8 * N * N)
    return ws[:8 * N * N].view(torch.float64).view(N, N)


def agglo_adjacency(ws, N):
    """The uint8 [N, N] adjacency of an agglo_merge workspace sized with connectivity, as a view."""
    at = (8 * N * N + 255) // 256 * 256
    _buffer(ws, "ws", _U8, at + N * N)
    return ws[at:at + N * N].view(N, N)


def agglo_distances(X, metric, squared, out, status):
    """out fp64 [N, N] contiguous = the distances between the rows of X f32 [N, D] (any row stride) in the direct form, all
    arithmetic in fp64: AGGLO_EUCLIDEAN (squared: the sum of squares, else its root), AGGLO_MANHATTAN, AGGLO_COSINE.
    Symmetric bit for bit, zero diagonal.  status int32 [2]: the values that are not finite, the zero rows (cosine)."""
    N, D, ldx = _matrix(X, "X")
    _dense(out, "out", _F64, (N, N)); _dense(status, "status", _I32, (2,))
    check(lib.vsom_agglo_distances(ptr(X), ldx, N, D, int(metric), int(bool(squared)), ptr(out), N, ptr(status), stream()),
          "vsom_agglo_distances")
    return out


def agglo_merge(ws, N, linkage, connectivity, children, distances, status):
    """The N - 1 merges of the matrix (and, connectivity: the adjacency) that ws holds -- uint8, at least
    agglo_workspace_bytes(N, connectivity) bytes (the entry checks its size), both overwritten -> children int32 [N - 1, 2]
    in scipy's numbering, distances fp64 [N - 1], status int32 [AGGLO_STATUS]: steps that found no adjacent pair, slots
    searched again, steps with such a slot.  Everything is enqueued; nothing is read back."""
    N = int(N)
    _buffer(ws, "ws", _U8)
    _dense(children, "children", _I32, (max(N - 1, 0), 2)); _dense(distances, "distances", _F64, (max(N - 1, 0),))
    _dense(status, "status", _I32, (AGGLO_STATUS,))
    check(lib.vsom_agglo_merge(ptr(ws), ws.numel(), N, int(linkage), int(bool(connectivity)), ptr(children), ptr(distances),
                               ptr(status), stream()), "vsom_agglo_merge")
    return children, distances


# ---------------------------------------------------------------- DBSCAN (dbscan.py)
# Evaluation wrappers under the contract stated at the agglomerative section: every tensor passes _matrix / _dense / _buffer
# before its address goes to the library, and a refusal is a ValueError.  No entry takes a workspace: every buffer is a
# typed output whose shape follows from N.  The bit matrix travels as int64 [N, dbscan_words(N)] (torch has no arithmetic
# on uint64; the 64 bits are the entry's): bit j & 63 of adj[i, j >> 6] is set iff rows i and j have a distance <= eps.
DBSCAN_MAX_N = 131072                                            # csrc/knn.hip: DBSCAN_MAX_N, 2 GiB of bits
DBSCAN_CLUSTERS, DBSCAN_CORE, DBSCAN_BORDER, DBSCAN_NOISE = 0, 1, 2, 3      # the words of dbscan_finish's record


def dbscan_words(N) -> int:
    """64-bit words in a row of the bit matrix of N rows."""
    return (int(N) + 63) // 64


def dbscan_neighbours(X, metric, eps, sq, adj, count, status):
    """adj int64 [N, dbscan_words(N)] = the eps-neighbourhood graph of the rows of X f32 [N, D] (any row stride) as bits:
    set iff (double)d <= eps with d the fp32 distance of umap_knn (DIST_EUCLIDEAN or DIST_COSINE), the diagonal set, the
    tail bits clear, a bad row empty in row and column, symmetric.  sq f32 [N]: the squared norms; count int32 [N]: the
    set bits of every row; status int64 [2]: the bad rows, the set bits.  All written in full; nothing is read back."""
    N, D, ldx = _matrix(X, "X")
    _dense(sq, "sq", _F32, (N,)); _dense(adj, "adj", _I64, (N, dbscan_words(N)))
    _dense(count, "count", _I32, (N,)); _dense(status, "status", _I64, (2,))
    check(lib.vsom_dbscan_neighbours(ptr(X), ldx, N, D, int(metric), float(eps), ptr(sq), ptr(adj), ptr(count), ptr(status),
                                     stream()), "vsom_dbscan_neighbours")
    return adj, count


def dbscan_threshold(M, eps, adj, count, status):
    """The same bit matrix from precomputed distances M [N, N]: float32 with any row stride, or float64 contiguous (what
    agglo_distances writes).  A NaN entry clears its bit, the diagonal is set.  status int64 [2]: NaN entries, set bits."""
    if isinstance(M, _Tensor) and M.dtype == _F64:
        N = _dense(M, "M", _F64, (None, None)).shape[0]
        _dense(M, "M", _F64, (N, N))
        ldm, wide = N, 1
    else:
        N, _, ldm = _matrix(M, "M")
        _matrix(M, "M", N, N)
        wide = 0
    _dense(adj, "adj", _I64, (N, dbscan_words(N))); _dense(count, "count", _I32, (N,)); _dense(status, "status", _I64, (2,))
    check(lib.vsom_dbscan_threshold(ptr(M), ldm, N, wide, float(eps), ptr(adj), ptr(count), ptr(status), stream()),
          "vsom_dbscan_threshold")
    return adj, count


def dbscan_init(count, min_samples, core, root):
    """core uint8 [N] = count >= min_samples; root int32 [N] = the row itself for a core row, -1 otherwise."""
    N = _dense(count, "count", _I32, (None,)).shape[0]
    _dense(core, "core", _U8, (N,)); _dense(root, "root", _I32, (N,))
    check(lib.vsom_dbscan_init(ptr(count), N, int(min_samples), ptr(core), ptr(root), stream()), "vsom_dbscan_init")
    return core, root


def dbscan_round(adj, core, root, rounds, changed):
    """`rounds` pairs of a hook and a pointer-jumping step over root, enqueued; changed int32 [1] is cleared first and
    raised when a hook moved a root.  Nothing is read back: the caller reads `changed` and repeats until it stays 0."""
    N = _dense(core, "core", _U8, (None,)).shape[0]
    _dense(adj, "adj", _I64, (N, dbscan_words(N))); _dense(root, "root", _I32, (N,)); _dense(changed, "changed", _I32, (1,))
    check(lib.vsom_dbscan_round(ptr(adj), N, ptr(core), ptr(root), int(rounds), ptr(changed), stream()), "vsom_dbscan_round")
    return changed


def dbscan_finish(adj, core, root, labels, record):
    """At the fixed point of dbscan_round: labels int64 [N] in sklearn's numbering (-1: noise) and record int32 [4]:
    clusters, core rows, border rows, noise rows (DBSCAN_CLUSTERS ..)."""
    N = _dense(core, "core", _U8, (None,)).shape[0]
    _dense(adj, "adj", _I64, (N, dbscan_words(N))); _dense(root, "root", _I32, (N,))
    _dense(labels, "labels", _I64, (N,)); _dense(record, "record", _I32, (4,))
    check(lib.vsom_dbscan_finish(ptr(adj), N, ptr(core), ptr(root), ptr(labels), ptr(record), stream()), "vsom_dbscan_finish")
    return labels, record


# ---------------------------------------------------------------- spectral embedding (spectral.py)
# Evaluation wrappers under the contract stated at the agglomerative section.  The graph is CSR on the device: int64 indptr
# [N + 1] and indices [nnz], fp64 data [nnz] (tsne_step's convention).  A block is an fp64 [N, l] tensor with innermost
# stride 1 and any row stride, l <= SPECTRAL_MAX_WIDTH; the blocks of one call share their row stride.
SPECTRAL_MAX_N = 131072                                          # csrc/spectral.hip: SP_MAX_N
SPECTRAL_MAX_WIDTH = 32                                          # SP_MAX_L
SPECTRAL_CHUNK = 512                                             # SP_CHUNK: the entries of one chain of a row's sum
SPECTRAL_STATUS = 5                                              # int64 words of spectral_degrees' status
SPECTRAL_ISOLATED, SPECTRAL_BAD_INDEX, SPECTRAL_BAD_WEIGHT, SPECTRAL_BAD_INDPTR, SPECTRAL_HEAVY = 0, 1, 2, 3, 4


def _block(t, name, rows=None, cols=None, ld=None, optional=False):
    """An fp64 block: on the device, 2-D, innermost stride 1, `rows` x `cols` and of row stride `ld` where given ->
    (rows, cols, row stride); (0, 0, 0) for an optional None."""
    if t is None and optional:
        return 0, 0, 0
    if isinstance(t, _Tensor) and t.is_cuda and t.dtype == _F64 and t.dim() == 2:
        r, c = t.shape
        stride = t.stride(0) if r > 1 else (ld if ld is not None else c)
        if (t.stride(1) == 1 or not t.numel()) and (rows is None or rows == r) and (cols is None or cols == c) and (
                ld is None or ld == stride):
            return r, c, stride
    _device(t, name, _F64)
    raise ValueError(f"{name}: expected a [{'any' if rows is None else rows}, {'any' if cols is None else cols}] float64 block with "
                     f"innermost stride 1{'' if ld is None else f' and row stride {ld}'}, got shape {tuple(t.shape)} with strides "
                     f"{t.stride()}")


def _csr(indptr, indices, data):
    """-> (N, nnz) of a device CSR triple."""
    N = _dense(indptr, "indptr", _I64, (None,)).shape[0] - 1
    nnz = _dense(indices, "indices", _I64, (None,)).shape[0]
    _dense(data, "data", _F64, (nnz,))
    if N < 1:
        raise ValueError(f"indptr: expected at least 2 elements, got {N + 1}")
    return N, nnz


def spectral_degrees(indptr, indices, data, d, s, heavy, status):
    """d fp64 [N] = the row sums of the CSR matrix without its diagonal, s fp64 [N] = d^-1/2 (0 for a row without weight),
    heavy int32 [N]: the rows of more than SPECTRAL_CHUNK entries (status[SPECTRAL_HEAVY] of them), status int64
    [SPECTRAL_STATUS]: isolated rows, indices outside [0, N), weights negative or not finite, bad indptr pairs, long rows."""
    N, nnz = _csr(indptr, indices, data)
    _dense(d, "d", _F64, (N,)); _dense(s, "s", _F64, (N,)); _dense(heavy, "heavy", _I32, (N,))
    _dense(status, "status", _I64, (SPECTRAL_STATUS,))
    check(lib.vsom_spectral_degrees(ptr(indptr), ptr(indices), ptr(data), N, nnz, ptr(d), ptr(s), ptr(heavy), ptr(status), stream()),
          "vsom_spectral_degrees")
    return d, s


def spectral_spmm(indptr, indices, data, s, Y1, Y0, out, alpha=1.0, c=0.0, beta=0.0, heavy=None, n_heavy=0):
    """out = alpha (M Y1 - c Y1) - beta Y0 with M = diag(s) A diag(s), A's diagonal skipped; Y0 may be None.  heavy /
    n_heavy: the list spectral_degrees wrote, or None (same bits, long rows then occupy one lane group each)."""
    N, nnz = _csr(indptr, indices, data)
    _dense(s, "s", _F64, (N,))
    _, l, ld = _block(Y1, "Y1", N)
    _block(Y0, "Y0", N, l, ld, optional=True); _block(out, "out", N, l, ld)
    _buffer(heavy, "heavy", _I32, int(n_heavy), optional=True)
    check(lib.vsom_spectral_spmm(ptr(indptr), ptr(indices), ptr(data), ptr(s), N, nnz, ptr(heavy), int(n_heavy) if heavy is not None else 0,
                                 ptr(Y1), ptr(Y0), ptr(out), ld, l, float(alpha), float(c), float(beta), stream()), "vsom_spectral_spmm")
    return out


def spectral_slabs(N) -> int:
    """The slab count the estimators use: a function of N alone, so that a fit is reproducible."""
    return max(1, min(512, int(N) // 256))


def spectral_ws_size(N, l, slabs) -> int:
    return int(lib.vsom_spectral_ws_size(int(N), int(l), int(slabs)))


def spectral_gram(V, W, G, H, slabs=None):
    """G fp64 [l, l] = V^T V and, with W and H, H = V^T W: slabs of rows summed in slab order."""
    N, l, ld = _block(V, "V")
    _block(W, "W", N, l, ld, optional=True)
    _dense(G, "G", _F64, (l, l)); _dense(H, "H", _F64, (l, l), optional=True)
    slabs = spectral_slabs(N) if slabs is None else int(slabs)
    need = spectral_ws_size(N, l, slabs)
    ws = scratch(need, V.device)
    check(lib.vsom_spectral_gram(ptr(V), ptr(W), ld, N, l, slabs, ptr(G), ptr(H), ptr(ws), need, stream()), "vsom_spectral_gram")
    return G, H


def spectral_rotate(V, T, out):
    """out [N, l_out] = V [N, l] T, T fp64 [l, l_out] dense on the device."""
    N, l, ldv = _block(V, "V")
    l_out = _dense(T, "T", _F64, (l, None)).shape[1]
    _, _, ldo = _block(out, "out", N, l_out)
    check(lib.vsom_spectral_rotate(ptr(V), ldv, N, l, ptr(T), l_out, ptr(out), ldo, stream()), "vsom_spectral_rotate")
    return out


def spectral_residual(V, W, theta, out, slabs=None):
    """out fp64 [l] = the squared norms of the columns of W - V diag(theta), from the differences themselves."""
    N, l, ld = _block(V, "V")
    _block(W, "W", N, l, ld)
    _dense(theta, "theta", _F64, (l,)); _dense(out, "out", _F64, (l,))
    slabs = spectral_slabs(N) if slabs is None else int(slabs)
    need = spectral_ws_size(N, l, slabs)
    ws = scratch(need, V.device)
    check(lib.vsom_spectral_residual(ptr(V), ptr(W), ld, N, l, ptr(theta), slabs, ptr(out), ptr(ws), need, stream()),
          "vsom_spectral_residual")
    return out


def spectral_embed(V, s, first, E, sign):
    """E f32 [N, n] = sign[j] * (s[i] * V[i, first + j]), rounded once; sign fp64 [n] (written) makes the entry of largest
    magnitude of every column positive, the smaller row on a tie."""
    N, l, ldv = _block(V, "V")
    _dense(s, "s", _F64, (N,))
    _, n, lde = _matrix(E, "E", N)
    _dense(sign, "sign", _F64, (n,))
    if not 0 <= int(first) <= l - n:
        raise ValueError(f"first: columns [{first}, {int(first) + n}) are not inside the block's {l}")
    check(lib.vsom_spectral_embed(ptr(V), ldv, ptr(s), N, int(first), n, ptr(E), lde, ptr(sign), stream()), "vsom_spectral_embed")
    return E


# ---------------------------------------------------------------- HDBSCAN (hdbscan.py)
# Evaluation wrappers under the contract stated at the agglomerative section.  No entry takes a workspace: every buffer is
# typed and its shape follows from N.  A row's candidate travels as int64 (the 64 bits are the entry's): the fp32 bits of
# the mutual-reachability distance in the high word, the other row in the low word, -1 (all ones) for none.
HDBSCAN_MAX_N = DBSCAN_MAX_N                                     # csrc/knn.hip: the limit of the DBSCAN section
HDBSCAN_COMPONENTS, HDBSCAN_EDGES, HDBSCAN_BAD, HDBSCAN_ROUNDS = 0, 1, 2, 3       # the words of the entries' record


def hdbscan_work(N) -> int:
    """int64 words of hdbscan_merge's work array."""
    return 2 * int(N)


def hdbscan_init(comp, edges, record):
    """comp int32 [N] = the row itself; edges int32 [N, 3] = -1; record int32 [4] = (N components, 0 edges, 0 bad rows,
    0 rounds)."""
    N = _dense(comp, "comp", _I32, (None,)).shape[0]
    _dense(edges, "edges", _I32, (N, 3)); _dense(record, "record", _I32, (4,))
    check(lib.vsom_hdbscan_init(N, ptr(comp), ptr(edges), ptr(record), stream()), "vsom_hdbscan_init")
    return comp, edges


def hdbscan_nearest(X, metric, core, comp, sq, best, record):
    """best int64 [N] = for every row of X f32 [N, D] (any row stride) the least (w, j) over the rows j of another
    component, w = max(core[i], core[j], d(i, j)) in fp32 with d the distance of umap_knn (DIST_EUCLIDEAN or DIST_COSINE),
    packed (bits of w) << 32 | j; -1 without one.  core f32 [N], comp int32 [N]; sq f32 [N] receives the squared norms,
    record[HDBSCAN_BAD] the bad rows.  Nothing is read back."""
    N, D, ldx = _matrix(X, "X")
    _dense(core, "core", _F32, (N,)); _dense(comp, "comp", _I32, (N,)); _dense(sq, "sq", _F32, (N,))
    _dense(best, "best", _I64, (N,)); _dense(record, "record", _I32, (4,))
    check(lib.vsom_hdbscan_nearest(ptr(X), ldx, N, D, int(metric), ptr(core), ptr(comp), ptr(sq), ptr(best), ptr(record), stream()),
          "vsom_hdbscan_nearest")
    return best


def hdbscan_nearest_matrix(M, core, comp, best, record):
    """The same candidates from precomputed distances M [N, N]: float32 with any row stride, or float64 contiguous (what
    agglo_distances writes).  w is the float32 rounding of max(core[i], core[j], M[i, j]).  An entry off the diagonal that
    is not finite in float32 offers nothing and is counted in record[HDBSCAN_BAD]."""
    if isinstance(M, _Tensor) and M.dtype == _F64:
        N = _dense(M, "M", _F64, (None, None)).shape[0]
        _dense(M, "M", _F64, (N, N))
        ldm, wide = N, 1
    else:
        N, _, ldm = _matrix(M, "M")
        _matrix(M, "M", N, N)
        wide = 0
    _dense(core, "core", _F32, (N,)); _dense(comp, "comp", _I32, (N,))
    _dense(best, "best", _I64, (N,)); _dense(record, "record", _I32, (4,))
    check(lib.vsom_hdbscan_nearest_matrix(ptr(M), ldm, N, wide, ptr(core), ptr(comp), ptr(best), ptr(record), stream()),
          "vsom_hdbscan_nearest_matrix")
    return best


def hdbscan_merge(best, comp, edges, work, record):
    """One Boruvka merge from the rows' candidates: every component's least edge under (w, lo, hi) goes to edges[label] as
    (lo, hi, bits of w), comp is relabelled, record's components, edges and rounds are updated.  work int64
    [hdbscan_work(N)] is overwritten.  Nothing is read back: the caller reads record and repeats until one component is left."""
    N = _dense(comp, "comp", _I32, (None,)).shape[0]
    _dense(best, "best", _I64, (N,)); _dense(edges, "edges", _I32, (N, 3))
    _dense(work, "work", _I64, (hdbscan_work(N),)); _dense(record, "record", _I32, (4,))
    check(lib.vsom_hdbscan_merge(ptr(best), N, ptr(comp), ptr(edges), ptr(work), ptr(record), stream()), "vsom_hdbscan_merge")
    return comp, edges


# ---------------------------------------------------------------- attention rollout (attention_rollout.py)
# Evaluation wrappers under the contract stated at the agglomerative section.  qkv is a block's saved [B N, 3 H hd] buffer
# (columns [3][H][hd]); the state is f32 [B, N].  4-byte accesses only: a qkv view at any float offset is legal input.
ROLLOUT_FUSIONS = {"mean": 0, "max": 1, "min": 2}                # csrc/attention_rollout.hip: RO_MEAN, RO_MAX, RO_MIN
ROLLOUT_MAX_N = 320                                              # RO_MAX_CHUNKS * 64


def attention_rollout_ws_size(B, N, H, hd) -> int:
    """Bytes of attention_rollout_step's workspace; 0 for a shape outside the kernel's limits."""
    return int(lib.vsom_attention_rollout_ws_size(int(B), int(N), int(H), int(hd)))


def attention_rollout_step(qkv, v_in, v_out, B, N, H, hd, fusion, alpha):
    """v_out[b, j] = sum_i v_in[b, i] A_b[i, j], A_b the residual-mixed, head-fused, row-normalised attention matrix of the
    block whose qkv this is (include/vitsom_hip.h has the formulas and the order of every sum).  fusion is a key of
    ROLLOUT_FUSIONS or its code; 0 < alpha <= 1.  v_out must not overlap v_in.  No N x N matrix is formed."""
    B, N, H, hd = int(B), int(N), int(H), int(hd)
    _dense(qkv, "qkv", _F32, (B * N, 3 * H * hd))
    _dense(v_in, "v_in", _F32, (B, N)); _dense(v_out, "v_out", _F32, (B, N))
    code = ROLLOUT_FUSIONS.get(fusion, fusion) if isinstance(fusion, str) else fusion
    if code not in (0, 1, 2):
        raise ValueError(f"fusion: expected one of {sorted(ROLLOUT_FUSIONS)} (or 0, 1, 2), got {fusion!r}")
    need = attention_rollout_ws_size(B, N, H, hd)
    ws = scratch(need, qkv.device)
    check(lib.vsom_attention_rollout_step(ptr(qkv), ptr(v_in), ptr(v_out), B, N, H, hd, int(code), float(alpha), ptr(ws), need, stream()),
          "vsom_attention_rollout_step")
    return v_out


def attention_rollout(qkvs, w, H, hd, fusion="mean", alpha=0.5):
    """The rollout of the query weights w f32 [B, N] over the blocks whose saved qkv buffers are listed in qkvs, in forward
    order: the step of the last block first, down to the first of the list.  Two [B, N] buffers take turns; the result is a
    fresh tensor and w is not written."""
    qkvs = list(qkvs)
    if not qkvs:
        raise ValueError("qkvs: expected at least one block's qkv buffer")
    B, N = _dense(w, "w", _F32, (None, None)).shape
    bufs, cur = [None, None], w
    for k, qkv in enumerate(reversed(qkvs)):
        if bufs[k & 1] is None:
            bufs[k & 1] = torch.empty_like(w)
        cur = attention_rollout_step(qkv, cur, bufs[k & 1], B, N, H, hd, fusion, alpha)
    return cur
