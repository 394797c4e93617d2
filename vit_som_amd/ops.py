"""Tensor-level wrappers over the C-ABI (one per entry point of include/vitsom_hip.h).

Every wrapper validates device / dtype / inner-stride, passes raw device pointers, row strides
and torch's current HIP stream, and raises ``VsomError`` on a non-zero status.  Nothing here
computes: there is no eager fallback.
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
    """table[a[i], b[i]] += 1 (int64 device tensors; table is [na, nb] int64, accumulated)."""
    assert a.dtype == torch.int64 and b.dtype == torch.int64 and table.dtype == torch.int64 and bad.dtype == torch.int32
    assert a.is_cuda and a.is_contiguous() and b.is_contiguous() and table.is_contiguous() and a.numel() == b.numel()
    na, nb = table.shape
    check(lib.vsom_contingency(ptr(a), ptr(b), a.numel(), na, nb, ptr(table), ptr(bad), stream()), "vsom_contingency")
    return table


def argmax_rows(x, out):
    rows, cols = x.shape
    _f32(x, "x")
    assert out.dtype == torch.int64
    check(lib.vsom_argmax_rows(ptr(x), _rows(x), rows, cols, ptr(out), stream()), "vsom_argmax_rows")
    return out


def proto_mosaic(pred, n, p, C, k0, map_size, images=None, canvas=None, gap=1):
    """Decoder output `pred` [chunk * (n + 1), p*p*C] -> images[k0 : k0 + chunk] ([K, C, S, S] float32) and / or the cells
    k0 .. k0 + chunk - 1 of the uint8 RGB `canvas` of the rows x cols map (see vsom_proto_mosaic)."""
    _f32(pred, "pred")
    rows, cols = int(map_size[0]), int(map_size[1])
    K, pd = rows * cols, p * p * C
    assert pred.is_contiguous() and pred.dim() == 2 and pred.shape[1] == pd and pred.shape[0] % (n + 1) == 0
    chunk, S = pred.shape[0] // (n + 1), int(round(n ** 0.5)) * p
    if images is not None:
        _f32(images, "images")
        assert images.is_contiguous() and tuple(images.shape) == (K, C, S, S)
    if canvas is not None:
        assert canvas.is_cuda and canvas.dtype == torch.uint8 and canvas.is_contiguous()
        assert tuple(canvas.shape) ==(rows * S + (rows - 1) * gap, cols * S + (cols - 1) * gap, 3)
    check(lib.vsom_proto_mosaic(ptr(pred), chunk, int(n), int(p), int(C), ptr(images), ptr(canvas), int(k0), K, rows, cols,
                                int(gap), stream()), "vsom_proto_mosaic")


def last_label(bmu, label, first_ordinal, cells, bad):
    """cells[bmu[i]] = max(cells[bmu[i]], (first_ordinal + i + 1) << 32 | label[i]) (cells: [K] int64, zeroed by the caller)."""
    assert bmu.dtype == torch.int64 and label.dtype == torch.int64 and cells.dtype == torch.int64 and bad.dtype == torch.int32
    assert bmu.is_cuda and bmu.is_contiguous() and label.is_contiguous() and cells.is_contiguous() and bmu.numel() == label.numel()
    check(lib.vsom_last_label(ptr(bmu), ptr(label), bmu.numel(), int(first_ordinal), cells.numel(), ptr(cells), ptr(bad),
                              stream()), "vsom_last_label")
    return cells


def map_stats(dist, bmu, grid_positions, adj_r2, first_ordinal, hits, qe_fix, te, nearest, bad, second=None):
    """One batch folded into the map-quality accumulators (see vsom_map_stats): hits / qe_fix [K] and te [1] int64 zeroed by
    the caller, nearest [K] int64 set to -1 (all-ones), bad [1] int32; `second` [B] int64 receives the runner-up units."""
    _f32(dist, "dist")
    _f32(grid_positions, "grid_positions")
    B, K = dist.shape
    assert dist.is_contiguous() and grid_positions.is_contiguous() and tuple(grid_positions.shape) == (K, 2)
    assert bmu.dtype == torch.int64 and bmu.is_contiguous() and bmu.numel() == B
    for t, n in ((hits, K), (qe_fix, K), (te, 1), (nearest, K)):
        assert t.dtype == torch.int64 and t.is_cuda and t.is_contiguous() and t.numel() == n
    assert bad.dtype == torch.int32 and bad.numel() == 1
    if second is not None:
        assert second.dtype == torch.int64 and second.is_contiguous() and second.numel() == B
    check(lib.vsom_map_stats(ptr(dist), ptr(bmu), B, K, ptr(grid_positions), float(adj_r2), int(first_ordinal), ptr(hits),
                             ptr(qe_fix), ptr(te), ptr(nearest), ptr(bad), ptr(second), stream()), "vsom_map_stats")


def umatrix(W, grid_positions, adj_r2, distance):
    """-> (u [K] f32, nbr_idx [K, 8] int32, nbr_dist [K, 8] f32) on the device (see vsom_umatrix).  The status word is read
    here, after the launch: a unit with more than 8 units within adj_r2 raises VsomError (VSOM_EUNSUPPORTED)."""
    _f32(W, "W")
    _f32(grid_positions, "grid_positions")
    K, L = W.shape
    assert W.is_contiguous() and grid_positions.is_contiguous() and tuple(grid_positions.shape) == (K, 2)
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


def augment_plan(index, params, N, H, S, scale, log_ratio, scale2, log_ratio2, flip_p, erase_p, seed, epoch):
    """params[b] <- the augmentation plan of row index[b] of a data set of N rows in `epoch` (see vsom_augment_plan);
    scale2 = None: one crop."""
    assert index.is_cuda and index.dtype == torch.int64 and index.is_contiguous() and index.dim() == 1
    assert params.is_cuda and params.dtype == torch.int32 and params.is_contiguous()
    assert params.dim() == 2 and params.shape[0] >= index.numel() and params.shape[1] == AUGMENT_PARAMS
    two = scale2 is not None
    s2, l2 = (scale2, log_ratio2) if two else ((0.0, 0.0), (0.0, 0.0))
    check(lib.vsom_augment_plan(ptr(index), int(N), index.numel(), int(H), int(S), float(scale[0]), float(scale[1]), float(log_ratio[0]),
                                float(log_ratio[1]), int(two), float(s2[0]), float(s2[1]), float(l2[0]), float(l2[1]),
                                float(flip_p), float(erase_p), int(seed), int(epoch), ptr(params), stream()), "vsom_augment_plan")
    return params


def augment_batch(src, index, params, out, S, R, off, mean, std, seed, epoch, out_u8=None):
    """out[b] <- the transformed row index[b] of the uint8 set `src` [N, C, H, W] (see vsom_augment_batch); params = None: the
    whole image, no flip, no erase."""
    assert src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous() and src.dim() == 4
    assert index.is_cuda and index.dtype == torch.int64 and index.is_contiguous() and index.dim() == 1
    N, C, H, W = src.shape
    B = index.numel()
    _f32(out, "out"), _f32(mean, "mean"), _f32(std, "std")
    assert out.is_contiguous() and out.numel() >= B * C * S * S and mean.numel() == C and std.numel() == C
    if params is not None:
        assert params.is_cuda and params.dtype == torch.int32 and params.is_contiguous()
        assert params.shape[0] >= B and params.shape[1] == AUGMENT_PARAMS
    if out_u8 is not None:
        assert out_u8.is_cuda and out_u8.dtype == torch.uint8 and out_u8.is_contiguous() and out_u8.numel() >= B * C * S * S
    check(lib.vsom_augment_batch(ptr(src), N, C, H, W, ptr(index), ptr(params), B, int(S), int(R), int(off), ptr(mean), ptr(std),
                                 int(seed), int(epoch), ptr(out), ptr(out_u8), stream()), "vsom_augment_batch")
    return out


RANDAUG_PARAMS = 72


def _pack_fill(fill):
    fill = tuple(int(v) for v in fill) + (0,) * (3 - len(fill))
    assert len(fill) == 3 and all(0 <= v <= 255 for v in fill)
    return fill[0] | fill[1] << 8 | fill[2] << 16


def randaug_plan(index, ra, N, S, randaug_n, autoaugment, flip1_p, fill_tv, fill_timm, seed, epoch):
    """ra[b] <- the RandAugment / rand-m9 record of row index[b] in `epoch` (see vsom_randaug_plan); fills: one level per channel."""
    assert index.is_cuda and index.dtype == torch.int64 and index.is_contiguous() and index.dim() == 1
    assert ra.is_cuda and ra.dtype == torch.int32 and ra.is_contiguous()
    assert ra.dim() == 2 and ra.shape[0] >= index.numel() and ra.shape[1] == RANDAUG_PARAMS
    check(lib.vsom_randaug_plan(ptr(index), int(N), index.numel(), int(S), int(randaug_n), int(bool(autoaugment)), float(flip1_p),
                                _pack_fill(fill_tv), _pack_fill(fill_timm), int(seed), int(epoch), ptr(ra), stream()), "vsom_randaug_plan")
    return ra


def augment_batch_ra(src, index, params, ra, out, S, mean, std, seed, epoch, out_u8=None):
    """out[b] <- the training transform of row index[b] with the op slots of `ra` between the crops (see vsom_augment_batch_ra)."""
    assert src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous() and src.dim() == 4
    assert index.is_cuda and index.dtype == torch.int64 and index.is_contiguous() and index.dim() == 1
    N, C, H, W = src.shape
    B = index.numel()
    _f32(out, "out"), _f32(mean, "mean"), _f32(std, "std")
    assert out.is_contiguous() and out.numel() >= B * C * S * S and mean.numel() == C and std.numel() == C
    for t, width in ((params, AUGMENT_PARAMS), (ra, RANDAUG_PARAMS)):
        assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.shape[0] >= B and t.shape[1] == width
    if out_u8 is not None:
        assert out_u8.is_cuda and out_u8.dtype == torch.uint8 and out_u8.is_contiguous() and out_u8.numel() >= B * C * S * S
    check(lib.vsom_augment_batch_ra(ptr(src), N, C, H, W, ptr(index), ptr(params), ptr(ra), B, int(S), ptr(mean), ptr(std), int(seed),
                                    int(epoch), ptr(out), ptr(out_u8), stream()), "vsom_augment_batch_ra")
    return out


# ---------------------------------------------------------------- data pipeline, image sets of varying size
def augment_plan_ragged(index, shapes, params, S, scale, log_ratio, scale2, log_ratio2, flip_p, erase_p, seed, epoch):
    """augment_plan with box 1 drawn on each sample's own (H_n, W_n) = shapes[index[b]] (see vsom_augment_plan_ragged)."""
    assert index.is_cuda and index.dtype == torch.int64 and index.is_contiguous() and index.dim() == 1
    assert shapes.is_cuda and shapes.dtype == torch.int32 and shapes.is_contiguous() and shapes.dim() == 2 and shapes.shape[1] == 2
    assert params.is_cuda and params.dtype == torch.int32 and params.is_contiguous()
    assert params.dim() == 2 and params.shape[0] >= index.numel() and params.shape[1] == AUGMENT_PARAMS
    two = scale2 is not None
    s2, l2 = (scale2, log_ratio2) if two else ((0.0, 0.0), (0.0, 0.0))
    check(lib.vsom_augment_plan_ragged(ptr(index), ptr(shapes), shapes.shape[0], index.numel(), int(S), float(scale[0]), float(scale[1]),
                                       float(log_ratio[0]), float(log_ratio[1]), int(two), float(s2[0]), float(s2[1]), float(l2[0]),
                                       float(l2[1]), float(flip_p), float(erase_p), int(seed), int(epoch), ptr(params), stream()),
          "vsom_augment_plan_ragged")
    return params


def augment_ragged_scratch_bytes(B: int, C: int, S: int) -> int:
    return lib.vsom_augment_ragged_scratch_bytes(int(B), int(C), int(S))


def augment_batch_ragged(data, offsets, shapes, C, max_h, max_w, index, params, out, S, R, mean, std, seed, epoch, scratch=None,
                         out_u8=None):
    """out[b] <- the transformed image index[b] of the ragged uint8 set (data, offsets, shapes) (see vsom_augment_batch_ragged);
    params = None: the evaluation transform Resize(R) -> CenterCrop(S); otherwise `scratch` (uint8,
    augment_ragged_scratch_bytes(B, C, S)) holds the image between the two crops."""
    assert data.is_cuda and data.dtype == torch.uint8 and data.is_contiguous() and data.dim() == 1
    assert offsets.is_cuda and offsets.dtype == torch.int64 and offsets.is_contiguous() and offsets.dim() == 1
    assert shapes.is_cuda and shapes.dtype == torch.int32 and shapes.is_contiguous() and tuple(shapes.shape) == (offsets.numel(), 2)
    assert index.is_cuda and index.dtype == torch.int64 and index.is_contiguous() and index.dim() == 1
    N, B = offsets.numel(), index.numel()
    _f32(out, "out"), _f32(mean, "mean"), _f32(std, "std")
    assert out.is_contiguous() and out.numel() >= B * C * S * S and mean.numel() == C and std.numel() == C
    if params is not None:
        assert params.is_cuda and params.dtype == torch.int32 and params.is_contiguous()
        assert params.shape[0] >= B and params.shape[1] == AUGMENT_PARAMS
        assert scratch is not None and scratch.is_cuda and scratch.dtype == torch.uint8 and scratch.is_contiguous()
    if out_u8 is not None:
        assert out_u8.is_cuda and out_u8.dtype == torch.uint8 and out_u8.is_contiguous() and out_u8.numel() >= B * C * S * S
    check(lib.vsom_augment_batch_ragged(ptr(data), data.numel(), ptr(offsets), ptr(shapes), N, int(C), int(max_h), int(max_w),
                                        ptr(index), ptr(params), B, int(S), int(R), ptr(mean), ptr(std), int(seed), int(epoch),
                                        ptr(scratch), 0 if scratch is None else scratch.numel(), ptr(out), ptr(out_u8), stream()),
          "vsom_augment_batch_ragged")
    return out


# ---------------------------------------------------------------- k-means (evaluate_kmeans)
def kmeans_workspace_bytes(N: int, D: int, k: int) -> int:
    return lib.vsom_kmeans_workspace_bytes(N, D, k)


def _kmeans_x(X):
    _f32(X, "X")
    assert X.dim() == 2, "X must be [N, D]"
    return X.shape[0], X.shape[1], _rows(X)


def kmeans_assign(X, centers, labels, prev_labels, mind, ws):
    """One Lloyd E-step + partial M-step: labels / mind written, cluster partials into ws."""
    N, D, ldx = _kmeans_x(X)
    _f32(centers, "centers"); _f32(mind, "mind")
    assert centers.is_contiguous() and centers.shape[1] == D and labels.dtype == torch.int64 and prev_labels.dtype == torch.int64
    assert labels.numel() == N and prev_labels.numel() == N and mind.numel() == N
    check(lib.vsom_kmeans_assign(ptr(X), ldx, N, D, ptr(centers), centers.shape[0], ptr(labels), ptr(prev_labels), ptr(mind),
                                 ptr(ws), ws.numel() * ws.element_size(), stream()), "vsom_kmeans_assign")


def kmeans_update(centers_old, centers_new, N, mind, counts, status, ws):
    """centers_new, counts [k] int64 and status [4] fp64 = (changed, center_shift_tot, empty, inertia)."""
    k, D = centers_old.shape
    assert centers_new.is_contiguous() and centers_old.is_contiguous() and counts.dtype == torch.int64 and status.dtype == torch.float64
    check(lib.vsom_kmeans_update(ptr(centers_old), ptr(centers_new), N, D, k, ptr(mind), ptr(counts), ptr(status), ptr(ws),
                                 ws.numel() * ws.element_size(), stream()), "vsom_kmeans_update")


def kmeans_relocate(X, labels, moves, centers_old, centers_new, counts, status, ws):
    """Apply the empty-cluster moves (int64 [m, 2] device tensor of (cluster, sample)) in order, then the centres again."""
    N, D, ldx = _kmeans_x(X)
    k = centers_old.shape[0]
    assert moves.dtype == torch.int64 and moves.is_contiguous() and moves.is_cuda
    check(lib.vsom_kmeans_relocate(ptr(X), ldx, N, D, k, ptr(labels), ptr(moves), moves.shape[0], ptr(centers_old),
                                   ptr(centers_new), ptr(counts), ptr(status), ptr(ws), ws.numel() * ws.element_size(),
                                   stream()), "vsom_kmeans_relocate")


def kmeanspp_dist(X, candidates, closest, dist, pots):
    """dist [T, N] = min(closest, squared distance to each candidate row); pots [T] fp64 = row sums of dist."""
    N, D, ldx = _kmeans_x(X)
    T = candidates.numel()
    assert candidates.dtype == torch.int64 and candidates.is_cuda and dist.shape == (T, N) and dist.is_contiguous()
    assert pots.dtype == torch.float64 and pots.numel() >= T
    check(lib.vsom_kmeanspp_dist(ptr(X), ldx, N, D, ptr(candidates), T, ptr(closest), ptr(dist), ptr(pots), stream()),
          "vsom_kmeanspp_dist")


def kmeans_colvar(X, k, out, ws):
    """out[0] = mean(var(X, axis=0)) in fp64."""
    N, D, ldx = _kmeans_x(X)
    assert out.dtype == torch.float64
    check(lib.vsom_kmeans_colvar(ptr(X), ldx, N, D, k, ptr(out), ptr(ws), ws.numel() * ws.element_size(), stream()),
          "vsom_kmeans_colvar")


# ---------------------------------------------------------------- UMAP (visualize_umap_progression)
UMAP_MAX_K = 64                                                  # csrc/knn.hip (KNN_MAX_K): one list entry per lane


def umap_knn(X, k, metric, knn_idx, knn_dist):
    """knn_idx int64 [N, k] / knn_dist f32 [N, k]: the exact k nearest rows of X (row itself first), ascending by
    (distance, index); metric DIST_EUCLIDEAN or DIST_COSINE."""
    N, D, ldx = _kmeans_x(X)
    assert knn_idx.dtype == torch.int64 and knn_idx.is_contiguous() and knn_idx.shape == (N, k)
    _f32(knn_dist, "knn_dist")
    assert knn_dist.is_contiguous() and knn_dist.shape == (N, k)
    ws = scratch(lib.vsom_umap_knn_workspace_bytes(N, k), X.device)
    check(lib.vsom_umap_knn(ptr(X), ldx, N, D, int(k), int(metric), ptr(knn_idx), ptr(knn_dist), ptr(ws), ws.numel(),
                            stream()), "vsom_umap_knn")
    return knn_idx, knn_dist


def umap_neg_sample(seed, epoch, edge, p, N) -> int:
    """The negative sample vsom_umap_epoch draws (host arithmetic)."""
    return int(lib.vsom_umap_neg_sample(int(seed), int(epoch), int(edge), int(p), int(N)))


def umap_epoch(indptr, indices, eps, next_s, eps_neg, next_neg, Y_in, Y_out, a, b, gamma, alpha, epoch, seed):
    """One synchronous layout epoch: Y_out from Y_in; next_s / next_neg (fp64 per edge) updated in place."""
    N, dim = Y_in.shape
    _f32(Y_in, "Y_in"); _f32(Y_out, "Y_out")
    assert Y_in.is_contiguous() and Y_out.is_contiguous() and Y_out.shape == (N, dim)
    assert indptr.dtype == indices.dtype == torch.int64 and indptr.numel() == N + 1
    nnz = indices.numel()
    for t in (eps, next_s, eps_neg, next_neg):
        assert t.dtype == torch.float64 and t.is_contiguous() and t.numel() == nnz and t.is_cuda
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
    (zeroed by the caller) counts refused edges; ws from umap_transform_workspace(M, k)."""
    M, k = knn_idx.shape
    N, dim = Y_train.shape
    _f32(Y_train, "Y_train"); _f32(Y, "Y")
    assert Y_train.is_contiguous() and Y.is_contiguous() and Y.shape == (M, dim)
    assert knn_idx.dtype == torch.int64 and knn_idx.is_contiguous() and knn_idx.is_cuda
    for t in (weights, eps):
        assert t.dtype == torch.float64 and t.is_contiguous() and t.shape == (M, k) and t.is_cuda
    assert status.dtype == torch.int32 and status.numel() == 1 and status.is_cuda
    assert ws.dtype == torch.uint8 and ws.is_cuda and ws.is_contiguous()
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
    ranges) are folded with this chunk.  exclude int64 [Nq]: a global bank ordinal each query never receives."""
    Nq, D, ldq = _kmeans_x(Q)
    Nb, Db, ldx = _kmeans_x(X)
    assert Db == D, "Q and X must have the same width"
    assert idx.dtype == torch.int64 and idx.is_contiguous() and idx.shape == (Nq, k)
    _f32(dist, "dist")
    assert dist.is_contiguous() and dist.shape == (Nq, k)
    if exclude is not None:
        assert exclude.dtype == torch.int64 and exclude.is_cuda and exclude.is_contiguous() and exclude.numel() == Nq
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
    N, D, lda = _kmeans_x(A)
    assert nbr.dtype == torch.int64 and nbr.is_cuda and nbr.is_contiguous() and nbr.dim() == 2 and nbr.shape[0] == N
    k = nbr.shape[1]
    for t in (less, tied):
        assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous() and t.shape == (N, k)
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
    clusters) and, with a workspace from silhouette_workspace, sums int64 [N, C]: the fixed-point distance sums.
    One synchronisation, to read status.  A NaN or infinite input (status[1] != 0) raises ValueError; a label outside the
    range does not: that row gets NaN, counts for nothing and is reported in status[0]."""
    N, D, ldx = _kmeans_x(X)
    C = int(n_clusters)
    assert labels.dtype == torch.int64 and labels.is_cuda and labels.is_contiguous() and labels.shape == (N,)
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
        assert ws.dtype == torch.uint8 and ws.is_cuda and ws.is_contiguous()
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
    """pred int64 [Nq] = first argmax of the fp64 class scores of each query's neighbour list (weights KNN_UNIFORM /
    KNN_DISTANCE / KNN_SOFTMAX); scores fp64 [Nq, n_classes] optionally; status int32 [2] (zeroed by the caller) counts
    refused neighbours and queries left without one (pred -1)."""
    Nq, k = idx.shape
    assert idx.dtype == torch.int64 and idx.is_cuda and idx.is_contiguous()
    _f32(dist, "dist")
    assert dist.is_contiguous() and dist.shape == (Nq, k)
    assert bank_labels.dtype == torch.int64 and bank_labels.is_cuda and bank_labels.is_contiguous()
    assert pred.dtype == torch.int64 and pred.is_contiguous() and pred.numel() == Nq
    assert status.dtype == torch.int32 and status.numel() == 2 and status.is_cuda
    if scores is not None:
        assert scores.dtype == torch.float64 and scores.is_contiguous() and scores.shape == (Nq, n_classes)
    check(lib.vsom_knn_vote(ptr(idx), ptr(dist), Nq, k, ptr(bank_labels), bank_labels.numel(), int(n_classes), int(weights),
                            float(temperature), ptr(pred), ptr(scores), ptr(status), stream()), "vsom_knn_vote")
    return pred


# ---------------------------------------------------------------- principal component analysis (pca.py)
PCA_MAX_WIDTH = 256                                              # csrc/pca.hip: PCA_MAX_L
PCA_PROJECT, PCA_BACKPROJECT = 0, 1                              # `which` of vsom_pca_slabs


def _pca_vec(t, n, name):
    """An optional contiguous f32 device vector of n elements (mean [D], scale [l])."""
    if t is not None:
        _f32(t, name)
        assert t.dim() == 1 and t.numel() == n and t.is_contiguous(), f"{name} must be a contiguous vector of {n}"
    return t


def _pca_f64(t, shape, name):
    assert t.dtype == torch.float64 and t.is_cuda and t.is_contiguous() and tuple(t.shape) == tuple(shape), \
        f"{name} must be a contiguous float64 device tensor of shape {tuple(shape)}"
    return t


def pca_slabs(N, D, l, which) -> int:
    """Floats of slab space pca_project (which = PCA_PROJECT) / pca_backproject (PCA_BACKPROJECT) take: host arithmetic."""
    return int(lib.vsom_pca_slabs(int(N), int(D), int(l), int(which)))


def pca_colstats(X, mean=None, var=None):
    """(mean f32 [D], var f64 [D]) of the columns of X [N, D]: fp64 sums in a fixed order, the mean rounded once, the
    unbiased variance about that rounded mean."""
    N, D, ldx = _kmeans_x(X)
    mean = torch.empty(D, dtype=torch.float32, device=X.device) if mean is None else _pca_vec(mean, D, "mean")
    var = torch.empty(D, dtype=torch.float64, device=X.device) if var is None else _pca_f64(var, (D,), "var")
    n_part = int(lib.vsom_pca_colstats_parts(N, D))
    part = scratch(8 * n_part, X.device)
    check(lib.vsom_pca_colstats(ptr(X), ldx, N, D, ptr(mean), ptr(var), ptr(part), part.numel() // 8, stream()), "vsom_pca_colstats")
    return mean, var


def pca_project(X, mean, B, scale, Y):
    """Y [N, l] = (X - mean) B^T diag(scale); mean [D] and scale [l] optional."""
    N, D, ldx = _kmeans_x(X)
    _f32(B, "B"); _f32(Y, "Y")
    assert B.dim() == 2 and B.shape[1] == D, "B must be [l, D]"
    l = B.shape[0]
    assert Y.dim() == 2 and Y.shape == (N, l), "Y must be [N, l]"
    _pca_vec(mean, D, "mean"); _pca_vec(scale, l, "scale")
    slabs = scratch(4 * pca_slabs(N, D, l, PCA_PROJECT), X.device)
    check(lib.vsom_pca_project(ptr(X), ldx, N, D, ptr(mean), ptr(B), _rows(B), l, ptr(scale), ptr(Y), _rows(Y), ptr(slabs),
                               slabs.numel() // 4, stream()), "vsom_pca_project")
    return Y


def pca_backproject(Y, X, mean, Zt):
    """Zt [l, D] = Y^T (X - mean); Y [N, l], mean [D] optional."""
    N, D, ldx = _kmeans_x(X)
    _f32(Y, "Y"); _f32(Zt, "Zt")
    assert Y.dim() == 2 and Y.shape[0] == N, "Y must be [N, l]"
    l = Y.shape[1]
    assert Zt.dim() == 2 and Zt.shape == (l, D), "Zt must be [l, D]"
    _pca_vec(mean, D, "mean")
    slabs = scratch(4 * pca_slabs(N, D, l, PCA_BACKPROJECT), X.device)
    check(lib.vsom_pca_backproject(ptr(Y), _rows(Y), ptr(X), ldx, N, D, ptr(mean), l, ptr(Zt), _rows(Zt), ptr(slabs),
                                   slabs.numel() // 4, stream()), "vsom_pca_backproject")
    return Zt


def pca_gram(Zt, G, B=None, H=None):
    """G f64 [l, l] = Zt Zt^T and, with B [l, D] and H f64 [l, l], H = B Zt^T: fp64 products and sums."""
    l, D, ldz = _kmeans_x(Zt)
    _pca_f64(G, (l, l), "G")
    assert (B is None) == (H is None), "B and H go together"
    if B is not None:
        _f32(B, "B")
        assert B.dim() == 2 and B.shape == (l, D), "B must have the shape of Zt"
        _pca_f64(H, (l, l), "H")
    check(lib.vsom_pca_gram(ptr(Zt), ldz, ptr(B), _rows(B) if B is not None else 0, l, D, ptr(G), ptr(H), stream()), "vsom_pca_gram")
    return G, H


def pca_rotate(T, Zt, Bout):
    """Bout [l_out, D] = T Zt, T f64 [l_out, l_in] on the device: fp64 accumulation, one rounding.  Bout may not overlap Zt."""
    l_in, D, ldz = _kmeans_x(Zt)
    assert T.dim() == 2 and T.shape[1] == l_in, "T must be [l_out, l_in]"
    l_out = T.shape[0]
    _pca_f64(T, (l_out, l_in), "T")
    _f32(Bout, "Bout")
    assert Bout.dim() == 2 and Bout.shape == (l_out, D), "Bout must be [l_out, D]"
    check(lib.vsom_pca_rotate(ptr(T), l_out, l_in, ptr(Zt), ldz, D, ptr(Bout), _rows(Bout), stream()), "vsom_pca_rotate")
    return Bout


def pca_reconstruct(Y, scale, B, mean, Xout):
    """Xout [M, D] = (Y diag(scale)) B + mean; Y [M, l], B [l, D], scale [l] and mean [D] optional."""
    M, l, ldy = _kmeans_x(Y)
    _f32(B, "B"); _f32(Xout, "Xout")
    assert B.dim() == 2 and B.shape[0] == l, "B must be [l, D]"
    D = B.shape[1]
    assert Xout.dim() == 2 and Xout.shape == (M, D), "Xout must be [M, D]"
    _pca_vec(scale, l, "scale"); _pca_vec(mean, D, "mean")
    check(lib.vsom_pca_reconstruct(ptr(Y), ldy, M, l, ptr(scale), ptr(B), _rows(B), D, ptr(mean), ptr(Xout), _rows(Xout), stream()),
          "vsom_pca_reconstruct")
    return Xout


# ---------------------------------------------------------------- Kohonen's batch map (SOMLayer.fit_batch)
def som_batch_accumulate(X, bmu, sums, counts, inv_norm=None, accumulate=False, bad=None):
    """counts [K] int64 = rows per unit, sums [K, D] float64 = per unit the sum of its rows of X [N, D] (times inv_norm [N]
    when given), every (unit, column) one fp64 chain in ascending row index (see vsom_som_batch_accumulate).  accumulate=True
    continues from what sums / counts hold: a row set cut into several calls gives the same bits as one call.
    bad: an int32 [1] device counter of BMUs outside [0, K) the caller zeroes and reads later; None: checked here (one
    host read) and raised as VsomError."""
    N, D, ldx = _kmeans_x(X)
    K = counts.numel()
    assert bmu.dtype == torch.int64 and bmu.is_cuda and bmu.dim() == 1 and bmu.is_contiguous() and bmu.numel() == N, \
        "bmu must be a contiguous int64 device vector of N"
    _pca_f64(sums, (K, D), "sums")
    assert counts.dtype == torch.int64 and counts.is_cuda and counts.dim() == 1 and counts.is_contiguous(), \
        "counts must be a contiguous int64 device vector"
    _pca_vec(inv_norm, N, "inv_norm")
    own = bad is None
    if own:
        bad = torch.zeros(1, dtype=torch.int32, device=X.device)
    assert bad.dtype == torch.int32 and bad.is_cuda and bad.numel() == 1
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
    """W_out [K, D] f32 = the batch-map update at radius sigma from sums [K, D] float64 and counts [K] int64 (see
    vsom_som_batch_update); normalize=True L2-normalises every row afterwards (the cosine map)."""
    K = counts.numel()
    assert sums.dim() == 2, "sums must be [K, D]"
    D = sums.shape[1]
    _pca_f64(sums, (K, D), "sums")
    assert counts.dtype == torch.int64 and counts.is_cuda and counts.dim() == 1 and counts.is_contiguous(), \
        "counts must be a contiguous int64 device vector"
    _f32(grid_positions, "grid_positions"); _f32(W_out, "W_out")
    assert grid_positions.is_contiguous() and tuple(grid_positions.shape) == (K, 2), "grid_positions must be [K, 2]"
    assert W_out.dim() == 2 and tuple(W_out.shape) == (K, D), "W_out must be [K, D]"
    n_part = int(lib.vsom_som_batch_update_parts(K))
    part = scratch(8 * n_part, sums.device)
    check(lib.vsom_som_batch_update(ptr(sums), ptr(counts), ptr(grid_positions), K, D, float(sigma), int(bool(normalize)), ptr(W_out),
                                    _rows(W_out), ptr(part), part.numel() // 8, stream()), "vsom_som_batch_update")
    return W_out


# ---------------------------------------------------------------- linear probe (linear_probe.py)
PROBE_MAX_CLASSES = 256                                          # csrc/linear_probe.hip: PROBE_MAX_C
PROBE_MAX_STEPS = 16                                             # the line search's ladder
LBFGS_MAX_MEMORY = 16
# the L-BFGS state record (state[:16]): indices
LBFGS_ALPHA0, LBFGS_GTP, LBFGS_GG, LBFGS_GMAX, LBFGS_COUNT, LBFGS_SKIPPED, LBFGS_ACCEPTED, LBFGS_SLOT, LBFGS_HEAD = range(9)
PROBE_STEP, PROBE_LS_STATUS, PROBE_F, PROBE_J = 12, 13, 14, 15
LBFGS_RECORD = 16


def _probe_labels(y, N):
    assert y.dtype == torch.int64 and y.is_cuda and y.dim() == 1 and y.is_contiguous() and y.numel() == N, \
        "y must be a contiguous int64 device vector of N"
    return y


def _probe_f64(t, n, name):
    """An optional contiguous fp64 device tensor of n elements."""
    if t is not None:
        assert t.dtype == torch.float64 and t.is_cuda and t.is_contiguous() and t.numel() == n, \
            f"{name} must be a contiguous float64 device tensor of {n} elements"
    return t


def probe_parts(N, C) -> int:
    """Doubles of scratch probe_residual / probe_linesearch take: host arithmetic."""
    return int(lib.vsom_probe_parts(int(N), int(C)))


def probe_fold(A, invstd, B, W=None, pen=None):
    """B f32 [C, D] = A o invstd (A fp64 [C, D], invstd fp64 [D]; one rounding); with W fp64 [C, D] and pen fp64 [3] also
    pen = (W.W, W.A, A.A)."""
    assert A.dim() == 2, "A must be [C, D]"
    C, D = A.shape
    _probe_f64(A, C * D, "A"); _probe_f64(invstd, D, "invstd")
    _f32(B, "B")
    assert B.dim() == 2 and tuple(B.shape) == (C, D), "B must be [C, D]"
    assert (W is None) == (pen is None), "W and pen go together"
    _probe_f64(W, C * D, "W"); _probe_f64(pen, 3, "pen")
    n_part = int(lib.vsom_probe_fold_parts(C, D)) if W is not None else 0
    part = scratch(8 * n_part, A.device)
    check(lib.vsom_probe_fold(ptr(A), ptr(invstd), C, D, ptr(B), _rows(B), ptr(W), ptr(pen), ptr(part), part.numel() // 8, stream()),
          "vsom_probe_fold")
    return B


def probe_residual(Z, b, y, R, loss, gb, status, pred=None, prob=None):
    """R f32 [N, C] = softmax(Z + b) - onehot(y), loss fp64 [1] = the summed cross-entropy, gb fp64 [C] = the column sums of
    R; pred int64 [N] and prob fp64 [N, C] optionally; status int32 [1] (zeroed by the caller) counts labels outside [0, C)."""
    N, C, ldz = _kmeans_x(Z)
    _f32(R, "R")
    assert R.dim() == 2 and tuple(R.shape) == (N, C), "R must be [N, C]"
    _probe_f64(b, C, "b"); _probe_f64(loss, 1, "loss"); _probe_f64(gb, C, "gb"); _probe_f64(prob, N * C, "prob")
    assert loss is not None and gb is not None
    _probe_labels(y, N)
    if pred is not None:
        _probe_labels(pred, N)
    assert status.dtype == torch.int32 and status.is_cuda and status.numel() == 1
    part = scratch(8 * probe_parts(N, C), Z.device)
    check(lib.vsom_probe_residual(ptr(Z), ldz, N, C, ptr(b), ptr(y), ptr(R), _rows(R), ptr(loss), ptr(gb), ptr(pred), ptr(prob),
                                  ptr(status), ptr(part), part.numel() // 8, stream()), "vsom_probe_residual")
    return R


def probe_linesearch(Z, Zp, b, pb, y, alpha0, nsteps, phi):
    """phi fp64 [nsteps]: the summed cross-entropy at Z + a_j Zp, b + a_j pb for a_j = alpha0 2^-j (alpha0 fp64 [1] on the
    device), in one launch."""
    N, C, ldz = _kmeans_x(Z)
    _f32(Zp, "Zp")
    assert Zp.dim() == 2 and tuple(Zp.shape) == (N, C) and _rows(Zp) == ldz, "Zp must have the shape and row stride of Z"
    assert (b is None) == (pb is None), "b and pb go together"
    _probe_f64(b, C, "b"); _probe_f64(pb, C, "pb"); _probe_f64(alpha0, 1, "alpha0"); _probe_f64(phi, int(nsteps), "phi")
    assert alpha0 is not None and phi is not None
    _probe_labels(y, N)
    part = scratch(8 * probe_parts(N, C), Z.device)
    check(lib.vsom_probe_linesearch(ptr(Z), ptr(Zp), ldz, N, C, ptr(b), ptr(pb), ptr(y), ptr(alpha0), int(nsteps), ptr(phi), ptr(part),
                                    part.numel() // 8, stream()), "vsom_probe_linesearch")
    return phi


def probe_step(phi, alpha0, f0, pen, gtp, lam, c1, Z, Zp, theta, p, s_new, rec):
    """The Armijo choice from the ladder phi, then Z += alpha Zp, theta += alpha p, s_new = alpha p; rec[12:16] =
    (alpha, status, F(alpha), j).  alpha0, f0, gtp fp64 [1], pen fp64 [3], rec fp64 [>= 16]: all on the device."""
    N, C, ldz = _kmeans_x(Z)
    _f32(Zp, "Zp")
    assert Zp.dim() == 2 and tuple(Zp.shape) == (N, C) and _rows(Zp) == ldz, "Zp must have the shape and row stride of Z"
    n = theta.numel()
    for t, k, name in ((phi, phi.numel(), "phi"), (alpha0, 1, "alpha0"), (f0, 1, "f0"), (pen, 3, "pen"), (gtp, 1, "gtp"),
                       (theta, n, "theta"), (p, n, "p"), (s_new, n, "s_new")):
        assert t is not None
        _probe_f64(t, k, name)
    assert rec.dtype == torch.float64 and rec.is_cuda and rec.is_contiguous() and rec.numel() >= LBFGS_RECORD
    check(lib.vsom_probe_step(ptr(phi), phi.numel(), ptr(alpha0), ptr(f0), ptr(pen), ptr(gtp), float(lam), float(c1), ptr(Z), ptr(Zp),
                              ldz, N, C, ptr(theta), ptr(p), ptr(s_new), n, ptr(rec), stream()), "vsom_probe_step")
    return rec


def probe_gradient(Zt, invstd, theta, gb, N, lam, g, g_prev=None, y_new=None):
    """g fp64 [n] = (Zt o invstd) / N + lam W, then gb / N when theta holds an intercept (n = C D + C); y_new = g - g_prev."""
    C, D, ldz = _kmeans_x(Zt)
    n = theta.numel()
    assert n in (C * D, C * D + C), "theta must hold C D or C D + C elements"
    intercept = n > C * D
    _probe_f64(invstd, D, "invstd"); _probe_f64(theta, n, "theta"); _probe_f64(g, n, "g")
    _probe_f64(gb, C, "gb"); _probe_f64(g_prev, n, "g_prev"); _probe_f64(y_new, n, "y_new")
    assert (g_prev is None) == (y_new is None), "g_prev and y_new go together"
    assert gb is not None or not intercept, "an intercept needs gb"
    check(lib.vsom_probe_gradient(ptr(Zt), ldz, ptr(invstd), ptr(theta), ptr(gb), C, D, int(intercept), int(N), float(lam), ptr(g_prev),
                                  ptr(g), ptr(y_new), stream()), "vsom_probe_gradient")
    return g


def lbfgs_state(m, device):
    """A zeroed state of the L-BFGS pieces for memory m: the record, the Gram matrix and the coefficients."""
    n = int(lib.vsom_lbfgs_state_doubles(int(m)))
    if n <= 0:
        raise ValueError(f"L-BFGS memory must be between 1 and {LBFGS_MAX_MEMORY}, got {m}")
    return torch.zeros(n, dtype=torch.float64, device=device)


def _lbfgs_args(S, Y, g, state):
    assert S.dim() == 2 and S.shape == Y.shape, "S and Y must be [m, n]"
    m, n = S.shape
    _probe_f64(S, m * n, "S"); _probe_f64(Y, m * n, "Y"); _probe_f64(g, n, "g")
    _probe_f64(state, int(lib.vsom_lbfgs_state_doubles(m)), "state")
    return m, n


def lbfgs_dots(S, Y, g, s_new, y_new, state, dots):
    """dots fp64 [3 (2 m + 3) + 1]: the products of (s_new, y_new, g) with every vector held, and max |g|, in one pass.
    s_new = y_new = None: there is no new pair."""
    m, n = _lbfgs_args(S, Y, g, state)
    assert (s_new is None) == (y_new is None), "s_new and y_new go together"
    _probe_f64(s_new, n, "s_new"); _probe_f64(y_new, n, "y_new"); _probe_f64(dots, 3 * (2 * m + 3) + 1, "dots")
    part = scratch(8 * int(lib.vsom_lbfgs_parts(n, m)), g.device)
    check(lib.vsom_lbfgs_dots(ptr(S), ptr(Y), ptr(g), ptr(s_new), ptr(y_new), n, m, int(s_new is not None), ptr(state), ptr(dots),
                              ptr(part), part.numel() // 8, stream()), "vsom_lbfgs_dots")
    return dots


def lbfgs_coeff(dots, m, has_new, state):
    """Takes the new pair in (or skips it), then the two-loop recursion on coefficients; has_new=False empties the history."""
    _probe_f64(dots, 3 * (2 * m + 3) + 1, "dots"); _probe_f64(state, int(lib.vsom_lbfgs_state_doubles(m)), "state")
    check(lib.vsom_lbfgs_coeff(ptr(dots), int(m), int(bool(has_new)), ptr(state), stream()), "vsom_lbfgs_coeff")
    return state


def lbfgs_combine(S, Y, g, s_new, y_new, state, p):
    """p fp64 [n] = the direction; an accepted pair is copied into its ring slot of S and Y first."""
    m, n = _lbfgs_args(S, Y, g, state)
    _probe_f64(s_new, n, "s_new"); _probe_f64(y_new, n, "y_new"); _probe_f64(p, n, "p")
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
    [N, k] at this perplexity; status int32 [1] (zeroed by the caller) counts the rows refused, which are not written."""
    _f32(knn_dist, "knn_dist")
    assert knn_dist.dim() == 2, "knn_dist must be [N, k]"
    N, ldk = knn_dist.shape[0], _rows(knn_dist)
    assert P.dim() == 2 and P.shape[0] == N, "P must be [N, k_eff]"
    k_eff = P.shape[1]
    _pca_f64(P, (N, k_eff), "P"); _pca_f64(beta, (N,), "beta")
    assert first >= 0 and first + k_eff <= knn_dist.shape[1], "columns [first, first + k_eff) must lie inside knn_dist"
    if knn_idx is not None:
        assert knn_idx.dtype == torch.int64 and knn_idx.is_cuda and knn_idx.shape == knn_dist.shape \
            and knn_idx.stride() == knn_dist.stride(), "knn_idx must be an int64 device tensor laid out as knn_dist"
    assert status.dtype == torch.int32 and status.is_cuda and status.numel() == 1
    check(lib.vsom_tsne_affinities(ptr(knn_dist), ptr(knn_idx), ldk, N, k_eff, int(first), int(bool(square)), float(perplexity),
                                   ptr(P), ptr(beta), ptr(status), stream()), "vsom_tsne_affinities")
    return P, beta


def _tsne_y(Y, name):
    _f32(Y, name)
    assert Y.dim() == 2 and Y.shape[1] == 2 and Y.is_contiguous(), f"{name} must be a contiguous [N, 2]"
    return Y.shape[0]


def tsne_repulsion(Y, rep, sumq, zpart):
    """rep fp64 [N, 2] = sum_j q^2 (y_i - y_j), sumq fp64 [N] = sum_j q over all j != i, q = 1 / (1 + |y_i - y_j|^2), and
    zpart fp64 [>= tsne_repulsion_parts(N)]: the sums of sumq over blocks of 64 rows (their sum is Z)."""
    N = _tsne_y(Y, "Y")
    _pca_f64(rep, (N, 2), "rep"); _pca_f64(sumq, (N,), "sumq")
    assert zpart.dtype == torch.float64 and zpart.is_cuda and zpart.dim() == 1 and zpart.is_contiguous()
    check(lib.vsom_tsne_repulsion(ptr(Y), N, ptr(rep), ptr(sumq), ptr(zpart), zpart.numel(), stream()), "vsom_tsne_repulsion")
    return rep, sumq, zpart


def tsne_step(indptr, indices, data, Y_in, Y_out, update, gains, rep, zpart, exaggeration, momentum, learning_rate, part,
              record=False):
    """One iteration: Y_out from Y_in, update and gains (f32 [N, 2]) in place, from tsne_repulsion's rep and zpart at Y_in
    and the joint P (CSR: int64, int64, fp64).  record: part fp64 [>= tsne_step_parts(N)] receives the (KL, |grad|^2)
    pairs of the row blocks; add them."""
    N = _tsne_y(Y_in, "Y_in")
    for t, name in ((Y_out, "Y_out"), (update, "update"), (gains, "gains")):
        assert _tsne_y(t, name) == N, f"{name} must be [N, 2]"
    assert indptr.dtype == indices.dtype == torch.int64 and indptr.is_cuda and indices.is_cuda
    assert indptr.is_contiguous() and indices.is_contiguous() and indptr.numel() == N + 1
    assert data.dtype == torch.float64 and data.is_cuda and data.is_contiguous() and data.numel() == indices.numel()
    _pca_f64(rep, (N, 2), "rep")
    for t in (zpart, part):
        assert t.dtype == torch.float64 and t.is_cuda and t.dim() == 1 and t.is_contiguous()
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


def _gmm_kd(means, prec, D):
    _f32(means, "means"); _f32(prec, "prec")
    assert means.dim() == 2 and means.shape[1] == D and means.is_contiguous(), "means must be a contiguous [K, D]"
    assert prec.shape == means.shape and prec.is_contiguous(), "prec must be a contiguous [K, D]"
    return means.shape[0]


def gmm_estep(X, means, prec, logc, resp, log_prob_norm, labels, estat, part=None):
    """log_prob_norm fp64 [N], resp f32 [N, K] (None: not wanted), labels int64 [N] (None likewise) of the mixture (means,
    prec f32 [K, D], logc fp64 [K]) in the direct form; estat fp64 [2] = (sum of log_prob_norm over the accepted rows, rows
    refused for a NaN or an infinity: theirs are NaN / -1)."""
    N, D, ldx = _kmeans_x(X)
    K = _gmm_kd(means, prec, D)
    _pca_f64(logc, (K,), "logc"); _pca_f64(log_prob_norm, (N,), "log_prob_norm"); _pca_f64(estat, (2,), "estat")
    ldr = K
    if resp is not None:
        _f32(resp, "resp")
        assert resp.dim() == 2 and tuple(resp.shape) == (N, K), "resp must be [N, K]"
        ldr = _rows(resp)
    if labels is not None:
        assert labels.dtype == torch.int64 and labels.is_cuda and labels.is_contiguous() and labels.numel() == N
    part = gmm_scratch(N, D, K, GMM_ESTEP, X.device) if part is None else part
    check(lib.vsom_gmm_estep(ptr(X), ldx, N, D, ptr(means), ptr(prec), ptr(logc), K, ptr(resp), ldr, ptr(log_prob_norm),
                             ptr(labels), ptr(estat), ptr(part), part.numel(), stream()), "vsom_gmm_estep")
    return log_prob_norm


def gmm_mstep(X, resp, means_old, part):
    """The M-step's per-slab partial sums (nk, S1, S2 shifted at means_old f32 [K, D]) into part, fp64
    [>= gmm_parts(N, D, K, GMM_MSTEP)]; gmm_params turns them into parameters."""
    N, D, ldx = _kmeans_x(X)
    _f32(resp, "resp"); _f32(means_old, "means_old")
    assert means_old.dim() == 2 and means_old.shape[1] == D and means_old.is_contiguous()
    K = means_old.shape[0]
    assert resp.dim() == 2 and tuple(resp.shape) == (N, K), "resp must be [N, K]"
    assert part.dtype == torch.float64 and part.is_cuda and part.dim() == 1 and part.is_contiguous()
    check(lib.vsom_gmm_mstep(ptr(X), ldx, N, D, ptr(resp), _rows(resp), ptr(means_old), K, ptr(part), part.numel(), stream()),
          "vsom_gmm_mstep")
    return part


def gmm_params(part, N, means_old, reg_covar, spherical, n_norm, estat, means, cov, prec, weights, logc, record):
    """New means f32 [K, D], cov fp64 ([K, D]; spherical: [K]), prec f32 [K, D], weights and logc fp64 [K] from gmm_mstep's
    part; weights = nk / n_norm, or nk / sum(nk) when n_norm == 0.  record fp64 [GMM_RECORD]: the lower bound estat[0] / N
    (estat None: NaN), the smallest nk, the smallest covariance, the covariances <= 0 or not finite, the refused rows."""
    K, D = means_old.shape
    _gmm_kd(means, prec, D)
    _f32(means_old, "means_old")
    assert means_old.is_contiguous() and means.shape[0] == K
    _pca_f64(cov, (K,) if spherical else (K, D), "cov")
    _pca_f64(weights, (K,), "weights"); _pca_f64(logc, (K,), "logc"); _pca_f64(record, (GMM_RECORD,), "record")
    if estat is not None:
        _pca_f64(estat, (2,), "estat")
    assert part.dtype == torch.float64 and part.is_cuda and part.dim() == 1 and part.is_contiguous()
    check(lib.vsom_gmm_params(ptr(part), part.numel(), int(N), D, K, ptr(means_old), float(reg_covar), int(bool(spherical)),
                              int(n_norm), ptr(estat), ptr(means), ptr(cov), ptr(prec), ptr(weights), ptr(logc), ptr(record),
                              stream()), "vsom_gmm_params")
    return record


def gmm_set_params(weights, cov, D, spherical, prec, logc, record, part=None):
    """prec f32 [K, D], logc fp64 [K] and record[GMM_MIN_COV], record[GMM_BAD_COV] from given weights fp64 [K] and
    covariances fp64 ([K, D]; spherical: [K])."""
    K = weights.numel()
    _pca_f64(weights, (K,), "weights"); _pca_f64(cov, (K,) if spherical else (K, D), "cov")
    _f32(prec, "prec")
    assert tuple(prec.shape) == (K, D) and prec.is_contiguous(), "prec must be a contiguous [K, D]"
    _pca_f64(logc, (K,), "logc"); _pca_f64(record, (GMM_RECORD,), "record")
    part = gmm_scratch(1, D, K, GMM_SET, weights.device) if part is None else part
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
