"""Inputs at the numerical edges of the kernels (saturated and offset softmax, LayerNorm rows with a large mean, a zero
variance or an outlier, exact GELU pre-activations, degenerate SOM operands, extreme AdamW gradients), each with its fp64
reference and its fp32 yardstick.  Pure torch on the CPU: tests/test_numeric_edges_cpu.py checks the cases themselves,
tests/test_numeric_edges_gpu.py runs them through vit_som_amd.ops.

A case holds
    inp   the fp32 inputs,
    ref   the outputs of the operation evaluated in fp64 on those inputs,
    y32   the same operation evaluated by plain torch in fp32 (the yardstick),
    e32   metric(y32[name], ref[name]) per output, in the metric the GPU test uses for that output,
    prop  the named property of the case, evaluated in the fp64 reference (a dict of booleans).
A kernel's error e_k on an output passes when e_k <= max(FLOOR, FACTOR * e32): FLOOR is the tolerance the entry point's
own test in test_ops_gpu.py uses on N(0, 1) inputs, and FACTOR = 4 covers another summation order and the fast
intrinsics (a few ulp each).  The evaluators take a `dtype` and, where a test needs one, a switch that selects a
deliberately wrong formulation (softmax without the max shift, one-pass variance, sign(0) = 1, a norm without the eps
clamp): test_numeric_edges_cpu.py feeds those to the same comparison and asserts that it rejects them."""
import functools
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import launch_plan_rows as R
from helpers import rel_err
from oracle import vitsom_oracle as O

FACTOR = 4.0
E32_MAX = 1e-3                                   # a case whose yardstick is worse than this would make the bound vacuous


def max_abs(a, ref):
    a, ref = torch.as_tensor(a).double(), torch.as_tensor(ref).double()
    return float((a - ref).abs().max()) if ref.numel() else 0.0


def bound(floor, e32):
    return max(floor, FACTOR * e32)


def accepts(e_k, floor, e32):
    """The comparison every edge test makes (NaN never passes)."""
    return bool(e_k <= bound(floor, e32))


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def make_case(name, inp, ref, y32, metric, prop):
    e32 = {k: metric[k](y32[k], ref[k]) for k in metric}
    return SimpleNamespace(name=name, inp=inp, ref=ref, y32=y32, metric=metric, e32=e32, prop=prop)


def finite(d):
    return all(bool(torch.isfinite(torch.as_tensor(v, dtype=torch.float64)).all()) for v in d.values())


# ------------------------------------------------------------------------------------------------------------ attention
# (B, N, H, hd): the smallest shapes that select each backward form (launch_plan_rows: attn.*), a ragged last tile,
# the scalar path, a second 64-key chunk and a single token
ATTN_SHAPES = [(2, 65, 2, 64), (2, 50, 2, 64), (2, 33, 2, 32), (2, 65, 2, 32), (2, 197, 2, 64), (2, 17, 2, 8), (2, 130, 1, 16),
               (2, 1, 2, 64)]
ATTN_KINDS = ["sat_first", "sat_last", "offset_pos", "offset_neg", "mixed"]
SAT_SCALE = 40.0
SAT_MARGIN = 20.0                                # a row is "affected" when the dominant key leads every other by this much
# rows of test_classifier_gpu.test_attention_q1_against_fp64 (hd 8, 32 and 64)
Q1_SHAPES = [(3, 5, 3, 8), (7, 37, 2, 8), (5, 17, 2, 32), (16, 65, 3, 64), (8, 197, 3, 64), (4, 257, 3, 64)]


def attention_ids(shapes=ATTN_SHAPES):
    """Every (shape, kind); the offset inputs need |score| > 88, which hd = 8 cannot reach inside e32 <= 1e-3."""
    return [(s, k) for s in shapes for k in ATTN_KINDS if not (s[3] == 8 and k.startswith("offset"))]


def attention_eval(qkv, dout, B, N, H, hd, dtype, shift=True):
    """softmax(q k^T / sqrt(hd)) v with its log-sum-exp, probabilities and input gradient.  shift=False: the softmax as
    exp(s) / sum exp(s), without the running-max subtraction."""
    x = qkv.to(dtype).clone().requires_grad_(True)
    q, k, v = x.reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-2, -1)) * hd ** -0.5
    if shift:
        p, lse = s.softmax(-1), torch.logsumexp(s, dim=-1)
    else:
        e = s.exp()
        z = e.sum(-1, keepdim=True)
        p, lse = e / z, z.log().squeeze(-1)
    out = (p @ v).transpose(1, 2).reshape(B, N, H * hd)
    out.backward(dout.to(dtype))
    return {"out": out.detach(), "lse": lse.detach(), "probs": p.detach(), "dqkv": x.grad, "scores": s.detach()}


def q1_eval(q, kv, dout, B, N, H, hd, dtype, shift=True):
    """Single-query attention (test_classifier_gpu._q1_ref) in `dtype`."""
    E = H * hd
    qq = q.to(dtype).view(B, H, hd).clone().requires_grad_(True)
    kvv = kv.to(dtype).clone().requires_grad_(True)
    k = kvv.view(B, N, 2, H, hd)[:, :, 0].permute(0, 2, 1, 3)
    v = kvv.view(B, N, 2, H, hd)[:, :, 1].permute(0, 2, 1, 3)
    s = torch.einsum("bhd,bhnd->bhn", qq, k) * hd ** -0.5
    if shift:
        p, lse = s.softmax(-1), torch.logsumexp(s, dim=-1)
    else:
        e = s.exp()
        z = e.sum(-1, keepdim=True)
        p, lse = e / z, z.log().squeeze(-1)
    o = torch.einsum("bhn,bhnd->bhd", p, v)
    o.backward(dout.to(dtype).view(B, H, hd))
    return {"out": o.detach().reshape(B, E), "lse": lse.detach(), "dq": qq.grad.reshape(B, E), "dkv": kvv.grad,
            "scores": s.detach().unsqueeze(2), "probs": p.detach().unsqueeze(2)}


def _saturation_prop(kind, scores, probs, dom, pairs):
    """Saturated: on every affected row (the dominant key `dom` leads by SAT_MARGIN) of the saturated (b, h) pairs the
    largest probability is above 1 - 1e-6, and there are such rows.  scores, probs: [B, H, rows, N]."""
    N = scores.shape[-1]
    sel = torch.zeros(scores.shape[:2], dtype=torch.bool)
    for b, h in pairs:
        sel[b, h] = True
    if N == 1:
        affected = sel[:, :, None].expand(scores.shape[:3])
    else:
        others = scores.clone()
        others[..., dom] = -math.inf
        affected = (scores[..., dom] - others.max(-1).values > SAT_MARGIN) & sel[:, :, None]
    pmax = probs.max(-1).values
    return {"affected_rows_exist": bool(affected.any()), "saturated": bool((pmax[affected] > 1 - 1e-6).all()),
            "plain_rows_remain": kind != "mixed" or N == 1 or bool((pmax[~sel] < 0.9).any())}


def _attention_inputs(kind, B, N, H, hd, q_view, k_view, seed):
    """Edits q_view / k_view ([B, rows, H, hd] views of the operand) in place; returns (dominant key, saturated pairs)."""
    every = [(b, h) for b in range(B) for h in range(H)]
    if kind in ("sat_first", "sat_last"):
        dom = 0 if kind == "sat_first" else N - 1
        k_view[:, dom] *= SAT_SCALE
        return dom, every
    if kind == "mixed":                          # half the (batch, head) pairs saturated, half plain, in one launch
        pairs = [(b, h) for b, h in every if (b * H + h) % 2 == 0]
        for b, h in pairs:
            k_view[b, 0, h] *= SAT_SCALE
        return 0, pairs
    off = 8.0 if hd == 16 else 5.0               # score ~ +-off^2 sqrt(hd): 200 at hd 64, 141 at hd 32, 256 at hd 16
    q_view.copy_(off + 0.01 * rnd(*q_view.shape, seed=seed + 1))
    k_view.copy_((off if kind == "offset_pos" else -off) + 0.01 * rnd(*k_view.shape, seed=seed + 2))
    return None, []


def _attention_prop(kind, ref, dom, pairs):
    if kind.startswith("offset"):
        return {"offset": float(ref["scores"].abs().min()) > 88.0}
    return _saturation_prop(kind, ref["scores"], ref["probs"], dom, pairs)


@functools.lru_cache(maxsize=None)
def attention_case(shape, kind):
    B, N, H, hd = shape
    E = H * hd
    qkv, dout = rnd(B, N, 3 * E, seed=1), rnd(B, N, E, seed=2)
    v5 = qkv.view(B, N, 3, H, hd)
    dom, pairs = _attention_inputs(kind, B, N, H, hd, v5[:, :, 0], v5[:, :, 1], seed=10)
    ref = attention_eval(qkv, dout, B, N, H, hd, torch.float64)
    y32 = attention_eval(qkv, dout, B, N, H, hd, torch.float32)
    metric = {"out": max_abs, "lse": max_abs, "probs": max_abs, "dqkv": rel_err}
    return make_case(f"attn-{'x'.join(map(str, shape))}-{kind}", {"qkv": qkv, "dout": dout}, ref, y32, metric,
                     _attention_prop(kind, ref, dom, pairs))


@functools.lru_cache(maxsize=None)
def q1_case(shape, kind):
    B, N, H, hd = shape
    E = H * hd
    g = torch.Generator().manual_seed(B * 1000 + N)
    q, kv, dout = torch.randn(B, E, generator=g), torch.randn(B * N, 2 * E, generator=g), torch.randn(B, E, generator=g)
    dom, pairs = _attention_inputs(kind, B, N, H, hd, q.view(B, 1, H, hd), kv.view(B, N, 2, H, hd)[:, :, 0], seed=20)
    ref = q1_eval(q, kv, dout, B, N, H, hd, torch.float64)
    y32 = q1_eval(q, kv, dout, B, N, H, hd, torch.float32)
    metric = {"out": max_abs, "lse": max_abs, "dq": rel_err, "dkv": rel_err}
    return make_case(f"q1-{'x'.join(map(str, shape))}-{kind}", {"q": q, "kv": kv, "dout": dout}, ref, y32, metric,
                     _attention_prop(kind, ref, dom, pairs))


# ------------------------------------------------------------------------------------------------------------ LayerNorm
# rows x cols: the 16-byte kernels (192, 96, 16, 4), MAXV = 16 (768) and the row counts of the fused dX GEMM
LN_SHAPES = [(70, 192), (70, 96), (37, 16), (20, 4), (9, 768), (2048, 192), (4096, 96)]
LN_KINDS = ["offset", "constant", "outlier", "tiny", "mixed"]
LN_EPS = 1e-6
LN_CONST = 3.25
LN_FUSED_ROWS = [r for r in R.PLAN_ROWS if r.row in ("ln.192", "ln.96")]


def _ln_rows(kind, x, seed):
    """x [rows, cols] ~ N(0.5, 2) turned into the rows of one kind; returns the mask of the constant rows."""
    rows, cols = x.shape
    const = torch.zeros(rows, dtype=torch.bool)
    ar = torch.arange(rows)
    which = {"offset": ar < 0, "constant": ar < 0, "outlier": ar < 0, "tiny": ar < 0}
    if kind == "mixed":                          # all four kinds interleaved in one launch
        for j, k in enumerate(("offset", "constant", "outlier", "tiny")):
            which[k] = ar % 4 == j
    elif kind == "constant":
        which["constant"] = ar % 3 == 0          # every third row
    else:
        which[kind] = ar >= 0
    x[which["offset"]] += 1000.0
    x[which["constant"]] = LN_CONST
    col = seed % cols
    x[which["outlier"], col] = 1e4
    x[which["tiny"]] *= 1e-4
    return which["constant"], which["tiny"]


def layernorm_eval(x, gamma, beta, dy, resid, dtype, one_pass=False):
    """LayerNorm forward and backward.  one_pass=True: the variance as E[x^2] - E[x]^2."""
    xl, gl, bl = (t.to(dtype).clone().requires_grad_(True) for t in (x, gamma, beta))
    mean = xl.mean(1, keepdim=True)
    if one_pass:
        var = (xl * xl).mean(1, keepdim=True) - mean * mean
        y = (xl - mean) * torch.rsqrt(var + LN_EPS) * gl + bl
    else:
        var = xl.var(1, unbiased=False, keepdim=True)
        y = F.layer_norm(xl, (x.shape[1],), gl, bl, LN_EPS)
    y.backward(dy.to(dtype))
    return {"y": y.detach(), "mean": mean.detach().squeeze(1), "var": var.detach().squeeze(1), "dx": xl.grad,
            "dx_resid": xl.grad + resid.to(dtype), "dgamma": gl.grad, "dbeta": bl.grad}


def _ln_prop(kind, ref, const, tiny):
    p = {}
    if kind in ("constant", "mixed"):
        p["constant_rows_have_zero_variance"] = bool(const.any()) and bool((ref["var"][const] == 0).all())
    if kind in ("tiny", "mixed"):
        p["tiny_rows_below_eps"] = bool(tiny.any()) and bool((ref["var"][tiny] < LN_EPS).all())
    if kind in ("offset", "mixed"):
        p["offset_rows_have_mean_1000"] = bool((ref["mean"] > 990).any())
    if kind in ("outlier", "mixed"):
        p["outlier_dominates"] = bool((ref["var"] > 1e5).any())
    return p


@functools.lru_cache(maxsize=None)
def layernorm_case(shape, kind):
    rows, cols = shape
    x = rnd(rows, cols, seed=1) * 2 + 0.5
    const, tiny = _ln_rows(kind, x, seed=7)
    gamma, beta = 1 + 0.1 * rnd(cols, seed=2), 0.1 * rnd(cols, seed=3)
    dy, resid = rnd(rows, cols, seed=4), rnd(rows, cols, seed=5)
    ref = layernorm_eval(x, gamma, beta, dy, resid, torch.float64)
    y32 = layernorm_eval(x, gamma, beta, dy, resid, torch.float32)
    metric = {"y": max_abs, "dx": rel_err, "dx_resid": rel_err, "dgamma": rel_err, "dbeta": rel_err}
    c = make_case(f"ln-{rows}x{cols}-{kind}", {"x": x, "gamma": gamma, "beta": beta, "dy": dy, "resid": resid}, ref, y32, metric,
                  _ln_prop(kind, ref, const, tiny))
    c.const = const
    return c


def ln_fused_eval(dy, Wt, x, gamma, dtype):
    """LayerNorm backward of dA = dY Wt^T (the Linear's input gradient): dx, dgamma, dbeta."""
    xl, gl = x.to(dtype).clone().requires_grad_(True), gamma.to(dtype).clone().requires_grad_(True)
    y = F.layer_norm(xl, (x.shape[1],), gl, None, LN_EPS)
    da = dy.to(dtype) @ Wt.to(dtype).T
    y.backward(da)
    return {"dx": xl.grad, "dgamma": gl.grad, "dbeta": da.sum(0), "var": xl.detach().var(1, unbiased=False),
            "mean": xl.detach().mean(1)}


@functools.lru_cache(maxsize=None)
def ln_fused_case(i, kind):
    M, N, K = LN_FUSED_ROWS[i].shape
    x = rnd(M, K, seed=3) * 2 + 0.5
    const, tiny = _ln_rows(kind, x, seed=7)
    dy, Wt, gamma = rnd(M, N, seed=1), rnd(K, N, seed=2, scale=0.05), 1 + 0.1 * rnd(K, seed=4)
    ref = ln_fused_eval(dy, Wt, x, gamma, torch.float64)
    y32 = ln_fused_eval(dy, Wt, x, gamma, torch.float32)
    metric = {"dx": rel_err, "dgamma": rel_err, "dbeta": rel_err}
    return make_case(f"lnfused-{M}x{N}x{K}-{kind}", {"x": x, "dy": dy, "Wt": Wt, "gamma": gamma}, ref, y32, metric,
                     _ln_prop(kind, ref, const, tiny))


# ------------------------------------------------------------------------------------------------------------ GELU epilogue
def gelu_sweep():
    """4096 points evenly spaced on [-12, 12], +-0, +-40, +-1e4."""
    return torch.cat([torch.linspace(-12.0, 12.0, 4096), torch.tensor([0.0, -0.0, 40.0, -40.0, 1e4, -1e4])])


def gelu_eval(pre, dtype):
    p = pre.to(dtype).clone().requires_grad_(True)
    act = F.gelu(p)
    act.sum().backward()
    return {"act": act.detach(), "grad": p.grad}


def act_err(a, ref):
    """test_ops_gpu.test_linear_gelu_fwd's metric of the activation: |a - ref| / (1 + |ref|), maximum."""
    a, ref = torch.as_tensor(a).double(), torch.as_tensor(ref).double()
    return float(((a - ref).abs() / (1 + ref.abs())).max())


@functools.lru_cache(maxsize=None)
def gelu_case(M, N, K):
    """The sweep cut into [M, K] operands x (the last one padded with zeros): with W[n] = e_(n % K) and b = 0 the
    pre-activation of column n is x[:, n % K], exactly, in every GEMM engine (one non-zero product per output)."""
    sweep = gelu_sweep()
    per = M * K
    nchunk = -(-sweep.numel() // per)
    xs = torch.zeros(nchunk * per)
    xs[:sweep.numel()] = sweep
    xs = xs.view(nchunk, M, K)
    W = torch.zeros(N, K)
    W[torch.arange(N), torch.arange(N) % K] = 1.0
    pre = xs[:, :, torch.arange(N) % K]                                  # [nchunk, M, N], exact
    ref, y32 = gelu_eval(pre, torch.float64), gelu_eval(pre, torch.float32)
    # the input-gradient GEMMs with the GELU derivative as their epilogue factor: dx = (dy W) * gelu'(x)
    dy = rnd(nchunk, M, N, seed=1)
    gg32 = gelu_eval(xs, torch.float32)["grad"]
    for d, dt in ((ref, torch.float64), (y32, torch.float32)):
        d["dx"] = (dy.to(dt) @ W.to(dt)) * gg32.to(dt)
    metric = {"act": act_err, "grad": max_abs, "dx": rel_err}
    prop = {"sweep_is_exact": bool((pre.double() == xs.double()[:, :, torch.arange(N) % K]).all()),
            "sweep_complete": sweep.numel() == 4102 and float(sweep[:4096].min()) == -12.0 and float(sweep[:4096].max()) == 12.0,
            "far_left_is_zero": bool((ref["act"][pre <= -40] == 0).all() and (ref["grad"][pre <= -40] == 0).all()),
            "far_right_is_identity": bool((ref["act"][pre >= 40] == pre.double()[pre >= 40]).all() and (ref["grad"][pre >= 40] == 1).all())}
    return make_case(f"gelu-{M}x{N}x{K}", {"x": xs, "W": W, "pre": pre, "dy": dy, "gg": gg32}, ref, y32, metric, prop)


# ------------------------------------------------------------------------------------------------------------ cross entropy, L1
CE_CLASSES = [1, 10, 64, 65, 1000]
CE_SMOOTHING = [0.0, 0.1]
CE_KINDS = ["equal", "one_huge", "spread", "label_last"]
CE_ROWS = 9                                      # three blocks of four waves, the last one ragged


def ce_eval(z, y, smoothing, dtype):
    zl = z.to(dtype).clone().requires_grad_(True)
    loss = F.cross_entropy(zl, y, label_smoothing=smoothing, reduction="sum")
    loss.backward()
    return {"loss": loss.detach().reshape(1), "dlogits": zl.grad}


@functools.lru_cache(maxsize=None)
def ce_case(C, smoothing, kind):
    g = torch.Generator().manual_seed(C)
    y = torch.randint(0, C, (CE_ROWS,), generator=g)
    if kind == "equal":
        z = torch.full((CE_ROWS, C), 2.5)
    elif kind == "one_huge":
        z = rnd(CE_ROWS, C, seed=3)
        z[torch.arange(CE_ROWS), torch.arange(CE_ROWS) % C] = 1e4
    elif kind == "spread":
        z = (torch.rand(CE_ROWS, C, generator=g) * 2 - 1) * 80
        z[:, 0], z[:, -1] = 80.0, -80.0
    else:
        z = rnd(CE_ROWS, C, seed=3) * 3
        y = torch.full((CE_ROWS,), C - 1)
    ref, y32 = ce_eval(z, y, smoothing, torch.float64), ce_eval(z, y, smoothing, torch.float32)
    prop = {"equal": kind != "equal" or bool((z == z[:, :1]).all()),
            "one_huge": kind != "one_huge" or float(z.max()) == 1e4,
            "spread": kind != "spread" or C == 1 or float(z.max() - z.min()) == 160.0,
            "label_last": kind != "label_last" or bool((y == C - 1).all())}
    return make_case(f"ce-C{C}-s{smoothing}-{kind}", {"z": z, "y": y}, ref, y32, {"loss": rel_err, "dlogits": max_abs}, prop)


L1_SIZES = [7, 128 * 784 + 3]
L1_UNPATCHIFY_SHAPES = [(4, 1, 28, 2), (3, 3, 8, 4)]         # (B, C, S, p)


@functools.lru_cache(maxsize=None)
def l1_case(n):
    """pred == target bitwise on every second element: the gradient there is exactly 0."""
    p, t = rnd(n, seed=1), rnd(n, seed=2)
    tie = torch.arange(n) % 2 == 0
    p[tie] = t[tie]
    ref = {"loss": (p.double() - t.double()).abs().sum().reshape(1), "sign": torch.sign(p - t).double()}
    y32 = {"loss": (p - t).abs().sum().reshape(1), "sign": torch.sign(p - t)}
    return make_case(f"l1-{n}", {"pred": p, "target": t, "tie": tie}, ref, y32, {"loss": rel_err},
                     {"ties_are_bitwise": bool((p[tie] == t[tie]).all()), "half_are_ties": int(tie.sum()) == (n + 1) // 2})


@functools.lru_cache(maxsize=None)
def l1_unpatchify_case(shape):
    B, C, S, p = shape
    n = (S // p) ** 2
    pred, img = rnd(B, n + 1, p * p * C, seed=1), rnd(B, C, S, S, seed=2)
    recon = O.unpatchify(pred[:, 1:, :], p)
    tie = (torch.arange(img.numel()) % 2 == 0).view(img.shape)
    img[tie] = recon[tie]
    out = {}
    for key, dt in (("ref", torch.float64), ("y32", torch.float32)):
        pl = pred.to(dt).clone().requires_grad_(True)
        loss = (O.unpatchify(pl[:, 1:, :], p) - img.to(dt)).abs().sum()
        loss.backward()
        out[key] = {"loss": loss.detach().reshape(1), "sign": pl.grad}
    zero = out["ref"]["sign"] == 0
    return make_case(f"l1unp-{'x'.join(map(str, shape))}", {"pred": pred, "img": img, "recon": recon, "zero": zero}, out["ref"],
                     out["y32"], {"loss": rel_err},
                     {"ties_are_bitwise": bool((img[tie] == recon[tie]).all()),
                      "half_and_cls_are_zero": int(zero.sum()) == int(tie.sum()) + B * p * p * C})


# ------------------------------------------------------------------------------------------------------------ SOM
# (B, K, L, map, topology)
SOM_SHAPES = [(33, 12, 48, (4, 3), "hexa"), (70, 256, 48, (16, 16), "square"), (64, 100, 3136, (10, 10), "square")]
SOM_T = [0.05, 1e4]                              # a one-hot neighbourhood (near Tmin) and a flat one
SOM_GAMMA = 0.37
NORM_EPS = 1e-12                                 # F.normalize


def cosine_dist(x, W, clamp=True):
    """1 - <x / max(|x|, eps), w / max(|w|, eps)>.  clamp=False: the norms without the eps clamp."""
    if clamp:
        return O.som_distances(x, W)
    return 1 - (x / x.norm(dim=1, keepdim=True)) @ (W / W.norm(dim=1, keepdim=True)).T


def som_eval(x, W, grid, T, fcn, dtype, bmu=None, clamp=True, matmul_form=False):
    """Distances, BMU, neighbourhood, loss = mean(h d) and the gradients of SOM_GAMMA * loss.  `bmu`: the indices the
    neighbourhood is built from (the fp64 argmin, so that the fp32 evaluation answers the same question).
    matmul_form: the euclidean distance as torch.cdist's |x|^2 + |w|^2 - 2 x.w, the form bmu_finalize_kernel restates."""
    xl, Wl = x.to(dtype).clone().requires_grad_(True), W.to(dtype).clone().requires_grad_(True)
    if fcn == "cosine":
        d = cosine_dist(xl, Wl, clamp)
    elif fcn == "euclidean":
        d = torch.cdist(xl, Wl, p=2, compute_mode="use_mm_for_euclid_dist" if matmul_form else "donot_use_mm_for_euclid_dist")
    else:
        d = torch.cdist(xl, Wl, p=1)
    own = d.detach().argmin(1)
    h = O.neighbourhood(own if bmu is None else bmu, grid.to(dtype), T)
    loss = O.som_loss(h, d)
    (SOM_GAMMA * loss).backward()
    return {"dist": d.detach(), "bmu": own, "h": h, "loss": loss.detach().reshape(1), "gW": Wl.grad, "gX": xl.grad}


def manhattan_grads(x, W, h, sign0=0.0):
    """The Manhattan gradients written out, d|x - w| / dx = sign(x - w) with sign(0) = sign0 (0 is torch's)."""
    B, K = h.shape
    c = SOM_GAMMA / (B * K) * h.double()
    sg = torch.sign(x.double()[:, None, :] - W.double()[None, :, :])
    sg[sg == 0] = sign0
    return {"gX": torch.einsum("bk,bkl->bl", c, sg), "gW": -torch.einsum("bk,bkl->kl", c, sg)}


def _som_operands(shape, kind):
    B, K, L = shape[:3]
    x = rnd(B, L, seed=1)
    W = torch.rand(K, L, generator=torch.Generator().manual_seed(2))
    if kind == "cos_zero":                       # one all-zero sample row, one all-zero prototype
        W = F.normalize(W, dim=1)
        x[2] = 0.0
        W[1] = 0.0
    elif kind == "cos_scaled":                   # rows scaled by 1e-5 and by 1e15: the norm stays above eps, the sum of
        W = F.normalize(W, dim=1)                # squares inside fp32
        x[1::3] *= 1e-5
        x[2::3] *= 1e15
    elif kind == "cos_identical":                # every prototype the same vector
        W = F.normalize(W[:1], dim=1).expand(K, L).contiguous()
    elif kind == "euclid_coincident":            # a prototype that IS a sample, and two identical prototypes
        W[3] = x[7]
        W[5] = W[4]
    elif kind == "manhattan_grid":               # multiples of 0.5: many x_j == w_j exactly, every sum exact in fp32
        x = torch.round(x * 2) / 2
        W = torch.round(W * 4 - 1) / 2
    return x, W


SOM_KINDS = {"cos_zero": "cosine", "cos_scaled": "cosine", "cos_identical": "cosine", "euclid_coincident": "euclidean",
             "manhattan_grid": "manhattan"}


@functools.lru_cache(maxsize=None)
def som_case(i, kind, T):
    shape = SOM_SHAPES[i]
    B, K, L, map_size, topo = shape
    fcn = SOM_KINDS[kind]
    x, W = _som_operands(shape, kind)
    grid = O.grid_positions(map_size, topo)
    ref = som_eval(x, W, grid, T, fcn, torch.float64)
    y32 = som_eval(x, W, grid, T, fcn, torch.float32, bmu=ref["bmu"], matmul_form=True)
    metric = {"dist": rel_err if fcn != "cosine" else max_abs, "h": max_abs, "loss": rel_err if fcn != "cosine" else max_abs,
              "gW": rel_err, "gX": rel_err}
    h32 = O.neighbourhood(ref["bmu"], grid, T)
    onehot = F.one_hot(ref["bmu"], K).float()
    srt = ref["dist"].sort(1).values
    prop = {}
    if T < 1:
        prop["dead_neighbourhood"] = bool(torch.equal(h32, onehot))
        prop["loss_is_mean_bmu_distance"] = abs(float(ref["loss"]) - float(srt[:, 0].sum()) / (B * K)) <= 1e-12 * max(1.0, float(srt[:, 0].sum()))
    else:
        prop["flat_neighbourhood"] = float(ref["h"].min()) > 1 - 1e-5
    if kind == "cos_zero":
        prop["zero_row_and_prototype_at_distance_1"] = bool((ref["dist"][2] == 1).all() and (ref["dist"][:, 1] == 1).all())
        prop["zero_row_bmu_is_0"] = int(ref["bmu"][2]) == 0
    if kind == "cos_scaled":
        plain = som_eval(rnd(B, L, seed=1), W, grid, T, fcn, torch.float64)
        ss = (x.double() ** 2).sum(1)
        prop["norms_inside_fp32"] = float(ss.min().sqrt()) > NORM_EPS and float(ss.max()) < 3e38 and float(ss.min()) > 1.2e-38
        prop["bmus_are_those_of_the_unscaled_rows"] = bool(torch.equal(plain["bmu"], ref["bmu"]))
        prop["no_near_ties"] = float((srt[:, 1] - srt[:, 0]).min()) > 2e-6
    if kind == "cos_identical":
        prop["every_bmu_is_0"] = bool((ref["bmu"] == 0).all())
    if kind == "euclid_coincident":
        prop["coincident"] = float(ref["dist"][7, 3]) == 0.0 and bool((ref["dist"][:, 4] == ref["dist"][:, 5]).all())
    if kind == "manhattan_grid":
        prop["many_exact_zeros"] = float((x[:, None, :8] == W[None, :, :8]).float().mean()) > 0.05
        prop["sums_exact_in_fp32"] = bool(torch.equal(y32["dist"].double(), ref["dist"]))
    c = make_case(f"som-{B}x{K}x{L}-{kind}-T{T:g}", {"x": x, "W": W, "grid": grid}, ref, y32, metric, prop)
    c.fcn, c.T, c.shape, c.onehot = fcn, T, shape, onehot
    return c


# ------------------------------------------------------------------------------------------------------------ AdamW
ADAMW_STEPS = [1, 1000]
ADAMW_HP = dict(lr=3e-3, b1=0.9, b2=0.999, eps=1e-8)
ADAMW_WD = [0.05, 0.0, 0.01, 0.05]


def adamw_eval(p, g, m, v, wd, step, dtype):
    outs = [O.adamw_reference(p[i].to(dtype), g[i].to(dtype), m[i].to(dtype), v[i].to(dtype), step, ADAMW_HP["lr"],
                              ADAMW_HP["b1"], ADAMW_HP["b2"], ADAMW_HP["eps"], wd[i]) for i in range(len(wd))]
    return {k: torch.stack([o[j] for o in outs]) for j, k in enumerate(("p", "m", "v"))}


@functools.lru_cache(maxsize=None)
def adamw_case(step):
    """One arena of 4 x 256 elements; the gradient chunks: 0 (with v = 0), 1e-20, 1e15, alternating +-1."""
    p = rnd(4, 256, seed=1)
    g = torch.zeros(4, 256)
    g[1], g[2] = 1e-20, 1e15
    g[3] = torch.where(torch.arange(256) % 2 == 0, 1.0, -1.0)
    if step == 1:
        m, v = torch.zeros(4, 256), torch.zeros(4, 256)
    else:                                        # moments as a long run on this gradient leaves them (chunk 0: still 0)
        m, v = 0.9 * g, 0.6 * g * g
    ref, y32 = adamw_eval(p, g, m, v, ADAMW_WD, step, torch.float64), adamw_eval(p, g, m, v, ADAMW_WD, step, torch.float32)
    prop = {"chunk0_is_all_zero": bool((g[0] == 0).all() and (v[0] == 0).all() and (m[0] == 0).all()),
            "chunks": float(g[1, 0]) == float(torch.tensor(1e-20)) and float(g[2, 0]) == float(torch.tensor(1e15)),
            "zero_gradient_only_decays": bool(torch.equal(ref["p"][0], p[0].double() * (1 - ADAMW_HP["lr"] * ADAMW_WD[0])))}
    return make_case(f"adamw-step{step}", {"p": p, "g": g, "m": m, "v": v}, ref, y32, {"p": max_abs}, prop)
