"""The kernels at the numerical edges of their inputs (tests/numeric_edges.py): every case runs through its
vit_som_amd.ops wrapper into NaN-filled outputs and is compared with the fp64 reference.  A kernel's error e_k passes
when e_k <= max(FLOOR, 4 e32), e32 being plain fp32 torch's error on the same inputs in the same metric; FLOOR is the
tolerance of the entry point's own test in test_ops_gpu.py / test_classifier_gpu.py (quoted at each use).  Index outputs
are exact, and where the reference is 0 or a copy the result must be too.  References are computed once per case
(lru_cache) and shared by the GEMM modes and hooks.  Every comparison prints
    EDGE|case|variant|output|e32|e_k|e_k / e32|bound
(pytest -s), the source of profiles/r11_numeric_edges.txt.

Cases with a bound of their own (reason and measured ratios: profiles/r11_numeric_edges.txt): see OWN_BOUND."""
import math

import numpy as np
import pytest
import torch

import launch_plan_rows as R
import numeric_edges as NE
from test_launch_plan_cpu import describe
from test_ops_gpu import GEMM_TOL, GRAD3_TOL, bmu_policy_ok

pytestmark = pytest.mark.gpu

DEV = "cuda"
MODE_IDS = ["f32", "split_bf16", "grad3"]



def score_ulps(c, n=2):
    """n fp32 ulps of the largest |score| of an attention case."""
    return n * float(np.spacing(np.float32(c.ref["scores"].abs().max())))


# Cases with a bound of their own, (case name, output): 2 fp32 ulp of the largest |score| of the case, in the forms that
# compute P = exp(s - lse) (every form but attn_shared_bf16x3, which normalises by its own scores and keeps the issue's
# bound).  Those kernels recompute s in another accumulation order than the forward that produced lse: s differs by an
# ulp or two of |s|, and P, hence everything linear in it, by that much relatively (fp32 torch shifts by the maximum of
# the same s and pays nothing).  Where nothing dilutes it the error shows whole:
#  - a single token whose score is large (sat_first, sat_last; |s| = 68): P = 1, dV = P dO, the reference's dQ and dK are
#    0 and e32 = 0; measured 6.3e-6 against the floor of 5e-6, bound 1.5e-5.  (offset_*, mixed: inside 5e-6, no own bound.)
#  - the single-query case: dq on its saturated rows is the cancellation p (dP - D) times the 40-fold key, and the
#    yardstick happens to hit 2.6e-6 there (4.7e-5 on the same input at (8, 197, 3, 64)); ratio 5.2, bound 1.5e-5.
# Measured ratios: profiles/r11_numeric_edges.txt.
OWN_BOUND = {("attn-2x1x2x64-sat_first", "dqkv"), ("attn-2x1x2x64-sat_last", "dqkv"), ("q1-16x65x3x64-sat_last", "dq")}


@pytest.fixture(scope="module")
def ops():
    from vit_som_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def lib():
    from vit_som_amd._lib import lib as _lib
    return _lib


def dev(t):
    return t.to(DEV)


def new(*s):
    return torch.full(s, float("nan"), device=DEV)


def name(v):
    return "-".join(str(e) for e in v) if isinstance(v, tuple) else str(v)


class Checks:
    """Measures every output, prints the figures, and fails at the end with the list of those out of bound."""

    def __init__(self, case):
        self.c, self.bad = case, []

    def err(self, variant, out, got, floor, ref=None, e32=None):
        c = self.c
        e32 = c.e32[out] if e32 is None else e32
        e_k = c.metric[out.split(".")[0]](got.detach().cpu(), c.ref[out] if ref is None else ref)
        lim = NE.bound(floor, e32)
        if (c.name, out) in OWN_BOUND and "bf16x3" not in variant:
            lim = max(lim, score_ulps(c))
        print(f"EDGE|{c.name}|{variant}|{out}|{e32:.3e}|{e_k:.3e}|{e_k / e32 if e32 else math.inf:.2f}|{lim:.3e}")
        if not e_k <= lim:
            self.bad.append((variant, out, e_k, lim))

    def true(self, variant, what, ok):
        if not ok:
            self.bad.append((variant, what))

    def done(self):
        assert not self.bad, (self.c.name, self.bad)


# ------------------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("mode", R.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape,kind", NE.attention_ids(), ids=name)
def test_attention_edges(ops, lib, shape, kind, mode):
    """attention_fwd / attention_probs (3e-6 absolute, test_attention) and attention_bwd under every hook (5e-6 relative;
    GRAD3_TOL where the plan runs the two-piece split)."""
    c = NE.attention_case(shape, kind)
    B, N, H, hd = shape
    E = H * hd
    k = Checks(c)
    prev = ops.get_gemm_mode()
    ops.set_gemm_mode(mode)
    try:
        qkv, dout = dev(c.inp["qkv"]), dev(c.inp["dout"])
        out, lse, probs = new(B, N, E), new(B, H, N), new(B, H, N, N)
        ops.attention_fwd(qkv, out, lse, B, N, H, hd)
        ops.attention_probs(qkv, lse, probs, B, N, H, hd)
        for o, got in (("out", out), ("lse", lse), ("probs", probs)):
            k.err(MODE_IDS[mode], o, got, 3e-6)
        for hook in R.HOOK_VALUES["attention_fused"]:
            ops.set_attention_fused(hook)
            plan = describe(lib, R.ATTENTION_BWD, (N, H, hd), 1)
            if plan[2] == 2:                        # the two-piece split: test_attention_bwd_two_piece_split_edges
                continue
            dqkv, delta = new(B, N, 3 * E), new(B, H, N)
            ops.attention_bwd(qkv, out, dout, lse, dqkv, delta, B, N, H, hd)
            k.err(f"{MODE_IDS[mode]}.hook{hook}.{plan[0]}", "dqkv", dqkv, 5e-6)
            k.true(f"hook{hook}", "delta finite", bool(torch.isfinite(delta).all()))
        torch.cuda.synchronize()
    finally:
        ops.set_gemm_mode(prev)
        ops.set_attention_fused(R.HOOK_DEFAULTS["attention_fused"])
    k.done()


SPLIT_SHAPES = [s for s in NE.ATTN_SHAPES if s[3] == 64 and s[1] <= 65]


@pytest.mark.parametrize("shape,kind", NE.attention_ids(SPLIT_SHAPES), ids=name)
def test_attention_bwd_two_piece_split_edges(ops, lib, shape, kind):
    """attention_bwd in the form the default mode runs at hd = 64, N <= 65 (attn_shared_bf16x3: dP and the accumulations
    on the two-piece bf16 split, the scores on three pieces, P normalised by the kernel's own scores), bound
    max(GRAD3_TOL, 4 e32).  With two-piece scores against the forward's lse this missed by up to 2.6e-3 on saturated rows
    (profiles/r11_numeric_edges.txt)."""
    c = NE.attention_case(shape, kind)
    B, N, H, hd = shape
    E = H * hd
    k = Checks(c)
    prev = ops.get_gemm_mode()
    ops.set_gemm_mode(R.GRAD3)
    try:
        ops.set_attention_fused(1)
        plan = describe(lib, R.ATTENTION_BWD, (N, H, hd), 1)
        assert plan[0] == "attn_shared_bf16x3" and plan[2] == 2
        qkv, dout = dev(c.inp["qkv"]), dev(c.inp["dout"])
        out, lse = new(B, N, E), new(B, H, N)
        ops.attention_fwd(qkv, out, lse, B, N, H, hd)
        dqkv, delta = new(B, N, 3 * E), new(B, H, N)
        ops.attention_bwd(qkv, out, dout, lse, dqkv, delta, B, N, H, hd)
        k.err("grad3.hook1.attn_shared_bf16x3", "dqkv", dqkv, GRAD3_TOL)
        torch.cuda.synchronize()
    finally:
        ops.set_gemm_mode(prev)
        ops.set_attention_fused(R.HOOK_DEFAULTS["attention_fused"])
    k.done()


@pytest.mark.parametrize("shape,kind", NE.attention_ids(NE.Q1_SHAPES), ids=name)
def test_attention_q1_edges(ops, shape, kind):
    """attention_q1_fwd / attention_q1_bwd: 1e-5 (test_attention_q1_against_fp64's bound)."""
    c = NE.q1_case(shape, kind)
    B, N, H, hd = shape
    E = H * hd
    k = Checks(c)
    q, kv, dout = dev(c.inp["q"]), dev(c.inp["kv"]), dev(c.inp["dout"])
    o, lse, dq, dkv = new(B, E), new(B, H), new(B, E), new(B * N, 2 * E)
    ops.attention_q1_fwd(q, kv, o, lse, B, N, H, hd)
    ops.attention_q1_bwd(dout, o, lse, q, kv, dq, dkv, B, N, H, hd)
    for out, got in (("out", o), ("lse", lse), ("dq", dq), ("dkv", dkv)):
        k.err("q1", out, got, 1e-5)
    k.done()


# ------------------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("shape,kind", [(s, kd) for s in NE.LN_SHAPES for kd in NE.LN_KINDS], ids=name)
def test_layernorm_edges(ops, shape, kind):
    """layernorm_fwd (3e-6 absolute), layernorm_bwd with and without the residual, and the deferred pair where the shape
    allows it (5e-6 relative: test_layernorm).  On a constant row y is beta and the mean the constant, bit for bit."""
    c = NE.layernorm_case(shape, kind)
    rows, cols = shape
    k = Checks(c)
    x, gamma, beta, dy, resid = (dev(c.inp[n]) for n in ("x", "gamma", "beta", "dy", "resid"))
    y, mean, rstd = new(rows, cols), new(rows), new(rows)
    ops.layernorm_fwd(x, gamma, beta, y, mean, rstd, NE.LN_EPS)
    k.err("fwd", "y", y, 3e-6)
    const = c.const
    if bool(const.any()):
        k.true("fwd", "y == beta on constant rows", torch.equal(y.cpu()[const], c.inp["beta"].expand(int(const.sum()), cols)))
        k.true("fwd", "mean == the constant", bool((mean.cpu()[const] == NE.LN_CONST).all()))
    k.true("fwd", "rstd finite", bool(torch.isfinite(rstd).all()))

    def bwd(variant, call, with_resid):
        dx, dg, db = new(rows, cols), new(cols), new(cols)
        call(dy, x, mean, rstd, gamma, resid if with_resid else None, dx, dg, db)
        k.err(variant, "dx_resid" if with_resid else "dx", dx, 5e-6)
        k.err(variant, "dgamma", dg, 5e-6)
        k.err(variant, "dbeta", db, 5e-6)

    bwd("bwd.resid", ops.layernorm_bwd, True)
    bwd("bwd", ops.layernorm_bwd, False)
    if ops.layernorm_bwd_deferrable(rows, cols):
        jobs = ops.LayerNormJobs(DEV)

        def deferred(*a):
            jobs.begin()
            jobs.bwd(*a)
            jobs.flush()

        bwd("deferred.resid", deferred, True)
    k.done()


@pytest.mark.parametrize("mode", [R.SPLIT, R.GRAD3], ids=MODE_IDS[1:])
@pytest.mark.parametrize("i,kind", [(i, kd) for i in range(len(NE.LN_FUSED_ROWS)) for kd in NE.LN_KINDS], ids=name)
def test_ln_fused_edges(ops, lib, i, kind, mode):
    """linear_bwd_input_ln at the rows ln.192 / ln.96 of the launch plan, both tile shapes, both split modes: the bounds
    of test_plan_row_against_fp64 (GEMM_TOL; GRAD3_TOL where the plan runs two planes)."""
    c = NE.ln_fused_case(i, kind)
    row = NE.LN_FUSED_ROWS[i]
    M, N, K = row.shape
    k = Checks(c)
    prev = ops.get_gemm_mode()
    ops.set_gemm_mode(mode)
    try:
        x, dy, Wt, gamma = (dev(c.inp[n]) for n in ("x", "dy", "Wt", "gamma"))
        y, mean, rstd = new(M, K), new(M), new(M)
        ops.layernorm_fwd(x, gamma, torch.zeros(K, device=DEV), y, mean, rstd, NE.LN_EPS)
        for tiles in R.HOOK_VALUES["ln_tiles"]:
            ops.set_ln_tiles(tiles)
            plan = describe(lib, row.op, row.shape, 1)
            assert plan is not None and ops.linear_bwd_input_ln_supported(M, N, K)
            tol = GRAD3_TOL if plan[2] == 2 else GEMM_TOL
            dx, dg, db = new(M, K), new(K), new(K)
            ops.linear_bwd_input_ln(dy, Wt, x, mean, rstd, gamma, None, dx, dg, db)
            for out, got in (("dx", dx), ("dgamma", dg), ("dbeta", db)):
                k.err(f"{MODE_IDS[mode]}.tiles{tiles}.{plan[1]}", out, got, tol)
        torch.cuda.synchronize()
    finally:
        ops.set_gemm_mode(prev)
        ops.set_ln_tiles(R.HOOK_DEFAULTS["ln_tiles"])
    k.done()


# ------------------------------------------------------------------------------------------------------------ GELU epilogue
@pytest.mark.parametrize("mode", R.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", [(70, 64, 4), (64, 16, 8)], ids=name)               # the second: the nt.m<=64 row
def test_gelu_edges(ops, shape, mode):
    """linear_gelu_fwd on exact pre-activations (the bounds of test_linear_gelu_fwd: 5e-6 on |act - ref| / (1 + |ref|)
    and on the derivative), and the input-gradient GEMMs with the derivative as their epilogue factor (GEMM_TOL;
    GRAD3_TOL for linear_bwd_input_t in the default mode, as test_linear_bwd_input_t)."""
    M, N, K = shape
    c = NE.gelu_case(M, N, K)
    k = Checks(c)
    prev = ops.get_gemm_mode()
    ops.set_gemm_mode(mode)
    try:
        xs, W, pre = dev(c.inp["x"]), dev(c.inp["W"]), c.inp["pre"]
        nchunk = xs.shape[0]
        bias = torch.zeros(N, device=DEV)
        grad, act = new(nchunk, M, N), new(nchunk, M, N)
        for j in range(nchunk):
            ops.linear_gelu_fwd(xs[j], W, bias, grad[j], act[j])
        k.err(MODE_IDS[mode], "act", act, 5e-6)
        k.err(MODE_IDS[mode], "grad", grad, 5e-6)
        act, grad = act.cpu(), grad.cpu()
        left, right = pre <= -40, pre >= 40
        k.true("fwd", "act == 0 at x <= -40", bool((act[left] == 0).all()))
        k.true("fwd", "grad == 0 at x <= -40", bool((grad[left] == 0).all()))
        k.true("fwd", "act == x at x >= 40", torch.equal(act[right], pre[right]))
        k.true("fwd", "grad == 1 at x >= 40", bool((grad[right] == 1).all()))
        if shape == (70, 64, 4):
            dy, gg = dev(c.inp["dy"]), dev(c.inp["gg"])
            Wt = W.T.contiguous()
            dx, dxt = new(nchunk, M, K), new(nchunk, M, K)
            for j in range(nchunk):
                ops.linear_bwd_input(dy[j], W, dx[j], gelu_grad=gg[j])
                ops.linear_bwd_input_t(dy[j], Wt, dxt[j], gelu_grad=gg[j])
            k.err(MODE_IDS[mode] + ".bwd_input", "dx", dx, GEMM_TOL)
            k.err(MODE_IDS[mode] + ".bwd_input_t", "dx", dxt, GRAD3_TOL if mode == R.GRAD3 else GEMM_TOL)
            dead = c.inp["gg"] == 0
            k.true("bwd", "dx == 0 where gelu' == 0", bool((dx.cpu()[dead] == 0).all() and (dxt.cpu()[dead] == 0).all()))
        torch.cuda.synchronize()
    finally:
        ops.set_gemm_mode(prev)
    k.done()


# ------------------------------------------------------------------------------------------------------------ cross entropy, L1
@pytest.mark.parametrize("C,smoothing,kind", [(C, s, kd) for C in NE.CE_CLASSES for s in NE.CE_SMOOTHING for kd in NE.CE_KINDS],
                         ids=name)
def test_cross_entropy_edges(ops, C, smoothing, kind):
    """cross_entropy_ls: the summed loss relative (2e-6: test_cross_entropy_ls's bound on losses of order 1; a loss that
    is exactly 0 -- one class -- must come out 0), dlogits absolute at grad_scale = 1 (5e-6, its bound on entries <= 1)."""
    c = NE.ce_case(C, smoothing, kind)
    k = Checks(c)
    loss, dz = torch.zeros(1, device=DEV), new(NE.CE_ROWS, C)
    ops.cross_entropy_ls(dev(c.inp["z"]), dev(c.inp["y"]), smoothing, loss, dlogits=dz, grad_scale=1.0)
    k.err("ce", "loss", loss, 2e-6)
    k.err("ce", "dlogits", dz, 5e-6)
    k.done()


@pytest.mark.parametrize("n", NE.L1_SIZES)
def test_l1_loss_edges(ops, n):
    """l1_loss with pred == target on every second element: the gradient there is exactly 0, elsewhere exactly
    +-grad_scale; the loss within test_l1_loss's 1e-5 sqrt(n) + 1e-6, taken relative to the loss."""
    c = NE.l1_case(n)
    k = Checks(c)
    p, t = c.inp["pred"], c.inp["target"]
    loss, dp = torch.zeros(1, device=DEV), new(n)
    ops.l1_loss(dev(p), dev(t), loss, dpred=dp, grad_scale=0.25)
    k.err("l1", "loss", loss, (1e-5 * n ** 0.5 + 1e-6) / float(c.ref["loss"]))
    k.true("l1", "gradient exactly 0 at the ties", bool((dp.cpu()[c.inp["tie"]] == 0).all()))
    k.true("l1", "gradient exactly +-scale elsewhere", torch.equal(dp.cpu(), 0.25 * torch.sign(p - t)))
    k.done()


@pytest.mark.parametrize("shape", NE.L1_UNPATCHIFY_SHAPES, ids=name)
def test_l1_unpatchify_edges(ops, shape):
    """l1_unpatchify with recon == img on every second pixel (test_l1_unpatchify's bounds: the mean loss to 1e-6, the
    gradient to 1e-9, the reconstruction a copy)."""
    c = NE.l1_unpatchify_case(shape)
    B, C, S, p = shape
    k = Checks(c)
    pred, img = c.inp["pred"], c.inp["img"]
    recon, loss, dpred = new(B, C, S, S), torch.zeros(1, device=DEV), new(*pred.shape)
    ops.l1_unpatchify(dev(pred), dev(img), loss, recon=recon, dpred=dpred, grad_scale=1.0 / img.numel(), p=p)
    k.true("l1unp", "recon is a copy", torch.equal(recon.cpu(), c.inp["recon"]))
    k.err("l1unp", "loss", loss, 1e-6 * img.numel() / float(c.ref["loss"]))
    k.true("l1unp", "gradient exactly 0 at the ties and on the CLS row", bool((dpred.cpu()[c.inp["zero"]] == 0).all()))
    k.true("l1unp", "gradient", torch.allclose(dpred.cpu().double(), c.ref["sign"] / img.numel(), atol=1e-9, rtol=0))
    k.done()


# ------------------------------------------------------------------------------------------------------------ SOM
FORWARD_ONLY = ("cos_scaled", "cos_identical")          # BMU properties; the neighbourhood runs on the other kinds
SOM_IDS = [(i, kd, T) for i in range(len(NE.SOM_SHAPES)) for kd in NE.SOM_KINDS for T in NE.SOM_T
           if not (kd in FORWARD_ONLY and T != NE.SOM_T[0])]
# relative bounds of test_som_neigh_loss_and_bwd / test_som_euclidean_fwd_and_bwd / test_som_manhattan_fwd_and_bwd
GRAD_FLOOR = {"cosine": 2e-5, "euclidean": 5e-5, "manhattan": 5e-6}
# distances: 2e-6 absolute (test_bmu_cosine); the matmul-form euclidean distance is a GEMM dot plus two norms under a
# square root, hence GEMM_TOL relative; Manhattan 2e-6 relative (test_som_manhattan_fwd_and_bwd)
DIST_FLOOR = {"cosine": 2e-6, "euclidean": GEMM_TOL, "manhattan": 2e-6}
# loss: 1e-6 absolute (cosine), 1e-5 relative (the other two), as the three tests above
LOSS_FLOOR = {"cosine": 1e-6, "euclidean": 1e-5, "manhattan": 1e-5}


@pytest.mark.parametrize("i,kind,T", SOM_IDS, ids=name)
def test_som_edges(ops, i, kind, T):
    c = NE.som_case(i, kind, T)
    B, K, L = c.shape[:3]
    fcn = c.fcn
    code = {"cosine": ops.DIST_COSINE, "euclidean": ops.DIST_EUCLIDEAN, "manhattan": ops.DIST_MANHATTAN}[fcn]
    k = Checks(c)
    x, W, grid = dev(c.inp["x"]), dev(c.inp["W"]), dev(c.inp["grid"])
    d64, bmu_ref = c.ref["dist"], c.ref["bmu"]
    dist, bmu = new(B, K), torch.full((B,), -1, dtype=torch.int64, device=DEV)
    inx = inw = None

    def bmu_checks(variant, dist, bmu):
        bm, di = bmu.cpu(), dist.cpu()
        k.true(variant, "bmu is the first argmin of the returned distances", torch.equal(bm, di.argmin(1)))
        k.true(variant, "bmu is the fp64 argmin outside near-ties", bmu_policy_ok(bm.clamp(0, K - 1), d64)[0])
        k.true(variant, "distances finite", bool(torch.isfinite(di).all()))
        if kind == "cos_zero":
            k.true(variant, "distance exactly 1 at the zero row / prototype", bool((di[2] == 1).all() and (di[:, 1] == 1).all()))
            k.true(variant, "zero row's BMU is 0", int(bm[2]) == 0)
        if kind == "cos_identical":
            k.true(variant, "every BMU is 0", bool((bm == 0).all()))
        if kind == "euclid_coincident":
            k.true(variant, "the coincident prototype wins, the lower twin wins", int(bm[7]) == 3 and bool((bm != 5).all()))
            k.true(variant, "bmu equals the fp64 argmin", torch.equal(bm, bmu_ref))
        if kind == "manhattan_grid":
            k.true(variant, "exact sums: distances and BMUs bitwise", torch.equal(di.double(), d64) and torch.equal(bm, bmu_ref))

    if fcn == "cosine":
        inx, inw = new(B), new(K)
        ops.row_inv_norm(x, inx)
        ops.row_inv_norm(W, inw)
        for nm, got, t in (("inv_nx", inx, c.inp["x"]), ("inv_nw", inw, c.inp["W"])):
            want = 1 / t.double().norm(dim=1).clamp_min(NE.NORM_EPS)
            k.true("row_inv_norm", nm + " to 2e-6 relative (test_bmu_cosine)", torch.allclose(got.cpu().double(), want, rtol=2e-6, atol=0))
        ops.bmu_cosine_fwd(x, W, inx, inw, dist, bmu)
        k.err("bmu_cosine", "dist", dist, DIST_FLOOR[fcn])
        bmu_checks("bmu_cosine", dist, bmu)
        dist3, bmu3, inx3, inw3 = new(B, K), torch.full((B,), -1, dtype=torch.int64, device=DEV), new(B), new(K)
        ops.bmu_cosine_x3_fwd(x, W, dist3, bmu3, inx3, inw3)
        k.err("bmu_cosine_x3", "dist", dist3, 1e-5)                          # test_bmu_cosine_x3_rerank
        bmu_checks("bmu_cosine_x3", dist3, bmu3)
        if kind == "cos_scaled":                                             # the BMUs of the unscaled rows, on the device
            plain = dev(NE.rnd(B, L, seed=1))
            ip, bp = new(B), torch.full((B,), -1, dtype=torch.int64, device=DEV)
            ops.row_inv_norm(plain, ip)
            ops.bmu_cosine_fwd(plain, W, ip, inw, None, bp)
            k.true("bmu_cosine", "scaling a row leaves its BMU", torch.equal(bmu, bp) and torch.equal(bmu3, bp))
    elif fcn == "euclidean":
        sx, sw = new(B), new(K)
        ops.row_sqnorm(x, sx)
        ops.row_sqnorm(W, sw)
        ops.bmu_euclid_fwd(x, W, sx, sw, dist, bmu)
        k.err("bmu_euclid", "dist", dist, DIST_FLOOR[fcn])
        bmu_checks("bmu_euclid", dist, bmu)
    else:
        ops.bmu_manhattan_fwd(x, W, dist, bmu)
        k.err("bmu_manhattan", "dist", dist, DIST_FLOOR[fcn])
        bmu_checks("bmu_manhattan", dist, bmu)

    same_bmu = torch.equal(bmu.cpu(), bmu_ref)
    if kind not in FORWARD_ONLY:
        k.true("bmu", "the BMUs the neighbourhood is built from are the reference's", same_bmu)
    if kind not in FORWARD_ONLY and same_bmu:
        scale = NE.SOM_GAMMA / (B * K)
        h, loss, coef = new(B, K), torch.zeros(1, device=DEV), new(B, K)
        rd, cd = (None, None) if fcn == "manhattan" else (new(B), new(K))
        ops.som_neigh_loss(dist, bmu, grid, T, loss, h=h, inv_nx=inx, inv_nw=inw, grad_scale=scale, coef=coef, row_dot=rd,
                           col_dot=cd, distance=code)
        off = c.onehot == 0
        if T < 1:
            k.true("neigh", "h is the one-hot of the BMU, bit for bit", torch.equal(h.cpu(), c.onehot))
            k.true("neigh", "coef exactly 0 off the BMU", bool((coef.cpu()[off] == 0).all()))
            if fcn != "manhattan":
                # row_dot and col_dot in closed form for a one-hot h (fp64, from the reference's distances): cosine
                # c (1 - d_i,b(i)) / |x_i|^2 and c sum_{i: b(i) = k} (1 - d_ik) / |w_k|^2, euclidean c / d_i,b(i) and
                # c sum_{i: b(i) = k} 1 / d_ik with 0 at d = 0; held to the gradients' bound
                db = d64.gather(1, bmu_ref.view(-1, 1)).squeeze(1)
                if fcn == "cosine":
                    term = 1 - db
                    wx = 1 / c.inp["x"].double().norm(dim=1).clamp_min(NE.NORM_EPS) ** 2
                    ww = 1 / c.inp["W"].double().norm(dim=1).clamp_min(NE.NORM_EPS) ** 2
                else:
                    term = torch.where(db > 0, 1 / db.clamp_min(1e-300), torch.zeros_like(db))
                    wx, ww = torch.ones(B, dtype=torch.float64), torch.ones(K, dtype=torch.float64)
                rd_ref = scale * wx * term
                cd_ref = scale * ww * torch.zeros(K, dtype=torch.float64).index_add_(0, bmu_ref, term)
                k.err("neigh", "gX.row_dot", rd, GRAD_FLOOR[fcn], rd_ref, 0.0)
                k.err("neigh", "gW.col_dot", cd, GRAD_FLOOR[fcn], cd_ref, 0.0)
        else:
            k.err("neigh", "h", h, 2e-6)                                     # test_som_neigh_loss_and_bwd
        k.err("neigh", "loss", loss / (B * K), LOSS_FLOOR[fcn])
        gW, gX = new(K, L), new(B, L)
        if fcn == "manhattan":
            ops.som_bwd_manhattan(x, W, coef, gW, gX, accumulate_gx=False)
        else:
            ops.som_bwd(x, W, coef, rd, cd, gW, gX, accumulate_gx=False)
        k.err("som_bwd", "gW", gW, GRAD_FLOOR[fcn])
        k.err("som_bwd", "gX", gX, GRAD_FLOOR[fcn])
        k.true("som_bwd", "gradients finite", bool(torch.isfinite(gW).all() and torch.isfinite(gX).all()))
        if kind == "cos_zero":                                               # the rows that do not carry a 1 / eps factor
            lw, lx = torch.arange(K) != 1, torch.arange(B) != 2
            k.err("som_bwd", "gW.live", gW.cpu()[lw], GRAD_FLOOR[fcn], c.ref["gW"][lw], NE.rel_err(c.y32["gW"][lw], c.ref["gW"][lw]))
            k.err("som_bwd", "gX.live", gX.cpu()[lx], GRAD_FLOOR[fcn], c.ref["gX"][lx], NE.rel_err(c.y32["gX"][lx], c.ref["gX"][lx]))
        # the same loss with the neighbourhood handed in as explicit weights
        loss2, coef2 = torch.zeros(1, device=DEV), new(B, K)
        rd2, cd2 = (None, None) if fcn == "manhattan" else (new(B), new(K))
        ops.som_weighted_loss(dist, h, loss2, inv_nx=inx, inv_nw=inw, grad_scale=scale, coef=coef2, row_dot=rd2, col_dot=cd2,
                              distance=code)
        k.err("weighted", "loss", loss2 / (B * K), LOSS_FLOOR[fcn])
        same = torch.equal(coef2, coef) and (rd is None or (torch.equal(rd2, rd) and torch.equal(cd2, cd)))
        k.true("weighted", "coefficients are those of the neighbourhood form", same)
    k.done()


# ------------------------------------------------------------------------------------------------------------ AdamW
@pytest.mark.parametrize("step", NE.ADAMW_STEPS)
def test_adamw_edges(ops, step):
    """adamw_step and adamw_step_planes on gradient chunks of 0, 1e-20, 1e15 and +-1: 2e-7 absolute (test_adamw_step);
    the planes form updates the arena bit for bit like the flat one."""
    c = NE.adamw_case(step)
    k = Checks(c)
    hp = NE.ADAMW_HP
    wd = torch.tensor(NE.ADAMW_WD, device=DEV)
    g = dev(c.inp["g"]).view(-1)
    state = []
    for planes in (False, True):
        p, m, v = (dev(c.inp[n]).view(-1).clone() for n in ("p", "m", "v"))
        buf = ops.bmu_planes_alloc(16, 32, DEV) if planes else None
        ops.adamw_step(p, g, m, v, wd, hp["lr"], hp["b1"], hp["b2"], hp["eps"], step,
                       planes=(256, 16, 32, buf) if planes else None)
        k.err("planes" if planes else "flat", "p", p.view(4, 256), 2e-7)
        k.true("adamw", "moments finite", bool(torch.isfinite(m).all() and torch.isfinite(v).all()))
        state.append((p, m, v))
    k.true("adamw", "planes form == flat form", all(torch.equal(a, b) for a, b in zip(*state)))
    k.done()
