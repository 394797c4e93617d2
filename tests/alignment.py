"""The host-side choice between the 16-byte load path and the element-wise one, as data: one row per entry point (or per
form of one) at the smallest shape that takes the 16-byte path, with what the SOURCE does when one operand alone stops
being 16-byte aligned.  tests/test_alignment_cpu.py pins every alignment test in vit_som_amd/csrc to these rows (or to
LEFT_OUT), calls every refusal on the host with stand-in pointers and holds include/vitsom_hip.h to them;
tests/test_alignment_gpu.py runs every row through its ops wrapper inside guarded arenas (memcheck.py, `shift`).  The
behaviours below were read from the dispatch conditions AND the kernel bodies, not asked of the library.

An operand's behaviour when its base is shifted by 1 or 2 elements (`shifted`), and, where the entry takes a leading
dimension for it, when its row pitch grows by 1 or 2 (`pitched`):
  SAME      the operand takes part in no dispatch and every kernel reads / writes it one element at a time (or decides the
            width of an access from the address, inside the kernel): the same kernels run, the outputs are bit-identical
            to the aligned call's;
  ELEMENT   the call falls to the element-wise path: no error, the outputs pass the row's check;
  REFUSED   no element-wise path exists: the library answers `code` before any launch that would use the operand (or, by
            "wrapper", the ops wrapper raises ValueError naming the argument).
A shift that leaves the base 16-byte aligned (two elements of an 8-byte type) is an aligned call: SAME whatever the marking.

Sites found (alignment tests: `aligned16(` and the spelled-out `& 15` / `& 7` / `& 3` pointer tests), by file -- SITES
below holds every one of them, with the rows that cross it:
  gemm_f32.hip     launch_gemm (a_vec, b_vec -> `fast`): every Linear / SOM / BMU GEMM; reduce_slabs2_internal (the slabs);
                   linear_bwd_input_ln_launch (refusal); linear_bwd_weight_impl (`vec`: the weight-gradient tiles); two
                   workspace tests.
  gemm_f32.h       reduce_slabs_body: the destination's alignment decides the store width inside the kernel.
  layernorm.hip    forward (X, Y, gamma, beta), backward (dY, X, gamma, dX, resid); ln_finish_many_kernel tests its partial
                   buffer in the kernel; two workspace tests.
  som.hip          row_inv_norm, row_sqnorm (X).       som_l1.hip  the Manhattan pass (X, W) and its backward (X, W, coef).
  pca.hip          pca_contract (A, B, mean); three workspace tests.
  knn.hip          knn_search (Q, X), knn_ranks (A), silhouette (X); four workspace tests.
  kmeans.hip       assign (X, centers); four workspace tests.       gmm.hip  E-step (X, means, prec).
  agglomerative.hip  distances (X); the 8-byte test of the merge workspace.
  batch_som.hip    accumulate (X), update (sums).      mapquality.hip  map_stats (dist), umatrix (W).
  mapviz.hip       proto_mosaic (pred).                umap.hip        one workspace test.
  bmu_x3.hip       the three-product BMU forms: x3_dots (X, W refused), both finalize entries (X, W refused: the
                   re-rank reads their rows wide), the finalize kernel's slab (workspace), planes_from (src), adamw_step_planes
                   (p, g, m, v), planes_dots (the images); three workspace / plane-buffer tests.
  attention.hip    forward and backward refuse at hd = 16, 32, 64 and have no requirement at hd <= 8.
  attention_q1.hip forward (q, kv, o), backward (dout, o, q, kv, dkv).
  misc.hip         adamw_step (p, g, m, v).            tsne.hip        repulsion (Y).
  augment.hip, augment_ragged.hip   the plan / batch entries refuse misaligned records and outputs; two in-kernel tests
                   of the image's byte offset.

The two finalize entries of the three-product BMU forms matter on their own: ops.bmu_cosine_x3_planes_fwd hands X and W to
vsom_bmu_cosine_x3_planes_finalize alone (the stage before it sees only the plane images), so that entry's own test of the
pointers is what keeps a shifted view from the re-rank's 16-byte loads.

Looked at and left out: LEFT_OUT below, each with its reason.

Far pitches -- a last row 2 GiB, 4 GiB or 2^31 elements from the base -- are the subject of tests/far_pitch.py, which reuses
these rows for every operand marked `ld=True`.
"""
import functools
import math
import re
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

import numeric_edges as NE
import pca_ref
from helpers import rel_err
from launch_plan_rows import (BWD_INPUT, BWD_INPUT_T, BWD_WEIGHT, BMU_COSINE_DOTS, F32, GRAD3, LINEAR_FWD, LINEAR_GELU_FWD,
                              LINEAR_RELU_FWD, LINEAR_RESIDUAL_FWD, SOM_BWD_GW, SPLIT)

SAME, ELEMENT = "same", "element"
EINVAL, EALIGN, EUNSUPPORTED, EWORKSPACE = -1, -2, -3, -4               # include/vitsom_hip.h: VSOM_E*
IN, OUT, INOUT = "in", "out", "inout"
F32T, F64T, I32T, I64T, U8T = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
EPS32 = 2.0 ** -23
GEMM_TOL = 2e-6                                  # test_ops_gpu.GEMM_TOL
ALL_MODES = (F32, SPLIT, GRAD3)
MODE_IDS = {F32: "f32", SPLIT: "split_bf16", GRAD3: "grad3"}


class REFUSED(namedtuple("REFUSED", "code by")):
    """The library's negative status (`by` = "library"), or the wrapper's ValueError (`by` = "wrapper", code None)."""
    __slots__ = ()

    def __new__(cls, code, by="library"):
        return super().__new__(cls, code, by)


# name: the wrapper's argument; dtype; role; ld: the entry takes a leading dimension for it; shifted / pitched: see above
Op = namedtuple("Op", "name dtype role ld shifted pitched", defaults=(False, SAME, None))
# A tensor the test allocates for an output: shape and dtype
Spec = namedtuple("Spec", "shape dtype")
# id; wrapper: the function of vit_som_amd.ops; entry: the C entries it reaches; make() -> case (t: operands by name -- a
# tensor for IN / INOUT, a Spec for OUT --, a: further arguments, plus whatever check needs); call(ops, t, a) runs the wrapper
# and may return a dict of tensors the wrapper allocated itself; check(case, out) -> list of complaints (empty: pass), out =
# every OUT / INOUT operand and every returned tensor, on the CPU; modes: the GEMM modes the row runs under (None: the
# current one); plan: (VSOM_PLAN_* op, shape) of a GEMM-family row for vsom_describe_plan
Row = namedtuple("Row", "id wrapper entry make call ops check modes plan", defaults=(None, None))


# ------------------------------------------------------------------------------------------------------- helpers
def ints(*shape, seed, lo=-3, hi=3):
    """Integers in [lo, hi] as float32: exact in fp32 and in every bf16 piece, sums independent of their order."""
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def exact(name, got, want):
    """got == want element for element (want: fp64 / int64 reference of an operation that is exact on its inputs)."""
    got, want = torch.as_tensor(got), torch.as_tensor(want)
    if got.shape != want.shape:
        return [f"{name}: shape {tuple(got.shape)} != {tuple(want.shape)}"]
    bad = got.double() != want.double()
    if bool(bad.any()):
        i = int(bad.reshape(-1).nonzero()[0])
        return [f"{name}: {int(bad.sum())} of {bad.numel()} elements differ from the exact result, the first at flat index {i}: "
                f"{float(got.reshape(-1)[i])!r} != {float(want.reshape(-1)[i])!r}"]
    return []


def close(name, got, ref64, y32, floor, metric):
    """numeric_edges' rule: e_k <= max(floor, 4 e32), e32 the float32 torch evaluation's error in the same metric."""
    e32, e_k = metric(y32, ref64), metric(got, ref64)
    print(f"ALIGN|{name}|e32={e32:.3e}|e_k={e_k:.3e}|bound={NE.bound(floor, e32):.3e}")
    return [] if NE.accepts(e_k, floor, e32) else [f"{name}: error {e_k:.3e} > max({floor:g}, 4 x {e32:.3e})"]


def close_nofloor(name, got, ref64, y32):
    """An entry without a floor of its own: 4 x max(e32, 2^-23), largest absolute error over largest absolute value
    (pca_ref.bound)."""
    e_k, lim = pca_ref.rel_err(got, ref64), pca_ref.bound(y32, ref64)
    print(f"ALIGN|{name}|e_k={e_k:.3e}|bound={lim:.3e}")
    return [] if e_k <= lim else [f"{name}: error {e_k:.3e} > 4 x max(e32, 2^-23) = {lim:.3e}"]


def case(t, a=None, **more):
    return SimpleNamespace(t=t, a=a or {}, **more)


def spec_like(ref, dtype=F32T):
    return Spec(tuple(ref.shape), dtype)


# ------------------------------------------------------------------------------------------------------- GEMM family
# M = 130: one full 128-row tile and a ragged one; N = 70: one 64-column tile and a tail; the extents along which the
# 16-byte loads run are multiples of 4 but not of 16 (52, 20)
LIN_M, LIN_N, LIN_K = 130, 70, 52


@functools.lru_cache(maxsize=None)
def _linear():
    x, W, b, R = ints(LIN_M, LIN_K, seed=1), ints(LIN_N, LIN_K, seed=2), ints(LIN_N, seed=3), ints(LIN_M, LIN_N, seed=4)
    pre = x.double() @ W.double().T + b.double()
    assert float(pre.abs().max()) < 2 ** 24
    return x, W, b, R, pre


def make_linear_fwd():
    x, W, b, _, pre = _linear()
    return case({"x": x, "W": W, "bias": b, "out": spec_like(pre)}, pre=pre)


def make_linear_gelu_fwd():
    x, W, b, _, pre = _linear()
    ref, y32 = NE.gelu_eval(pre, F64T), NE.gelu_eval(pre.float(), F32T)
    return case({"x": x, "W": W, "bias": b, "grad": spec_like(pre), "act": spec_like(pre)}, ref=ref, y32=y32)


def check_linear_gelu_fwd(c, out):
    """test_linear_gelu_fwd's bounds on exact (integer) pre-activations: 5e-6 on |act - ref| / (1 + |ref|) and on gelu'."""
    return (close("act", out["act"], c.ref["act"], c.y32["act"], 5e-6, NE.act_err) +
            close("grad", out["grad"], c.ref["grad"], c.y32["grad"], 5e-6, NE.max_abs))


def make_linear_relu_fwd():
    x, W, b, _, pre = _linear()
    return case({"x": x, "W": W, "bias": b, "ygrad": spec_like(pre), "yact": spec_like(pre)}, pre=pre)


def make_linear_residual_fwd():
    x, W, b, R, pre = _linear()
    return case({"x": x, "W": W, "bias": b, "R": R, "out": spec_like(pre)}, a={"r_mod": LIN_M}, pre=pre + R.double())


@functools.lru_cache(maxsize=None)
def _bwd():
    dy, W = ints(LIN_M, LIN_K, seed=5), ints(LIN_K, LIN_N - 2, seed=6)             # dX [130, 68] = dY [130, 52] W [52, 68]
    return dy, W, dy.double() @ W.double()


def make_linear_bwd_input():
    dy, W, dx = _bwd()
    return case({"dy": dy, "W": W, "dx": spec_like(dx)}, dx=dx)


def make_linear_bwd_input_t():
    dy, W, dx = _bwd()
    return case({"dy": dy, "Wt": W.T.contiguous(), "dx": spec_like(dx)}, dx=dx)


def make_linear_bwd_weight(M=LIN_M, N=68, K=LIN_K):
    def make():
        dy, x = ints(M, N, seed=7), ints(M, K, seed=8)                               # dW [N, K] = dY^T X, db [N]
        dW, db = dy.double().T @ x.double(), dy.double().sum(0)
        assert float(dW.abs().max()) < 2 ** 24
        return case({"dy": dy, "x": x, "dW": spec_like(dW), "db": spec_like(db)}, dW=dW, db=db)
    return make


SOM_B, SOM_K, SOM_L = 70, 16, 52                                                     # K % 4: the k-strided coef takes 16-byte loads


def make_som_bwd():
    x, W, coef = ints(SOM_B, SOM_L, seed=9), ints(SOM_K, SOM_L, seed=10), ints(SOM_B, SOM_K, seed=11)
    rd, cd = ints(SOM_B, seed=12), ints(SOM_K, seed=13)
    gW = coef.double().T @ x.double() + cd.double()[:, None] * W.double()
    gX = coef.double() @ W.double() + rd.double()[:, None] * x.double()
    return case({"x": x, "W": W, "coef": coef, "row_dot": rd, "col_dot": cd, "gW": spec_like(gW), "gX": spec_like(gX)}, gW=gW, gX=gX)


def _bmu_ints(B, K, L):
    return ints(B, L, seed=14), ints(K, L, seed=15)


def make_bmu_euclid(B, K, L):
    def make():
        x, W = _bmu_ints(B, K, L)
        sx, sw = (x.double() ** 2).sum(1), (W.double() ** 2).sum(1)
        d2 = sx[:, None] + sw[None, :] - 2 * (x.double() @ W.double().T)
        # integers below 2^24 and sqrtf correctly rounded (numpy's float32 root is; torch's vectorised one on the host is not)
        dist = torch.from_numpy(np.sqrt(d2.numpy().astype(np.float32)))
        return case({"x": x, "W": W, "sq_x": sx.float(), "sq_w": sw.float(), "dist": Spec((B, K), F32T), "bmu": Spec((B,), I64T)},
                    dist=dist, bmu=d2.argmin(1))
    return make


def check_dist_bmu(c, out):
    return exact("dist", out["dist"], c.dist) + exact("bmu", out["bmu"], c.bmu)


def make_bmu_manhattan(B, K, L):
    def make():
        x, W = _bmu_ints(B, K, L)
        d = (x.double()[:, None, :] - W.double()[None, :, :]).abs().sum(-1)
        return case({"x": x, "W": W, "dist": Spec((B, K), F32T), "bmu": Spec((B,), I64T)}, dist=d, bmu=d.argmin(1))
    return make


def make_som_bwd_manhattan():
    x, W, coef = ints(SOM_B, SOM_L, seed=9), ints(SOM_K, SOM_L, seed=10), ints(SOM_B, SOM_K, seed=11)
    sg = torch.sign(x.double()[:, None, :] - W.double()[None, :, :])
    gX, gW = torch.einsum("bk,bkl->bl", coef.double(), sg), -torch.einsum("bk,bkl->kl", coef.double(), sg)
    return case({"x": x, "W": W, "coef": coef, "gW": spec_like(gW), "gX": spec_like(gX)}, gW=gW, gX=gX)


def make_bmu_cosine(B, K, L, planes=False):
    """N(0, 1) samples against uniform prototypes, as test_bmu_cosine: dist to the cosine floors, the BMU by bmu_policy_ok."""
    def make():
        x = rnd(B, L, seed=1)
        W = torch.rand(K, L, generator=torch.Generator().manual_seed(2))
        ref, y32 = NE.cosine_dist(x.double(), W.double()), NE.cosine_dist(x, W)
        t = {"x": x, "W": W, "dist": Spec((B, K), F32T), "bmu": Spec((B,), I64T), "inv_nx": Spec((B,), F32T), "inv_nw": Spec((K,), F32T)}
        return case(t, ref=ref, y32=y32, inx=1 / x.double().norm(dim=1).clamp_min(NE.NORM_EPS),
                    inw=1 / W.double().norm(dim=1).clamp_min(NE.NORM_EPS))
    return make


def check_bmu_cosine(floor):
    def check(c, out):
        from test_ops_gpu import bmu_policy_ok
        bad = close("dist", out["dist"], c.ref, c.y32, floor, NE.max_abs)
        bm = out["bmu"]
        if not torch.equal(bm, out["dist"].argmin(1)):
            bad.append("bmu is not the first argmin of the returned distances")
        if not bmu_policy_ok(bm.clamp(0, c.ref.shape[1] - 1), c.ref)[0]:
            bad.append("bmu differs from the fp64 argmin outside a near-tie")
        for n, want in (("inv_nx", c.inx), ("inv_nw", c.inw)):                         # 2e-6 relative (test_bmu_cosine)
            if not torch.allclose(out[n].double(), want, rtol=2e-6, atol=0):
                bad.append(f"{n}: beyond 2e-6 relative")
        return bad
    return check


def make_bmu_cosine_exact(B, K, L):
    inner = make_bmu_cosine(B, K, L)

    def make():
        c = inner()
        c.t["inv_nx"], c.t["inv_nw"] = c.inx.float(), c.inw.float()                    # inputs of the exact form
        return c
    return make


def check_bmu_cosine_exact(c, out):
    from test_ops_gpu import bmu_policy_ok
    bad = close("dist", out["dist"], c.ref, c.y32, 2e-6, NE.max_abs)
    if not torch.equal(out["bmu"], out["dist"].argmin(1)):
        bad.append("bmu is not the first argmin of the returned distances")
    if not bmu_policy_ok(out["bmu"].clamp(0, c.ref.shape[1] - 1), c.ref)[0]:
        bad.append("bmu differs from the fp64 argmin outside a near-tie")
    return bad


def make_planes_from():
    src = ints(192, 256, seed=16)
    return case({"src": src}, a={"R": 192, "L": 256})


def make_reduce_slabs():
    slabs = ints(37, 1028, seed=17)                                                  # 37 slabs (>= 32) of 1028 = 4 x 257 columns
    return case({"slabs": slabs, "out": Spec((1028,), F32T)}, want=slabs.double().sum(0))


PE = dict(B=9, C=3, S=8, p=2, E=20)                                                  # 144 patch rows of 12 values: a 128-row tile and a tail


def make_patch_embed_fwd():
    B, C, S, p, E = PE["B"], PE["C"], PE["S"], PE["p"], PE["E"]
    g = S // p
    n, pd = g * g, C * p * p
    img, Wpe, bpe = ints(B, C, S, S, seed=40), ints(E, pd, seed=41), ints(E, seed=42)
    pos, cls = ints(n + 1, E, seed=43), ints(E, seed=44)
    xp = img.unfold(2, p, p).unfold(3, p, p).permute(0, 2, 3, 1, 4, 5).reshape(B * n, pd)
    tok = torch.empty(B, n + 1, E, dtype=F64T)
    tok[:, 1:] = (xp.double() @ Wpe.double().T + bpe.double()).view(B, n, E) + pos.double()[1:]
    tok[:, 0] = cls.double() + pos.double()[0]
    return case({"img": img, "Wpe": Wpe, "bpe": bpe, "pos": pos, "cls_token": cls, "tokens": spec_like(tok), "xp_ws": spec_like(xp)},
                {"p": p}, tokens=tok, xp=xp)


def make_transpose_many():
    shapes = [(33, 20), (70, 52)]
    src = ints(sum(r * c for r, c in shapes), seed=45)
    table, want, off = [], [], 0
    for r, c in shapes:
        table.append([off, off, r, c])
        want.append(src[off:off + r * c].view(r, c).T.reshape(-1))
        off += r * c
    return case({"src_base": src, "dst_base": Spec((off,), F32T), "table": torch.tensor(table, dtype=I64T)},
                {"max_rows": 70, "max_cols": 52}, want=torch.cat(want))


LNF_M, LNF_N, LNF_K = 2048, 64, 192                                                  # the smallest supported shape (32 row tiles of 64)


def make_linear_bwd_input_ln():
    x = rnd(LNF_M, LNF_K, seed=3) * 2 + 0.5
    dy, Wt, gamma = rnd(LNF_M, LNF_N, seed=1), rnd(LNF_K, LNF_N, seed=2) * 0.05, 1 + 0.1 * rnd(LNF_K, seed=4)
    ref, y32 = NE.ln_fused_eval(dy, Wt, x, gamma, F64T), NE.ln_fused_eval(dy, Wt, x, gamma, F32T)
    t = {"dy": dy, "Wt": Wt, "x": x, "mean": ref["mean"].float(), "rstd": torch.rsqrt(ref["var"] + NE.LN_EPS).float(), "gamma": gamma,
         "dx": spec_like(x), "dgamma": Spec((LNF_K,), F32T), "dbeta": Spec((LNF_K,), F32T)}
    return case(t, ref=ref, y32=y32)


def check_linear_bwd_input_ln(c, out):
    """test_plan_row_against_fp64 / test_ln_fused_edges in VSOM_GEMM_SPLIT_BF16 mode (three planes): GEMM_TOL, relative."""
    return [m for n in ("dx", "dgamma", "dbeta") for m in close(n, out[n], c.ref[n], c.y32[n], GEMM_TOL, rel_err)]


# ------------------------------------------------------------------------------------------------------- row norms
def make_row_norm(rows, cols, squared):
    def make():
        x = ints(rows, cols, seed=18) if squared else rnd(rows, cols, seed=18)
        s = (x.double() ** 2).sum(1)
        ref = s if squared else 1 / s.sqrt().clamp_min(1e-12)
        y32 = (x ** 2).sum(1) if squared else 1 / x.norm(dim=1).clamp_min(1e-12)
        return case({"x": x, "out": Spec((rows,), F32T)}, ref=ref, y32=y32)
    return make


# ------------------------------------------------------------------------------------------------------- LayerNorm
LN_ROWS = 70                                                                          # four 16-row groups and a ragged one


def make_layernorm(cols, backward):
    def make():
        x = rnd(LN_ROWS, cols, seed=1) * 2 + 0.5
        gamma, beta = 1 + 0.1 * rnd(cols, seed=2), 0.1 * rnd(cols, seed=3)
        dy, resid = rnd(LN_ROWS, cols, seed=4), rnd(LN_ROWS, cols, seed=5)
        ref, y32 = NE.layernorm_eval(x, gamma, beta, dy, resid, F64T), NE.layernorm_eval(x, gamma, beta, dy, resid, F32T)
        for d in (ref, y32):
            d["rstd"] = torch.rsqrt(d["var"] + NE.LN_EPS)
        if not backward:
            t = {"x": x, "gamma": gamma, "beta": beta, "y": spec_like(x), "mean": Spec((LN_ROWS,), F32T), "rstd": Spec((LN_ROWS,), F32T)}
        else:                                                                         # mean / rstd as an exact forward leaves them
            t = {"dy": dy, "x": x, "mean": ref["mean"].float(), "rstd": ref["rstd"].float(), "gamma": gamma, "resid": resid,
                 "dx": spec_like(x), "dgamma": Spec((cols,), F32T), "dbeta": Spec((cols,), F32T)}
        return case(t, ref=ref, y32=y32)
    return make


def check_layernorm_fwd(c, out):
    """y: 3e-6 absolute (test_layernorm, test_layernorm_edges); mean and rstd have no floor of their own."""
    return (close("y", out["y"], c.ref["y"], c.y32["y"], 3e-6, NE.max_abs) +
            close_nofloor("mean", out["mean"], c.ref["mean"], c.y32["mean"]) +
            close_nofloor("rstd", out["rstd"], c.ref["rstd"], c.y32["rstd"]))


def check_layernorm_bwd(c, out):
    """5e-6 relative (test_layernorm, test_layernorm_edges)."""
    return (close("dx", out["dx"], c.ref["dx_resid"], c.y32["dx_resid"], 5e-6, rel_err) +
            close("dgamma", out["dgamma"], c.ref["dgamma"], c.y32["dgamma"], 5e-6, rel_err) +
            close("dbeta", out["dbeta"], c.ref["dbeta"], c.y32["dbeta"], 5e-6, rel_err))


# ------------------------------------------------------------------------------------------------------- attention
ATTN_B, ATTN_H = 2, 2


def make_attention(N, hd, backward):
    def make():
        B, H, E = ATTN_B, ATTN_H, ATTN_H * hd
        qkv, dout = rnd(B, N, 3 * E, seed=1), rnd(B, N, E, seed=2)
        ref, y32 = NE.attention_eval(qkv, dout, B, N, H, hd, F64T), NE.attention_eval(qkv, dout, B, N, H, hd, F32T)
        for d, dt in ((ref, F64T), (y32, F32T)):                                       # delta[b, h, i] = <dout, out> over the head
            d["delta"] = (dout.to(dt) * d["out"]).view(B, N, H, hd).sum(-1).permute(0, 2, 1).contiguous()
        a = {"B": B, "N": N, "H": H, "hd": hd}
        if not backward:
            return case({"qkv": qkv, "out": Spec((B, N, E), F32T), "lse": Spec((B, H, N), F32T)}, a, ref=ref, y32=y32)
        return case({"qkv": qkv, "out": ref["out"].float(), "dout": dout, "lse": ref["lse"].float(), "dqkv": Spec((B, N, 3 * E), F32T),
                     "delta": Spec((B, H, N), F32T)}, a, ref=ref, y32=y32)
    return make


def check_attention_fwd(c, out):
    """3e-6 absolute (test_attention, test_attention_edges)."""
    return (close("out", out["out"], c.ref["out"], c.y32["out"], 3e-6, NE.max_abs) +
            close("lse", out["lse"], c.ref["lse"], c.y32["lse"], 3e-6, NE.max_abs))


def check_attention_bwd(c, out):
    """dqkv 5e-6 relative (test_attention_edges; the rows run in VSOM_GEMM_SPLIT_BF16 mode, where every form of the backward
    has fp32 products); the workspace delta has no floor of its own."""
    return (close("dqkv", out["dqkv"], c.ref["dqkv"], c.y32["dqkv"], 5e-6, rel_err) +
            close_nofloor("delta", out["delta"], c.ref["delta"], c.y32["delta"]))


Q1 = dict(B=3, N=17, H=2, hd=16)


def make_q1(backward):
    def make():
        B, N, H, hd = Q1["B"], Q1["N"], Q1["H"], Q1["hd"]
        E = H * hd
        q, kv, dout = rnd(B, E, seed=1), rnd(B * N, 2 * E, seed=2), rnd(B, E, seed=3)
        ref, y32 = NE.q1_eval(q, kv, dout, B, N, H, hd, F64T), NE.q1_eval(q, kv, dout, B, N, H, hd, F32T)
        if not backward:
            return case({"q": q, "kv": kv, "out": Spec((B, E), F32T), "lse": Spec((B, H), F32T)}, dict(Q1), ref=ref, y32=y32)
        return case({"dout": dout, "out": ref["out"].float(), "lse": ref["lse"].float(), "q": q, "kv": kv, "dq": Spec((B, E), F32T),
                     "dkv": Spec((B * N, 2 * E), F32T)}, dict(Q1), ref=ref, y32=y32)
    return make


def check_q1(names):
    def check(c, out):
        """1e-5 (test_attention_q1_against_fp64, test_attention_q1_edges): out / lse absolute, dq / dkv relative."""
        bad = []
        for n in names:
            bad += close(n, out[n], c.ref[n], c.y32[n], 1e-5, NE.max_abs if n in ("out", "lse") else rel_err)
        return bad
    return check


# ------------------------------------------------------------------------------------------------------- losses, AdamW
def make_cross_entropy():
    rows, C = 9, 20
    z, y = rnd(rows, C, seed=3) * 3, torch.randint(0, C, (rows,), generator=torch.Generator().manual_seed(4))
    ref, y32 = NE.ce_eval(z, y, 0.1, F64T), NE.ce_eval(z, y, 0.1, F32T)
    return case({"logits": z, "y": y, "loss_sum": Spec((1,), F32T), "dlogits": Spec((rows, C), F32T)}, ref=ref, y32=y32)


def check_cross_entropy(c, out):
    """test_cross_entropy_ls: the summed loss 2e-6 relative, dlogits 5e-6 absolute at grad_scale = 1."""
    return (close("loss", out["loss_sum"], c.ref["loss"], c.y32["loss"], 2e-6, rel_err) +
            close("dlogits", out["dlogits"], c.ref["dlogits"], c.y32["dlogits"], 5e-6, NE.max_abs))


def make_som_neigh_loss():
    B, K, L, grid_shape = 33, 12, 48, (4, 3)
    from oracle import vitsom_oracle as O
    x = rnd(B, L, seed=1)
    W = torch.nn.functional.normalize(torch.rand(K, L, generator=torch.Generator().manual_seed(2)), dim=1)
    grid = O.grid_positions(grid_shape, "hexa").float().contiguous()
    d64 = NE.cosine_dist(x.double(), W.double())
    bmu = d64.argmin(1)
    T = 1.5
    out = {}
    for key, dt in (("ref", F64T), ("y32", F32T)):
        d = d64.to(dt)
        h = O.neighbourhood(bmu, grid.to(dt), T)
        out[key] = {"h": h, "loss": (h * d).sum().reshape(1)}
    return case({"dist": d64.float(), "bmu": bmu, "grid": grid, "loss_sum": Spec((1,), F32T), "h": Spec((B, K), F32T)}, {"T": T},
                ref=out["ref"], y32=out["y32"], n=B * K)


def check_som_neigh_loss(c, out):
    """test_som_neigh_loss_and_bwd: h 2e-6 absolute, the mean loss 1e-6 absolute."""
    return (close("h", out["h"], c.ref["h"], c.y32["h"], 2e-6, NE.max_abs) +
            close("loss", out["loss_sum"] / c.n, c.ref["loss"] / c.n, c.y32["loss"] / c.n, 1e-6, NE.max_abs))


def make_adamw():
    e = NE.adamw_case(1000)
    t = {n: e.inp[n].reshape(-1).clone() for n in ("p", "g", "m", "v")}
    t["wd_chunk"] = torch.tensor(NE.ADAMW_WD)
    return case(t, {"step": 1000}, ref=e.ref, y32=e.y32)


def call_adamw_planes(ops, t, a):
    hp = NE.ADAMW_HP
    buf = ops.bmu_planes_alloc(16, 32, t["p"].device)                                # the [16, 32] slice at element 256, as test_adamw_edges
    ops.adamw_step(t["p"], t["g"], t["m"], t["v"], t["wd_chunk"], hp["lr"], hp["b1"], hp["b2"], hp["eps"], a["step"],
                   planes=(256, 16, 32, buf))


def check_adamw(c, out):
    """2e-7 absolute on the parameters (test_adamw_step, test_adamw_edges)."""
    bad = close("p", out["p"].view(4, 256), c.ref["p"], c.y32["p"], 2e-7, NE.max_abs)
    if not bool(torch.isfinite(out["m"]).all() and torch.isfinite(out["v"]).all()):
        bad.append("moments not finite")
    return bad


# ------------------------------------------------------------------------------------------------------- evaluation
PCA_N, PCA_D, PCA_L = 130, 52, 10


@functools.lru_cache(maxsize=None)
def _pca():
    X, B, mean = ints(PCA_N, PCA_D, seed=20), ints(PCA_L, PCA_D, seed=21), ints(PCA_D, seed=22, lo=-2, hi=2)
    scale = 2.0 ** ints(PCA_L, seed=23, lo=-1, hi=1)
    Y = (X.double() - mean.double()) @ B.double().T * scale.double()
    return X, B, mean, scale, Y


def make_pca_project():
    X, B, mean, scale, Y = _pca()
    return case({"X": X, "mean": mean, "B": B, "scale": scale, "Y": spec_like(Y)}, want=Y)


def make_pca_backproject():
    X, _, mean, _, _ = _pca()
    Y = ints(PCA_N, PCA_L, seed=24)
    Zt = Y.double().T @ (X.double() - mean.double())
    return case({"Y": Y, "X": X, "mean": mean, "Zt": spec_like(Zt)}, want=Zt)


KNN_NQ, KNN_NB, KNN_D, KNN_K = 70, 130, 20, 5                                         # 130 bank rows: three 64-column tiles


def make_knn_query():
    import knn_ref
    Q, X = ints(KNN_NQ, KNN_D, seed=25), ints(KNN_NB, KNN_D, seed=26)
    d2 = ((Q.double()[:, None, :] - X.double()[None, :, :]) ** 2).sum(-1)
    D32 = np.sqrt(d2.numpy().astype(np.float32))                                      # what the device computes, exactly
    idx, dist = knn_ref.topk(D32.astype(np.float64), KNN_K)
    return case({"Q": Q, "X": X, "idx": Spec((KNN_NQ, KNN_K), I64T), "dist": Spec((KNN_NQ, KNN_K), F32T)},
                idx=torch.from_numpy(idx), dist=torch.from_numpy(dist))


def check_knn_query(c, out):
    return exact("idx", out["idx"], c.idx) + exact("dist", out["dist"], c.dist)


def make_knn_ranks():
    import embedding_quality_ref as ER
    A = ints(KNN_NB, KNN_D, seed=27)
    D2 = ER.sq_distances(A.numpy())
    nbr = ER.neighbours(D2, KNN_K)
    less, tied = ER.counts(D2, nbr)
    return case({"A": A, "nbr": torch.from_numpy(nbr), "less": Spec((KNN_NB, KNN_K), I32T), "tied": Spec((KNN_NB, KNN_K), I32T)},
                less=torch.from_numpy(less), tied=torch.from_numpy(tied))


def check_knn_ranks(c, out):
    return exact("less", out["less"], c.less) + exact("tied", out["tied"], c.tied)


def make_silhouette():
    import silhouette_ref as SR
    N, C = KNN_NB, 5
    X = ints(N, KNN_D, seed=28)
    y = torch.randint(0, C, (N,), generator=torch.Generator().manual_seed(29))
    D32, M = SR.exact_euclidean32(X.numpy())
    S, want = SR.device_restatement(D32, y.numpy(), C, M, SR.EUCLIDEAN)
    return case({"X": X, "labels": y}, {"C": C}, S=S, want=want)


def check_silhouette(c, out):
    """test_silhouette_gpu.py::test_exact_on_integer_data: the fixed-point sums are the restatement's, sil / a / b within
    1e-15 of it, the integer outputs equal."""
    bad = []
    if not np.array_equal(out["sums"].numpy(), c.S):
        bad.append("sums differ from the restatement's")
    for k in ("sil", "a", "b"):
        err = float(np.nanmax(np.abs(out[k].numpy() - c.want[k])))
        if not err <= 1e-15:
            bad.append(f"{k}: {err:.3e} from the restatement")
    for k in ("nearest", "counts"):
        if not np.array_equal(out[k].numpy(), c.want[k]):
            bad.append(f"{k} differs")
    if float(out["score"][0]) != c.want["score"] or [int(v) for v in out["status"]] != c.want["status"]:
        bad.append("score or status differs")
    return bad


BS_N, BS_D, BS_K = 130, 52, 12


def make_som_batch_accumulate():
    X = ints(BS_N, BS_D, seed=30)
    bmu = torch.randint(0, BS_K, (BS_N,), generator=torch.Generator().manual_seed(31))
    sums = torch.zeros(BS_K, BS_D, dtype=F64T).index_add_(0, bmu, X.double())
    return case({"X": X, "bmu": bmu, "sums": Spec((BS_K, BS_D), F64T), "counts": Spec((BS_K,), I64T)},
                sums=sums, counts=torch.bincount(bmu, minlength=BS_K))


def check_som_batch_accumulate(c, out):
    return exact("sums", out["sums"], c.sums) + exact("counts", out["counts"], c.counts)


KM_N, KM_D, KM_K = 130, 52, 5


def make_kmeans_assign():
    X, C = ints(KM_N, KM_D, seed=34), ints(KM_K, KM_D, seed=35)
    d2 = ((X.double()[:, None, :] - C.double()[None, :, :]) ** 2).sum(-1)
    return case({"X": X, "centers": C, "labels": Spec((KM_N,), I64T), "prev_labels": torch.zeros(KM_N, dtype=I64T),
                 "mind": Spec((KM_N,), F32T)}, labels=d2.argmin(1), mind=d2.min(1).values)


def call_kmeans_assign(ops, t, a):
    X = t["X"]
    ws = torch.empty(ops.kmeans_workspace_bytes(KM_N, KM_D, KM_K), dtype=U8T, device=X.device)
    ops.kmeans_assign(X, t["centers"], t["labels"], t["prev_labels"], t["mind"], ws)


GM_N, GM_D, GM_K = 70, 52, 5                                                         # two 32-row steps and a ragged one


def make_gmm_estep():
    import gmm_ref as GR
    X, means, prec, w = GR.mixture_case(GM_N, GM_D, GM_K, "diag")
    prec = prec.astype(np.float32).astype(np.float64)                                 # the precisions as the kernel sees them
    logc = GR.logc64(w, prec, GM_D)
    ref = GR.estep64(X, means, prec, w)
    lpn32, resp32 = GR.estep32(X, means, prec, logc)
    t = {"X": torch.from_numpy(np.ascontiguousarray(X)).float(), "means": torch.from_numpy(np.ascontiguousarray(means)).float(),
         "prec": torch.from_numpy(prec).float(), "logc": torch.from_numpy(logc), "resp": Spec((GM_N, GM_K), F32T),
         "log_prob_norm": Spec((GM_N,), F64T), "labels": Spec((GM_N,), I64T), "estat": Spec((2,), F64T)}
    return case(t, ref=ref, e32=dict(lpn=GR.err(lpn32, ref["lpn"]), resp=GR.err(resp32, ref["resp"])))


def check_gmm_estep(c, out):
    """test_gmm_gpu.py's _check_estep: lpn and resp within max(FLOOR, 4 e32) relative to the largest reference value, labels
    equal where the fp64 top-two gap is clear, estat = (the sum of lpn, no refused row)."""
    import gmm_ref as GR
    bad = []
    for key, got in (("lpn", out["log_prob_norm"]), ("resp", out["resp"])):
        e_k, lim = GR.err(got.numpy(), c.ref[key]), GR.bound(GR.FLOOR, c.e32[key])
        print(f"ALIGN|gmm {key}|e32={c.e32[key]:.3e}|e_k={e_k:.3e}|bound={lim:.3e}")
        if not e_k <= lim:
            bad.append(f"{key}: error {e_k:.3e} > {lim:.3e}")
    if not c.e32["lpn"] <= GR.E32_MAX:
        bad.append("the yardstick itself is off")
    clear = c.ref["gap"] > GR.GAP
    if (~clear).mean() > GR.MAX_UNCLEAR or not np.array_equal(out["labels"].numpy()[clear], c.ref["labels"][clear]):
        bad.append("labels differ from the fp64 argmax where the gap is clear")
    lpn, estat = out["log_prob_norm"].numpy(), out["estat"].numpy()
    if estat[1] != 0 or abs(estat[0] - lpn.sum()) > 1e-12 * max(np.abs(lpn).sum(), 1.0):
        bad.append("estat is not (sum of log_prob_norm, 0)")
    return bad


def make_som_batch_update():
    import batch_som_ref as BR
    side = (4, 3)
    K, D = side[0] * side[1], BS_D
    rng = np.random.RandomState(36)
    counts = rng.randint(0, 9, K).astype(np.int64)
    counts[0] = 0                                                                     # a unit nobody hit
    sums = rng.standard_normal((K, D)) * counts[:, None]
    pos = BR.grid_positions(side[0], side[1], "square")
    sigma = 1.3
    return case({"sums": torch.from_numpy(sums), "counts": torch.from_numpy(counts), "grid_positions": torch.from_numpy(pos),
                 "W_out": Spec((K, D), F32T)}, {"sigma": sigma},
                ref=BR.update(sums, counts, pos, sigma), y32=BR.update(sums, counts, pos, sigma, dtype=np.float32))


def make_tsne_repulsion():
    N = 130
    Y = rnd(N, 2, seed=32)
    out = {}
    for key, dt in (("ref", F64T), ("y32", F32T)):
        y = Y.to(dt)
        diff = y[:, None, :] - y[None, :, :]
        q = 1 / (1 + (diff ** 2).sum(-1))
        q.fill_diagonal_(0)
        out[key] = {"rep": ((q * q)[:, :, None] * diff).sum(1), "sumq": q.sum(1)}
    return case({"Y": Y, "rep": Spec((N, 2), F64T), "sumq": Spec((N,), F64T), "zpart": Spec((math.ceil(N / 64),), F64T)},
                ref=out["ref"], y32=out["y32"])


def check_tsne_repulsion(c, out):
    """No floor of its own here: 4 x max(e32, 2^-23)."""
    bad = close_nofloor("rep", out["rep"], c.ref["rep"], c.y32["rep"]) + close_nofloor("sumq", out["sumq"], c.ref["sumq"], c.y32["sumq"])
    return bad + close_nofloor("zpart", out["zpart"].sum().reshape(1), c.ref["sumq"].sum().reshape(1), c.y32["sumq"].sum().reshape(1))


def make_umatrix():
    K, L, side = 12, 52, (4, 3)
    W = ints(K, L, seed=33)
    gy, gx = torch.meshgrid(torch.arange(side[0]), torch.arange(side[1]), indexing="ij")
    grid = torch.stack([gy.reshape(-1), gx.reshape(-1)], 1).float().contiguous()
    d = (W.double()[:, None, :] - W.double()[None, :, :]).abs().sum(-1)                # Manhattan: exact on integers
    g2 = ((grid.double()[:, None, :] - grid.double()[None, :, :]) ** 2).sum(-1)
    idx, dist = torch.full((K, 8), -1, dtype=I64T), torch.zeros(K, 8, dtype=F64T)
    for k in range(K):
        nb = [j for j in range(K) if j != k and g2[k, j] <= 1.0]
        idx[k, :len(nb)] = torch.tensor(nb)
        dist[k, :len(nb)] = d[k, nb]
    u = torch.tensor([float(dist[k][idx[k] >= 0].sum() / int((idx[k] >= 0).sum())) for k in range(K)], dtype=F64T)
    return case({"W": W, "grid_positions": grid}, {"adj_r2": 1.0}, idx=idx, dist=dist, u=u)


def check_umatrix(c, out):
    bad = exact("nbr_idx", out["nbr_idx"], c.idx) + exact("nbr_dist", out["nbr_dist"], c.dist)
    if not torch.equal(out["u"], c.u.float()):                                        # fp64 mean of exact terms, rounded once
        bad.append("u is not the correctly rounded mean")
    return bad


# ------------------------------------------------------------------------------------------------------- the calls
def _dist_code(ops, name):
    return {"euclidean": ops.DIST_EUCLIDEAN, "cosine": ops.DIST_COSINE, "manhattan": ops.DIST_MANHATTAN}[name]


def call_attention_fwd(ops, t, a):
    ops.attention_fwd(t["qkv"], t["out"], t["lse"], a["B"], a["N"], a["H"], a["hd"])


def call_attention_bwd(ops, t, a):
    ops.attention_bwd(t["qkv"], t["out"], t["dout"], t["lse"], t["dqkv"], t["delta"], a["B"], a["N"], a["H"], a["hd"])


def call_adamw(ops, t, a):
    hp = NE.ADAMW_HP
    ops.adamw_step(t["p"], t["g"], t["m"], t["v"], t["wd_chunk"], hp["lr"], hp["b1"], hp["b2"], hp["eps"], a["step"])


def call_silhouette(ops, t, a):
    ws = ops.silhouette_workspace(t["X"].shape[0], a["C"], t["X"].device)
    r = ops.silhouette(t["X"], t["labels"], ops.DIST_EUCLIDEAN, a["C"], ws=ws)
    return {"sil": r.sil, "a": r.a, "b": r.b, "nearest": r.nearest, "counts": r.counts, "cluster_mean": r.cluster_mean, "score": r.score,
            "sums": r.sums, "status": torch.tensor(r.status)}


def call_umatrix(ops, t, a):
    u, nbr_idx, nbr_dist = ops.umatrix(t["W"], t["grid_positions"], a["adj_r2"], ops.DIST_MANHATTAN)
    return {"u": u, "nbr_idx": nbr_idx, "nbr_dist": nbr_dist}


def call_planes_fwd(ops, t, a):
    """The plane images are made from aligned copies of the values: what is under test is the operand the finalize stage reads."""
    x, W = t["x"], t["W"]
    xp, wp = ops.bmu_planes_alloc(x.shape[0], x.shape[1], x.device), ops.bmu_planes_alloc(W.shape[0], W.shape[1], x.device)
    ops.bmu_planes_from(x.contiguous().clone(), xp)
    ops.bmu_planes_from(W.contiguous().clone(), wp)
    ops.bmu_cosine_x3_planes_fwd(x, W, xp, wp, t["dist"], t["bmu"], t["inv_nx"], t["inv_nw"])


def call_planes_from(ops, t, a):
    planes = ops.bmu_planes_alloc(a["R"], a["L"], t["src"].device)
    ops.bmu_planes_from(t["src"], planes)
    return {"planes": planes}


def check_planes_from(c, out):
    """The image is checked by the planes form of the BMU pass (bmu_cosine_x3_planes_fwd row, test_ops_gpu); here the
    squared-norm partials behind it: exact on integers."""
    R, L = c.a["R"], c.a["L"]
    img = 2 * math.ceil(L / 32) * math.ceil(R / 32) * 2048
    sq = out["planes"][img:img + math.ceil(L / 64) * R * 4].view(F32T).view(-1, R)
    return exact("squared-norm partials", sq.sum(0), (c.t["src"].double() ** 2).sum(1))


# ------------------------------------------------------------------------------------------------------- the table
def gemm_ops(a, b, *rest):
    """The two GEMM operands of launch_gemm (gemm_f32.hip:140-147): either one off the 16-byte grid clears `fast`, the
    element-wise kernel runs (and, in the split modes, the f32 engine: the split engine has no other form)."""
    return [a, b, *rest]


X_LD = dict(ld=True, shifted=ELEMENT, pitched=ELEMENT)
OUT_LD = dict(ld=True, shifted=SAME, pitched=SAME)
ALIGN = REFUSED(EALIGN)

ROWS = [
    # ---- launch_gemm: A and B choose the path; bias, R, rowscale and C are read / written one element at a time (gemm_epilogue)
    Row("linear_fwd", "linear_fwd", "vsom_linear_fwd", make_linear_fwd,
        lambda ops, t, a: ops.linear_fwd(t["x"], t["W"], t["bias"], t["out"]),
        gemm_ops(Op("x", F32T, IN, **X_LD), Op("W", F32T, IN, shifted=ELEMENT), Op("bias", F32T, IN), Op("out", F32T, OUT, **OUT_LD)),
        lambda c, out: exact("out", out["out"], c.pre), ALL_MODES, (LINEAR_FWD, (LIN_M, LIN_N, LIN_K))),
    Row("linear_gelu_fwd", "linear_gelu_fwd", "vsom_linear_gelu_fwd", make_linear_gelu_fwd,
        lambda ops, t, a: ops.linear_gelu_fwd(t["x"], t["W"], t["bias"], t["grad"], t["act"]),
        gemm_ops(Op("x", F32T, IN, **X_LD), Op("W", F32T, IN, shifted=ELEMENT), Op("bias", F32T, IN), Op("grad", F32T, OUT),
                 Op("act", F32T, OUT)),
        check_linear_gelu_fwd, ALL_MODES, (LINEAR_GELU_FWD, (LIN_M, LIN_N, LIN_K))),
    Row("linear_relu_fwd", "linear_relu_fwd", "vsom_linear_relu_fwd", make_linear_relu_fwd,
        lambda ops, t, a: ops.linear_relu_fwd(t["x"], t["W"], t["bias"], t["ygrad"], t["yact"]),
        gemm_ops(Op("x", F32T, IN, **X_LD), Op("W", F32T, IN, shifted=ELEMENT), Op("bias", F32T, IN), Op("ygrad", F32T, OUT),
                 Op("yact", F32T, OUT)),
        lambda c, out: exact("yact", out["yact"], c.pre.clamp_min(0)) + exact("ygrad", out["ygrad"], (c.pre > 0).double()),
        ALL_MODES, (LINEAR_RELU_FWD, (LIN_M, LIN_N, LIN_K))),
    Row("linear_residual_fwd", "linear_residual_fwd", "vsom_linear_residual_fwd", make_linear_residual_fwd,
        lambda ops, t, a: ops.linear_residual_fwd(t["x"], t["W"], t["bias"], t["R"], a["r_mod"], t["out"]),
        gemm_ops(Op("x", F32T, IN, **X_LD), Op("W", F32T, IN, shifted=ELEMENT), Op("bias", F32T, IN), Op("R", F32T, IN, **OUT_LD),
                 Op("out", F32T, OUT, **OUT_LD)),
        lambda c, out: exact("out", out["out"], c.pre), ALL_MODES, (LINEAR_RESIDUAL_FWD, (LIN_M, LIN_N, LIN_K))),
    Row("linear_bwd_input", "linear_bwd_input", "vsom_linear_bwd_input", make_linear_bwd_input,
        lambda ops, t, a: ops.linear_bwd_input(t["dy"], t["W"], t["dx"]),
        gemm_ops(Op("dy", F32T, IN, **X_LD), Op("W", F32T, IN, shifted=ELEMENT), Op("dx", F32T, OUT, **OUT_LD)),
        lambda c, out: exact("dx", out["dx"], c.dx), ALL_MODES, (BWD_INPUT, (LIN_M, LIN_K, LIN_N - 2))),
    Row("linear_bwd_input_t", "linear_bwd_input_t", "vsom_linear_bwd_input_t", make_linear_bwd_input_t,
        lambda ops, t, a: ops.linear_bwd_input_t(t["dy"], t["Wt"], t["dx"]),
        gemm_ops(Op("dy", F32T, IN, **X_LD), Op("Wt", F32T, IN, shifted=ELEMENT), Op("dx", F32T, OUT, **OUT_LD)),
        lambda c, out: exact("dx", out["dx"], c.dx), ALL_MODES, (BWD_INPUT_T, (LIN_M, LIN_K, LIN_N - 2))),
    # gemm_f32.hip:388 (`vec`) decides the tile kernels, which this shape does not select (the -tiles row does); the generic
    # GEMM behind it takes launch_gemm's choice.  dW and db leave through reduce_slabs_body, which tests each destination in the kernel (gemm_f32.h:620)
    Row("linear_bwd_weight", "linear_bwd_weight", "vsom_linear_bwd_weight", make_linear_bwd_weight(),
        lambda ops, t, a: ops.linear_bwd_weight(t["dy"], t["x"], t["dW"], t["db"]),
        gemm_ops(Op("dy", F32T, IN, **X_LD), Op("x", F32T, IN, **X_LD), Op("dW", F32T, OUT), Op("db", F32T, OUT)),
        lambda c, out: exact("dW", out["dW"], c.dW) + exact("db", out["db"], c.db), ALL_MODES, (BWD_WEIGHT, (LIN_M, 68, LIN_K))),
    # the smallest shape of the 192 x 64 weight-gradient tiles (launch_plan_rows: wgrad.192x64): gemm_f32.hip:388 sends a misaligned
    # dY or X to the generic GEMM above instead
    Row("linear_bwd_weight-tiles", "linear_bwd_weight", "vsom_linear_bwd_weight", make_linear_bwd_weight(256, 192, 64),
        lambda ops, t, a: ops.linear_bwd_weight(t["dy"], t["x"], t["dW"], t["db"]),
        gemm_ops(Op("dy", F32T, IN, **X_LD), Op("x", F32T, IN, **X_LD), Op("dW", F32T, OUT), Op("db", F32T, OUT)),
        lambda c, out: exact("dW", out["dW"], c.dW) + exact("db", out["db"], c.db), ALL_MODES, (BWD_WEIGHT, (256, 192, 64))),
    Row("som_bwd", "som_bwd", "vsom_som_bwd", make_som_bwd,
        lambda ops, t, a: ops.som_bwd(t["x"], t["W"], t["coef"], t["row_dot"], t["col_dot"], t["gW"], t["gX"], accumulate_gx=False),
        gemm_ops(Op("x", F32T, IN, **X_LD), Op("W", F32T, IN, shifted=ELEMENT), Op("coef", F32T, IN, shifted=ELEMENT),
                 Op("row_dot", F32T, IN), Op("col_dot", F32T, IN), Op("gW", F32T, OUT), Op("gX", F32T, OUT, **OUT_LD)),
        lambda c, out: exact("gW", out["gW"], c.gW) + exact("gX", out["gX"], c.gX), ALL_MODES, (SOM_BWD_GW, (SOM_B, SOM_K, SOM_L))),
    Row("bmu_euclid_fwd-70x15x256", "bmu_euclid_fwd", "vsom_bmu_euclid_fwd", make_bmu_euclid(70, 15, 256),
        lambda ops, t, a: ops.bmu_euclid_fwd(t["x"], t["W"], t["sq_x"], t["sq_w"], t["dist"], t["bmu"]),
        gemm_ops(Op("x", F32T, IN, **X_LD), Op("W", F32T, IN, shifted=ELEMENT), Op("sq_x", F32T, IN), Op("sq_w", F32T, IN),
                 Op("dist", F32T, OUT), Op("bmu", I64T, OUT)),
        check_dist_bmu, ALL_MODES, (BMU_COSINE_DOTS, (70, 15, 256))),
    Row("bmu_euclid_fwd-33x100x48", "bmu_euclid_fwd", "vsom_bmu_euclid_fwd", make_bmu_euclid(33, 100, 48),
        lambda ops, t, a: ops.bmu_euclid_fwd(t["x"], t["W"], t["sq_x"], t["sq_w"], t["dist"], t["bmu"]),
        gemm_ops(Op("x", F32T, IN, **X_LD), Op("W", F32T, IN, shifted=ELEMENT), Op("sq_x", F32T, IN), Op("sq_w", F32T, IN),
                 Op("dist", F32T, OUT), Op("bmu", I64T, OUT)),
        check_dist_bmu, ALL_MODES, (BMU_COSINE_DOTS, (33, 100, 48))),
    Row("bmu_cosine_fwd-70x15x256", "bmu_cosine_fwd", "vsom_bmu_cosine_dots + vsom_bmu_cosine_finalize", make_bmu_cosine_exact(70, 15, 256),
        lambda ops, t, a: ops.bmu_cosine_fwd(t["x"], t["W"], t["inv_nx"], t["inv_nw"], t["dist"], t["bmu"]),
        gemm_ops(Op("x", F32T, IN, **X_LD), Op("W", F32T, IN, shifted=ELEMENT), Op("inv_nx", F32T, IN), Op("inv_nw", F32T, IN),
                 Op("dist", F32T, OUT), Op("bmu", I64T, OUT)),
        check_bmu_cosine_exact, ALL_MODES, (BMU_COSINE_DOTS, (70, 15, 256))),
    Row("bmu_cosine_fwd-33x100x48", "bmu_cosine_fwd", "vsom_bmu_cosine_dots + vsom_bmu_cosine_finalize", make_bmu_cosine_exact(33, 100, 48),
        lambda ops, t, a: ops.bmu_cosine_fwd(t["x"], t["W"], t["inv_nx"], t["inv_nw"], t["dist"], t["bmu"]),
        gemm_ops(Op("x", F32T, IN, **X_LD), Op("W", F32T, IN, shifted=ELEMENT), Op("inv_nx", F32T, IN), Op("inv_nw", F32T, IN),
                 Op("dist", F32T, OUT), Op("bmu", I64T, OUT)),
        check_bmu_cosine_exact, ALL_MODES, (BMU_COSINE_DOTS, (33, 100, 48))),
    # the patch matrix xp_ws is written by the gather and is then the GEMM's A; bias, position rows and the mapped output rows
    # are element accesses
    Row("patch_embed_fwd", "patch_embed_fwd", "vsom_patch_embed_fwd", make_patch_embed_fwd,
        lambda ops, t, a: ops.patch_embed_fwd(t["img"], t["Wpe"], t["bpe"], t["pos"], t["cls_token"], t["tokens"], t["xp_ws"], a["p"]),
        gemm_ops(Op("xp_ws", F32T, OUT, shifted=ELEMENT), Op("Wpe", F32T, IN, shifted=ELEMENT), Op("img", F32T, IN), Op("bpe", F32T, IN),
                 Op("pos", F32T, IN), Op("cls_token", F32T, IN), Op("tokens", F32T, OUT)),
        lambda c, out: exact("tokens", out["tokens"], c.tokens) + exact("xp_ws", out["xp_ws"], c.xp), ALL_MODES,
        (LINEAR_RESIDUAL_FWD, (PE["B"] * 16, PE["E"], 12))),
    # ---- reduce_slabs2_internal (gemm_f32.hip:195): the slabs and their stride; the destination is tested in the kernel
    Row("reduce_slabs", "reduce_slabs", "vsom_reduce_slabs", make_reduce_slabs,
        lambda ops, t, a: ops.reduce_slabs(t["slabs"], t["out"]),
        [Op("slabs", F32T, IN, **X_LD), Op("out", F32T, OUT)], lambda c, out: exact("out", out["out"], c.want)),
    # ---- the three-product cosine BMU forms (bmu_x3.hip): no element-wise form; the caller falls back to bmu_cosine_fwd
    Row("bmu_cosine_x3_fwd-70x15x256", "bmu_cosine_x3_fwd", "vsom_bmu_cosine_x3_dots + vsom_bmu_cosine_x3_finalize",
        make_bmu_cosine(70, 15, 256),
        lambda ops, t, a: ops.bmu_cosine_x3_fwd(t["x"], t["W"], t["dist"], t["bmu"], t["inv_nx"], t["inv_nw"]),
        [Op("x", F32T, IN, ld=True, shifted=ALIGN, pitched=ALIGN), Op("W", F32T, IN, shifted=ALIGN), Op("dist", F32T, OUT),
         Op("bmu", I64T, OUT), Op("inv_nx", F32T, OUT), Op("inv_nw", F32T, OUT)],
        check_bmu_cosine(1e-5)),                                                       # test_bmu_cosine_x3_rerank
    Row("bmu_cosine_x3_fwd-33x100x48", "bmu_cosine_x3_fwd", "vsom_bmu_cosine_x3_dots + vsom_bmu_cosine_x3_finalize",
        make_bmu_cosine(33, 100, 48),
        lambda ops, t, a: ops.bmu_cosine_x3_fwd(t["x"], t["W"], t["dist"], t["bmu"], t["inv_nx"], t["inv_nw"]),
        [Op("x", F32T, IN, ld=True, shifted=ALIGN, pitched=ALIGN), Op("W", F32T, IN, shifted=ALIGN), Op("dist", F32T, OUT),
         Op("bmu", I64T, OUT), Op("inv_nx", F32T, OUT), Op("inv_nw", F32T, OUT)],
        check_bmu_cosine(1e-5)),
    # x and W reach vsom_bmu_cosine_x3_planes_finalize only (the re-rank), which answers VSOM_EALIGN; a pitch that is no
    # multiple of 4 is outside the form's plan: VSOM_EINVAL
    Row("bmu_cosine_x3_planes_fwd-192x15x256", "bmu_cosine_x3_planes_fwd", "vsom_bmu_cosine_x3_planes_dots + vsom_bmu_cosine_x3_planes_finalize",
        make_bmu_cosine(192, 15, 256), call_planes_fwd,
        [Op("x", F32T, IN, ld=True, shifted=ALIGN, pitched=REFUSED(EINVAL)), Op("W", F32T, IN, shifted=ALIGN), Op("dist", F32T, OUT),
         Op("bmu", I64T, OUT), Op("inv_nx", F32T, OUT), Op("inv_nw", F32T, OUT)],
        check_bmu_cosine(1e-5)),
    Row("bmu_planes_from", "bmu_planes_from", "vsom_bmu_planes_from", make_planes_from, call_planes_from,
        [Op("src", F32T, IN, ld=True, shifted=REFUSED(EINVAL), pitched=REFUSED(EINVAL))], check_planes_from),
    # ---- gemm_f32.hip:334: the LayerNorm-fused input gradient has the 16-byte kernels only (split modes; three planes here)
    Row("linear_bwd_input_ln", "linear_bwd_input_ln", "vsom_linear_bwd_input_ln", make_linear_bwd_input_ln,
        lambda ops, t, a: ops.linear_bwd_input_ln(t["dy"], t["Wt"], t["x"], t["mean"], t["rstd"], t["gamma"], None, t["dx"],
                                                  t["dgamma"], t["dbeta"]),
        [Op("dy", F32T, IN, ld=True, shifted=ALIGN, pitched=ALIGN), Op("Wt", F32T, IN, shifted=ALIGN), Op("x", F32T, IN, shifted=ALIGN),
         Op("mean", F32T, IN), Op("rstd", F32T, IN), Op("gamma", F32T, IN, shifted=ALIGN), Op("dx", F32T, OUT, shifted=ALIGN),
         Op("dgamma", F32T, OUT), Op("dbeta", F32T, OUT)], check_linear_bwd_input_ln, (SPLIT,)),
    # ---- misc.hip: the batched transpose moves single elements through LDS: nothing to choose
    Row("transpose_many", "transpose_many", "vsom_transpose_many", make_transpose_many,
        lambda ops, t, a: ops.transpose_many(t["src_base"], t["dst_base"], t["table"], a["max_rows"], a["max_cols"]),
        [Op("src_base", F32T, IN), Op("dst_base", F32T, OUT), Op("table", I64T, IN)], lambda c, out: exact("dst", out["dst_base"], c.want)),
    # ---- som.hip:256,268
    Row("row_inv_norm", "row_inv_norm", "vsom_row_inv_norm", make_row_norm(70, 52, False),
        lambda ops, t, a: ops.row_inv_norm(t["x"], t["out"]),
        [Op("x", F32T, IN, **X_LD), Op("out", F32T, OUT)],
        lambda c, out: close("inv_norm", out["out"], c.ref, c.y32, 2e-6, rel_err)),    # 2e-6 relative (test_bmu_cosine)
    Row("row_sqnorm", "row_sqnorm", "vsom_row_sqnorm", make_row_norm(70, 52, True),
        lambda ops, t, a: ops.row_sqnorm(t["x"], t["out"]),
        [Op("x", F32T, IN, **X_LD), Op("out", F32T, OUT)], lambda c, out: exact("sqnorm", out["out"], c.ref)),
    # ---- som_l1.hip:230,240: one kernel, the width of each operand's loads a flag of its own
    Row("bmu_manhattan_fwd-70x15x256", "bmu_manhattan_fwd", "vsom_bmu_manhattan_fwd", make_bmu_manhattan(70, 15, 256),
        lambda ops, t, a: ops.bmu_manhattan_fwd(t["x"], t["W"], t["dist"], t["bmu"]),
        [Op("x", F32T, IN, **X_LD), Op("W", F32T, IN, shifted=ELEMENT), Op("dist", F32T, OUT), Op("bmu", I64T, OUT)], check_dist_bmu),
    Row("bmu_manhattan_fwd-33x100x48", "bmu_manhattan_fwd", "vsom_bmu_manhattan_fwd", make_bmu_manhattan(33, 100, 48),
        lambda ops, t, a: ops.bmu_manhattan_fwd(t["x"], t["W"], t["dist"], t["bmu"]),
        [Op("x", F32T, IN, **X_LD), Op("W", F32T, IN, shifted=ELEMENT), Op("dist", F32T, OUT), Op("bmu", I64T, OUT)], check_dist_bmu),
    Row("som_bwd_manhattan", "som_bwd_manhattan", "vsom_som_bwd_manhattan", make_som_bwd_manhattan,
        lambda ops, t, a: ops.som_bwd_manhattan(t["x"], t["W"], t["coef"], t["gW"], t["gX"], accumulate_gx=False),
        [Op("x", F32T, IN, **X_LD), Op("W", F32T, IN, shifted=ELEMENT), Op("coef", F32T, IN, shifted=ELEMENT), Op("gW", F32T, OUT),
         Op("gX", F32T, OUT, **OUT_LD)],
        lambda c, out: exact("gW", out["gW"], c.gW) + exact("gX", out["gX"], c.gX)),
    # ---- som.hip's loss kernels read and write one element at a time: nothing to choose
    Row("som_neigh_loss", "som_neigh_loss", "vsom_som_neigh_loss", make_som_neigh_loss,
        lambda ops, t, a: ops.som_neigh_loss(t["dist"], t["bmu"], t["grid"], a["T"], t["loss_sum"], h=t["h"]),
        [Op("dist", F32T, IN), Op("bmu", I64T, IN), Op("grid", F32T, IN), Op("loss_sum", F32T, OUT), Op("h", F32T, OUT)],
        check_som_neigh_loss),
    Row("cross_entropy_ls", "cross_entropy_ls", "vsom_cross_entropy_ls", make_cross_entropy,
        lambda ops, t, a: ops.cross_entropy_ls(t["logits"], t["y"], 0.1, t["loss_sum"], dlogits=t["dlogits"], grad_scale=1.0),
        [Op("logits", F32T, IN), Op("y", I64T, IN), Op("loss_sum", F32T, OUT), Op("dlogits", F32T, OUT)], check_cross_entropy),
]

# ---- layernorm.hip:254,280: X, Y, gamma, beta (forward) and dY, X, gamma, dX, resid (backward) select the 16-byte kernel;
# mean / rstd are one element per row, dgamma / dbeta leave through reduce_slabs_body
for _cols in (16, 96, 192):
    ROWS.append(Row(f"layernorm_fwd-{_cols}", "layernorm_fwd", "vsom_layernorm_fwd", make_layernorm(_cols, False),
                    lambda ops, t, a: ops.layernorm_fwd(t["x"], t["gamma"], t["beta"], t["y"], t["mean"], t["rstd"], NE.LN_EPS),
                    [Op("x", F32T, IN, shifted=ELEMENT), Op("gamma", F32T, IN, shifted=ELEMENT), Op("beta", F32T, IN, shifted=ELEMENT),
                     Op("y", F32T, OUT, shifted=ELEMENT), Op("mean", F32T, OUT), Op("rstd", F32T, OUT)], check_layernorm_fwd))
    ROWS.append(Row(f"layernorm_bwd-{_cols}", "layernorm_bwd", "vsom_layernorm_bwd", make_layernorm(_cols, True),
                    lambda ops, t, a: ops.layernorm_bwd(t["dy"], t["x"], t["mean"], t["rstd"], t["gamma"], t["resid"], t["dx"],
                                                        t["dgamma"], t["dbeta"]),
                    [Op("dy", F32T, IN, shifted=ELEMENT), Op("x", F32T, IN, shifted=ELEMENT), Op("mean", F32T, IN), Op("rstd", F32T, IN),
                     Op("gamma", F32T, IN, shifted=ELEMENT), Op("resid", F32T, IN, shifted=ELEMENT), Op("dx", F32T, OUT, shifted=ELEMENT),
                     Op("dgamma", F32T, OUT), Op("dbeta", F32T, OUT)], check_layernorm_bwd))

# ---- attention.hip:1469,1485: the vector kernels (hd = 16, 32, 64) refuse, the scalar ones (hd <= 8) have no requirement
for _N, _hd in ((17, 16), (65, 64), (17, 8), (65, 3)):
    _b = ALIGN if _hd % 16 == 0 else SAME
    ROWS.append(Row(f"attention_fwd-N{_N}-hd{_hd}", "attention_fwd", "vsom_attention_fwd", make_attention(_N, _hd, False), call_attention_fwd,
                    [Op("qkv", F32T, IN, shifted=_b), Op("out", F32T, OUT, shifted=_b), Op("lse", F32T, OUT)], check_attention_fwd))
    ROWS.append(Row(f"attention_bwd-N{_N}-hd{_hd}", "attention_bwd", "vsom_attention_bwd", make_attention(_N, _hd, True), call_attention_bwd,
                    [Op("qkv", F32T, IN, shifted=_b), Op("out", F32T, IN, shifted=_b), Op("dout", F32T, IN, shifted=_b), Op("lse", F32T, IN),
                     Op("dqkv", F32T, OUT, shifted=_b), Op("delta", F32T, OUT)], check_attention_bwd, (SPLIT,)))

ROWS += [
    # ---- attention_q1.hip:161,178 (o is refused by the forward although the kernel writes it one element at a time)
    Row("attention_q1_fwd", "attention_q1_fwd", "vsom_attention_q1_fwd", make_q1(False),
        lambda ops, t, a: ops.attention_q1_fwd(t["q"], t["kv"], t["out"], t["lse"], a["B"], a["N"], a["H"], a["hd"]),
        [Op("q", F32T, IN, shifted=ALIGN), Op("kv", F32T, IN, shifted=ALIGN), Op("out", F32T, OUT, shifted=ALIGN), Op("lse", F32T, OUT)],
        check_q1(("out", "lse"))),
    Row("attention_q1_bwd", "attention_q1_bwd", "vsom_attention_q1_bwd", make_q1(True),
        lambda ops, t, a: ops.attention_q1_bwd(t["dout"], t["out"], t["lse"], t["q"], t["kv"], t["dq"], t["dkv"], a["B"], a["N"], a["H"], a["hd"]),
        [Op("dout", F32T, IN, shifted=ALIGN), Op("out", F32T, IN, shifted=ALIGN), Op("lse", F32T, IN), Op("q", F32T, IN, shifted=ALIGN),
         Op("kv", F32T, IN, shifted=ALIGN), Op("dq", F32T, OUT), Op("dkv", F32T, OUT, shifted=ALIGN)], check_q1(("dq", "dkv"))),
    # ---- misc.hip:396
    Row("adamw_step", "adamw_step", "vsom_adamw_step", make_adamw, call_adamw,
        [Op("p", F32T, INOUT, shifted=ALIGN), Op("g", F32T, IN, shifted=ALIGN), Op("m", F32T, INOUT, shifted=ALIGN),
         Op("v", F32T, INOUT, shifted=ALIGN), Op("wd_chunk", F32T, IN)], check_adamw),
    # ---- bmu_x3.hip (adamw_step_planes): the same refusal, the arena walk of adamw_step plus the slice's image
    Row("adamw_step_planes", "adamw_step", "vsom_adamw_step_planes", make_adamw, call_adamw_planes,
        [Op("p", F32T, INOUT, shifted=ALIGN), Op("g", F32T, IN, shifted=ALIGN), Op("m", F32T, INOUT, shifted=ALIGN),
         Op("v", F32T, INOUT, shifted=ALIGN), Op("wd_chunk", F32T, IN)], check_adamw),
    # ---- pca.hip:236-246: X, B (Y) and the mean; scale and the output go through pca_reduce_kernel, element by element
    Row("pca_project", "pca_project", "vsom_pca_project", make_pca_project,
        lambda ops, t, a: ops.pca_project(t["X"], t["mean"], t["B"], t["scale"], t["Y"]),
        [Op("X", F32T, IN, **X_LD), Op("mean", F32T, IN, shifted=ELEMENT), Op("B", F32T, IN, **X_LD), Op("scale", F32T, IN),
         Op("Y", F32T, OUT, **OUT_LD)], lambda c, out: exact("Y", out["Y"], c.want)),
    Row("pca_backproject", "pca_backproject", "vsom_pca_backproject", make_pca_backproject,
        lambda ops, t, a: ops.pca_backproject(t["Y"], t["X"], t["mean"], t["Zt"]),
        [Op("Y", F32T, IN, **X_LD), Op("X", F32T, IN, **X_LD), Op("mean", F32T, IN, shifted=ELEMENT), Op("Zt", F32T, OUT, **OUT_LD)],
        lambda c, out: exact("Zt", out["Zt"], c.want)),
    # ---- knn.hip:333,1042,1082: the operands of the tile contraction; lists, labels and counters are element accesses
    Row("knn_query", "knn_query", "vsom_knn_query", make_knn_query,
        lambda ops, t, a: ops.knn_query(t["Q"], t["X"], KNN_K, ops.DIST_EUCLIDEAN, t["idx"], t["dist"]),
        [Op("Q", F32T, IN, **X_LD), Op("X", F32T, IN, **X_LD), Op("idx", I64T, OUT), Op("dist", F32T, OUT)], check_knn_query),
    Row("knn_ranks", "knn_ranks", "vsom_knn_ranks", make_knn_ranks,
        lambda ops, t, a: ops.knn_ranks(t["A"], t["nbr"], ops.DIST_EUCLIDEAN, t["less"], t["tied"]),
        [Op("A", F32T, IN, **X_LD), Op("nbr", I64T, IN), Op("less", I32T, OUT), Op("tied", I32T, OUT)], check_knn_ranks),
    Row("silhouette", "silhouette", "vsom_silhouette", make_silhouette, call_silhouette,
        [Op("X", F32T, IN, **X_LD), Op("labels", I64T, IN)], check_silhouette),
    # ---- batch_som.hip:388 (421, the update's fp64 sums: test_batch_som_gpu.py runs it on the sums this call leaves)
    Row("som_batch_accumulate", "som_batch_accumulate", "vsom_som_batch_accumulate", make_som_batch_accumulate,
        lambda ops, t, a: ops.som_batch_accumulate(t["X"], t["bmu"], t["sums"], t["counts"]),
        [Op("X", F32T, IN, **X_LD), Op("bmu", I64T, IN), Op("sums", F64T, OUT), Op("counts", I64T, OUT)], check_som_batch_accumulate),
    # batch_som.hip:421: the fp64 sums choose the update's kernel; one element (8 bytes) leaves the 16-byte grid, two do not
    Row("som_batch_update", "som_batch_update", "vsom_som_batch_update", make_som_batch_update,
        lambda ops, t, a: ops.som_batch_update(t["sums"], t["counts"], t["grid_positions"], a["sigma"], t["W_out"]),
        [Op("sums", F64T, IN, shifted=ELEMENT), Op("counts", I64T, IN), Op("grid_positions", F32T, IN), Op("W_out", F32T, OUT, **OUT_LD)],
        lambda c, out: close_nofloor("W", out["W_out"], c.ref, c.y32)),
    # ---- kmeans.hip:423 (also test_kmeans_gpu.py's unaligned rows, against sklearn's iteration)
    Row("kmeans_assign", "kmeans_assign", "vsom_kmeans_assign", make_kmeans_assign, call_kmeans_assign,
        [Op("X", F32T, IN, **X_LD), Op("centers", F32T, IN, shifted=ELEMENT), Op("labels", I64T, OUT), Op("prev_labels", I64T, IN),
         Op("mind", F32T, OUT)], lambda c, out: exact("labels", out["labels"], c.labels) + exact("mind", out["mind"], c.mind)),
    # ---- gmm.hip:401: X, means and precisions go through row_tile_pass's loads; logc, the staging rows, resp (ldr),
    # log_prob_norm, labels and estat are element accesses of the kernel's second half
    Row("gmm_estep", "gmm_estep", "vsom_gmm_estep", make_gmm_estep,
        lambda ops, t, a: ops.gmm_estep(t["X"], t["means"], t["prec"], t["logc"], t["resp"], t["log_prob_norm"], t["labels"], t["estat"]),
        [Op("X", F32T, IN, **X_LD), Op("means", F32T, IN, shifted=ELEMENT), Op("prec", F32T, IN, shifted=ELEMENT), Op("logc", F64T, IN),
         Op("resp", F32T, OUT, **OUT_LD), Op("log_prob_norm", F64T, OUT), Op("labels", I64T, OUT), Op("estat", F64T, OUT)],
        check_gmm_estep),
    # ---- tsne.hip:316: Y is read as float2, the entry asks for 16 bytes
    Row("tsne_repulsion", "tsne_repulsion", "vsom_tsne_repulsion", make_tsne_repulsion,
        lambda ops, t, a: ops.tsne_repulsion(t["Y"], t["rep"], t["sumq"], t["zpart"]),
        [Op("Y", F32T, IN, shifted=ALIGN), Op("rep", F64T, OUT), Op("sumq", F64T, OUT), Op("zpart", F64T, OUT)], check_tsne_repulsion),
    # ---- mapquality.hip:258
    Row("umatrix", "umatrix", "vsom_umatrix", make_umatrix, call_umatrix,
        [Op("W", F32T, IN, shifted=ELEMENT), Op("grid_positions", F32T, IN)], check_umatrix),
]

ROW_BY_ID = {r.id: r for r in ROWS}
assert len(ROW_BY_ID) == len(ROWS)


def rows_of(wrapper):
    return [r.id for r in ROWS if r.wrapper == wrapper]


# ------------------------------------------------------------------------------------------------------- the sites
# One alignment test in the sources: `aligned16(` or a pointer masked with 15 / 7 / 3
SITE = re.compile(r"aligned16\(|uintptr_t>?\)?\s*\(?\w+\)?\s*&\s*(?:15|7|3)u?\b|\(img & 15\)")

# Reasons for what no row of the table crosses
LEFT_OUT = {
    "definition": "common.h defines aligned16",
    "workspace": "a workspace, partial, slab or plane buffer the caller sizes by a query: test_memory_contract_cpu.py "
                 "(test_a_workspace_one_byte_short_is_refused_before_any_launch, P + 8) and the COVERED_ELSEWHERE tests it names; "
                 "the GPU rows keep every workspace aligned",
    "in-kernel": "the kernel tests the address in the expression that chooses the access: host and kernel cannot disagree",
    "agglomerative": "test_agglomerative_gpu.py: the 'offset' variant",
    "map_stats": "test_mapquality_gpu.py::test_map_stats_crafted_rows_and_unaligned_base",
    "proto_mosaic": "test_mapviz_gpu.py::test_proto_mosaic_unaligned_pred",
    "planes-dots": "vsom_bmu_cosine_x3_planes_dots refuses misaligned plane images: called on the host by test_alignment_cpu.py; "
                   "the refusal is host arithmetic on the two pointers and nothing is launched before it, so there are no outputs to inspect",
    "pipeline": "the data pipeline's plan / batch entries: the ops wrappers pass the caller's params, ra, out, out_u8 and scratch "
                "straight through, and the entries refuse on the host before any launch; test_alignment_cpu.py calls every one of "
                "these refusals with stand-in pointers.  No GPU row: an aligned call's check would be the PIL byte comparison of "
                "test_data_gpu.py / test_randaug_gpu.py / test_ragged_gpu.py over again",
}

# file -> [(text the source line contains, alignment tests on that line, row ids that cross it or a LEFT_OUT key)]
SITES = {
    "common.h": [("inline bool aligned16(const void* p)", 2, "definition")],
    "gemm_f32.hip": [
        ("g.a_vec = aligned16(g.A)", 1, ["linear_fwd", "linear_gelu_fwd", "linear_relu_fwd", "linear_residual_fwd", "linear_bwd_input",
                                         "linear_bwd_input_t", "linear_bwd_weight", "linear_bwd_weight-tiles", "patch_embed_fwd", "som_bwd", "bmu_euclid_fwd-70x15x256",
                                         "bmu_euclid_fwd-33x100x48", "bmu_cosine_fwd-70x15x256", "bmu_cosine_fwd-33x100x48"]),
        ("g.b_vec = aligned16(g.B)", 1, ["linear_fwd", "linear_gelu_fwd", "linear_relu_fwd", "linear_residual_fwd", "linear_bwd_input",
                                         "linear_bwd_input_t", "linear_bwd_weight", "linear_bwd_weight-tiles", "patch_embed_fwd", "som_bwd", "bmu_euclid_fwd-70x15x256",
                                         "bmu_euclid_fwd-33x100x48", "bmu_cosine_fwd-70x15x256", "bmu_cosine_fwd-33x100x48"]),
        ("const int vec = aligned16(slabs)", 1, ["reduce_slabs"]),
        ("VSOM_REQUIRE(aligned16(dY) && aligned16(Wt) && aligned16(X) && aligned16(gamma) && aligned16(dX) &&", 5, ["linear_bwd_input_ln"]),
        ("(!resid || aligned16(resid)) && lddy % 4 == 0 && N % 4 == 0, VSOM_EALIGN,", 1, ["linear_bwd_input_ln"]),
        ("VSOM_REQUIRE(part && aligned16(part) && part_bytes >= (size_t)p.parts", 1, "workspace"),
        ('VSOM_REQUIRE(aligned16(ws), VSOM_EALIGN, "linear_bwd_weight', 1, "workspace"),
        ("const bool vec = aligned16(dY) && aligned16(X) && lddy % 4 == 0", 2, ["linear_bwd_weight-tiles"]),
    ],
    "gemm_f32.h": [("(reinterpret_cast<uintptr_t>(dst) & 15u) == 0", 1, ["reduce_slabs", "linear_bwd_weight", "linear_bwd_weight-tiles"])],
    "layernorm.hip": [
        ("const int vec = ((reinterpret_cast<uintptr_t>(part) & 15u) == 0)", 1, "in-kernel"),
        ("if (cols % 4 == 0 && cols <= 256 && aligned16(X) && aligned16(Y) && aligned16(gamma) && aligned16(beta))", 4,
         ["layernorm_fwd-16", "layernorm_fwd-96", "layernorm_fwd-192"]),
        ("const bool v4 = cols % 4 == 0 && cols <= 256 && aligned16(dY) && aligned16(X) && aligned16(gamma) && aligned16(dX) &&", 4,
         ["layernorm_bwd-16", "layernorm_bwd-96", "layernorm_bwd-192"]),
        ("(!resid || aligned16(resid));", 1, ["layernorm_bwd-16", "layernorm_bwd-96", "layernorm_bwd-192"]),
        ('VSOM_REQUIRE(aligned16(ws), VSOM_EALIGN, "layernorm_bwd', 1, "workspace"),
        ("VSOM_REQUIRE(part && aligned16(part) && part_bytes >= vsom_layernorm_bwd_workspace_bytes", 1, "workspace"),
    ],
    "som.hip": [("const int vec = aligned16(X) && (ldx % 4 == 0);", 1, ["row_inv_norm", "row_sqnorm"])] * 2,
    "som_l1.hip": [
        ("per, (int)(aligned16(X) && ldx % 4 == 0), (int)(aligned16(W) && L % 4 == 0));", 2,
         ["bmu_manhattan_fwd-70x15x256", "bmu_manhattan_fwd-33x100x48"]),
        ("const int vx = aligned16(X) && ldx % 4 == 0, vw = aligned16(W) && L % 4 == 0, vc = aligned16(coef)", 3, ["som_bwd_manhattan"]),
    ],
    "tsne.hip": [("VSOM_REQUIRE(aligned16(Y), VSOM_EALIGN", 1, ["tsne_repulsion"])],
    "misc.hip": [("VSOM_REQUIRE(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v), VSOM_EALIGN", 4, ["adamw_step"])],
    "attention_q1.hip": [
        ("VSOM_REQUIRE(aligned16(q) && aligned16(kv) && aligned16(o), VSOM_EALIGN", 3, ["attention_q1_fwd"]),
        ("VSOM_REQUIRE(aligned16(dout) && aligned16(o) && aligned16(q) && aligned16(kv) && aligned16(dkv), VSOM_EALIGN", 5,
         ["attention_q1_bwd"]),
    ],
    "attention.hip": [
        ("VSOM_REQUIRE(hdp % 16 != 0 || (aligned16(qkv) && aligned16(out)), VSOM_EALIGN", 2, rows_of("attention_fwd")),
        ("VSOM_REQUIRE(hdp % 16 != 0 || (aligned16(qkv) && aligned16(out) && aligned16(dout) && aligned16(dqkv)), VSOM_EALIGN", 4,
         rows_of("attention_bwd")),
    ],
    "augment.hip": [
        ("if ((img & 15) == 0 && ((uintptr_t)src & 15) == 0) {", 2, "in-kernel"),
        ("if ((img & 15) == 0 && ((uintptr_t)src & 15) == 0) {", 2, "in-kernel"),
        ('VSOM_REQUIRE(vsom::aligned16(params), VSOM_EALIGN, "augment_plan', 1, "pipeline"),
        ("VSOM_REQUIRE(vsom::aligned16(out) && (!params || vsom::aligned16(params)) && ((uintptr_t)out_u8 & 3) == 0, VSOM_EALIGN", 3, "pipeline"),
        ('VSOM_REQUIRE(vsom::aligned16(ra), VSOM_EALIGN, "randaug_plan', 1, "pipeline"),
        ("VSOM_REQUIRE(vsom::aligned16(out) && vsom::aligned16(params) && vsom::aligned16(ra) && ((uintptr_t)out_u8 & 3) == 0", 4, "pipeline"),
    ],
    "augment_ragged.hip": [
        ("VSOM_REQUIRE(vsom::aligned16(params) && ((uintptr_t)shapes & 3) == 0, VSOM_EALIGN", 2, "pipeline"),
        ("VSOM_REQUIRE(vsom::aligned16(data) && vsom::aligned16(out) && (!params || vsom::aligned16(params)) &&", 3, "pipeline"),
        ("(!params || vsom::aligned16(scratch)) && ((uintptr_t)out_u8 & 3) == 0 && ((uintptr_t)offsets & 7) == 0 &&", 3, "pipeline"),
        ("((uintptr_t)shapes & 3) == 0,", 1, "pipeline"),
    ],
    "gmm.hip": [("const bool vec = D % 4 == 0 && ldx % 4 == 0 && aligned16(X) && aligned16(means) && aligned16(prec);", 3, ["gmm_estep"])],
    "kmeans.hip": [
        ("VSOM_REQUIRE(ws && aligned16(ws) && ws_bytes >= vsom_kmeans_workspace_bytes(N, D, k), VSOM_EWORKSPACE", 1, "workspace")] * 4 + [
        ("const bool vec = D % 4 == 0 && ldx % 4 == 0 && aligned16(X) && aligned16(centers);", 2, ["kmeans_assign"])],
    "knn.hip": [
        ("const bool qvec = D % 4 == 0 && ldq % 4 == 0 && aligned16(Q), xvec = D % 4 == 0 && ldx % 4 == 0 && aligned16(X);", 2, ["knn_query"]),
        ("VSOM_REQUIRE(ws && aligned16(ws) && ws_bytes >= vsom_knn_query_workspace_bytes", 1, "workspace"),
        ("VSOM_REQUIRE(ws && aligned16(ws) && ws_bytes >= vsom_umap_knn_workspace_bytes", 1, "workspace"),
        ("VSOM_REQUIRE(ws && aligned16(ws) && ws_bytes >= vsom_knn_ranks_workspace_bytes", 1, "workspace"),
        ("const bool vec = D % 4 == 0 && lda % 4 == 0 && aligned16(A);", 1, ["knn_ranks"]),
        ("VSOM_REQUIRE(ws && aligned16(ws) && ws_bytes >= vsom_silhouette_workspace_bytes", 1, "workspace"),
        ("const bool vec = D % 4 == 0 && ldx % 4 == 0 && aligned16(X);", 1, ["silhouette"]),
    ],
    "pca.hip": [
        ("g.a_vec = aligned16(g.A) && g.lda % 4 == 0;", 1, ["pca_project", "pca_backproject"]),
        ("g.b_vec = aligned16(g.B) && g.ldb % 4 == 0;", 1, ["pca_project", "pca_backproject"]),
        ("const bool fast = g.a_vec && g.b_vec && xcols % 4 == 0 && (!mean || aligned16(mean))", 1, ["pca_project", "pca_backproject"]),
        ('VSOM_REQUIRE(aligned16(part), VSOM_EALIGN, "pca_colstats', 1, "workspace"),
        ('VSOM_REQUIRE(aligned16(slabs), VSOM_EALIGN, "pca_project', 1, "workspace"),
        ('VSOM_REQUIRE(aligned16(slabs), VSOM_EALIGN, "pca_backproject', 1, "workspace"),
    ],
    "umap.hip": [("VSOM_REQUIRE(ws && aligned16(ws) && ws_bytes >= vsom_umap_transform_workspace_bytes", 1, "workspace")],
    "mapviz.hip": [("const bool vec = (p * p * C) % 4 == 0 && vsom::aligned16(pred);", 1, "proto_mosaic")],
    "mapquality.hip": [
        ("if (K % 4 == 0 && vsom::aligned16(dist)) {", 1, "map_stats"),
        ("const bool vec = L % 4 == 0 && vsom::aligned16(W);", 1, ["umatrix"]),
    ],
    "batch_som.hip": [
        ("const bool vec = D % 4 == 0 && ldx % 4 == 0 && aligned16(X);", 1, ["som_batch_accumulate"]),
        ("if (D % 4 == 0 && aligned16(sums))", 1, ["som_batch_update"]),
    ],
    "agglomerative.hip": [
        ("const bool vec = D % 4 == 0 && ldx % 4 == 0 && aligned16(X);", 1, "agglomerative"),
        ("VSOM_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7u) == 0, VSOM_EALIGN", 1, "workspace"),
    ],
    "bmu_x3.hip": [
        ("if (K % 4 == 0 && aligned16(slab))", 1, "workspace"),
        ("const BmuPlan p = x3_plan(B, K, L, ldx, aligned16(X) && aligned16(W), false);", 2, rows_of("bmu_cosine_x3_fwd")),
        ("VSOM_REQUIRE(ws && ws_bytes >= p.ws_bytes && aligned16(ws), VSOM_EWORKSPACE", 1, "workspace"),
        ('VSOM_REQUIRE(aligned16(X) && aligned16(W), VSOM_EALIGN, "bmu_cosine_x3_finalize', 2, rows_of("bmu_cosine_x3_fwd")),
        ("VSOM_REQUIRE(planes && aligned16(planes) && planes_bytes >= vsom_bmu_planes_bytes(R, L), VSOM_EWORKSPACE", 1, "workspace"),
        ("VSOM_REQUIRE(src && ld >= L && ld % 4 == 0 && aligned16(src), VSOM_EINVAL", 1, ["bmu_planes_from"]),
        ("VSOM_REQUIRE(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v), VSOM_EALIGN", 4, ["adamw_step_planes"]),
        ("VSOM_REQUIRE(xplanes && wplanes && aligned16(xplanes) && aligned16(wplanes), VSOM_EINVAL", 2, "planes-dots"),
        ("VSOM_REQUIRE(ws && aligned16(ws) && ws_bytes >= p.ws_bytes, VSOM_EWORKSPACE", 1, "workspace"),
        ('VSOM_REQUIRE(aligned16(X) && aligned16(W), VSOM_EALIGN, "bmu_cosine_x3_planes_finalize', 2,
         ["bmu_cosine_x3_planes_fwd-192x15x256"]),
    ],
}


# ------------------------------------------------------------------------------------------------------- host refusals
# Every REFUSED operand of the table and of the LEFT_OUT entries whose refusal has no wrapper path, as a call of the C entry
# with stand-in pointers (nothing is launched: the refusal precedes every launch).  entry, operand -> (code, call(P_of)), P_of
# maps an operand name to its pointer; header: words the entry's comment in include/vitsom_hip.h must hold for that operand.
P = 4096
BIG = 1 << 40


def host_refusals(L):
    """-> {(entry, operand): (code, call(ptr_of), the status the aligned call must NOT return)}; L = _lib.lib."""
    r = {}

    def add(entry, operands, code, call):
        for o in operands:
            r[(entry, o)] = (code, call)

    add("vsom_adamw_step", "pgmv", EALIGN,
        lambda p: L.vsom_adamw_step(p("p"), p("g"), p("m"), p("v"), P, 1024, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, 1, None))
    need = L.vsom_bmu_planes_bytes(70, 72)
    add("vsom_adamw_step_planes", "pgmv", EALIGN,
        lambda p: L.vsom_adamw_step_planes(p("p"), p("g"), p("m"), p("v"), P, 8192, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, 1, 256, 70, 72, P,
                                           need, None))
    add("vsom_attention_fwd", ["qkv", "out"], EALIGN, lambda p: L.vsom_attention_fwd(p("qkv"), p("out"), P, 2, 17, 2, 16, None))
    add("vsom_attention_bwd", ["qkv", "out", "dout", "dqkv"], EALIGN,
        lambda p: L.vsom_attention_bwd(p("qkv"), p("out"), p("dout"), P, p("dqkv"), P, 2, 17, 2, 16, None))
    add("vsom_attention_q1_fwd", ["q", "kv", "o"], EALIGN, lambda p: L.vsom_attention_q1_fwd(p("q"), p("kv"), p("o"), P, 3, 17, 2, 16, None))
    add("vsom_attention_q1_bwd", ["dout", "o", "q", "kv", "dkv"], EALIGN,
        lambda p: L.vsom_attention_q1_bwd(p("dout"), p("o"), P, p("q"), p("kv"), P, p("dkv"), 3, 17, 2, 16, None))
    add("vsom_tsne_repulsion", ["Y"], EALIGN, lambda p: L.vsom_tsne_repulsion(p("Y"), 130, P, P, P, 3, None))
    B, K, Ld = 70, 15, 256
    ws3 = L.vsom_bmu_cosine_x3_workspace_bytes(B, K, Ld)
    add("vsom_bmu_cosine_x3_dots", ["X", "W"], EALIGN, lambda p: L.vsom_bmu_cosine_x3_dots(p("X"), Ld, p("W"), B, K, Ld, P, ws3, None))
    add("vsom_bmu_cosine_x3_finalize", ["X", "W"], EALIGN,
        lambda p: L.vsom_bmu_cosine_x3_finalize(p("X"), Ld, p("W"), P, 0, P, P, P, P, None, B, K, Ld, None))
    B2 = 192
    add("vsom_bmu_cosine_x3_planes_finalize", ["X", "W"], EALIGN,
        lambda p: L.vsom_bmu_cosine_x3_planes_finalize(p("X"), Ld, p("W"), P, P, P, 0, P, P, P, P, None, B2, K, Ld, None))
    add("vsom_bmu_cosine_x3_planes_dots", ["xplanes", "wplanes"], EINVAL,
        lambda p: L.vsom_bmu_cosine_x3_planes_dots(p("xplanes"), p("wplanes"), B2, K, Ld, P, 0, None))
    add("vsom_bmu_planes_from", ["src"], EINVAL, lambda p: L.vsom_bmu_planes_from(p("src"), Ld, B2, Ld, P, 0, None))
    M, N, Kk = 2048, 64, 192
    add("vsom_linear_bwd_input_ln", ["dY", "Wt", "X", "gamma", "resid", "dX"], EALIGN,
        lambda p: L.vsom_linear_bwd_input_ln(p("dY"), N, p("Wt"), M, N, Kk, p("X"), P, P, p("gamma"), p("resid"), p("dX"), P, P, P, 0, None))
    add("vsom_linear_bwd_input_ln_partial", ["dY", "Wt", "X", "gamma", "resid", "dX"], EALIGN,
        lambda p: L.vsom_linear_bwd_input_ln_partial(p("dY"), N, p("Wt"), M, N, Kk, p("X"), P, P, p("gamma"), p("resid"), p("dX"), P, 0, None))
    crop = (0.08, 1.0, -0.28, 0.28, 0, 0.08, 1.0, -0.28, 0.28, 0.5, 0.25)
    add("vsom_augment_plan", ["params"], EALIGN, lambda p: L.vsom_augment_plan(P, 100, 8, 32, 32, *crop, 7, 0, p("params"), None))
    add("vsom_augment_batch", ["params", "out", "out_u8"], EALIGN,
        lambda p: L.vsom_augment_batch(P, 100, 3, 32, 32, P, p("params"), 8, 32, 32, 0, P, P, 7, 0, p("out"), p("out_u8"), None))
    add("vsom_randaug_plan", ["ra"], EALIGN, lambda p: L.vsom_randaug_plan(P, 100, 8, 32, 2, 1, 0.5, 0, 0, 7, 0, p("ra"), None))
    add("vsom_augment_batch_ra", ["params", "ra", "out", "out_u8"], EALIGN,
        lambda p: L.vsom_augment_batch_ra(P, 100, 3, 32, 32, P, p("params"), p("ra"), 8, 32, P, P, 7, 0, p("out"), p("out_u8"), None))
    add("vsom_augment_plan_ragged", ["params", "shapes"], EALIGN,
        lambda p: L.vsom_augment_plan_ragged(P, p("shapes"), 100, 8, 64, *crop, 7, 0, p("params"), None))
    add("vsom_augment_batch_ragged", ["data", "offsets", "shapes", "params", "scratch", "out", "out_u8"], EALIGN,
        lambda p: L.vsom_augment_batch_ragged(p("data"), 1 << 20, p("offsets"), p("shapes"), 100, 3, 200, 200, P, p("params"), 8, 64, 64, P, P,
                                              7, 0, p("scratch"), 1 << 20, p("out"), p("out_u8"), None))
    return r


# how far a stand-in pointer is moved: by 4 and by 8 bytes (off the 16-byte grid both times); the operands with a weaker
# requirement are moved by what breaks it
WEAK = {"out_u8": (1, 2), "shapes": (1, 2), "offsets": (4, 4)}

# entry -> the operands of the table's rows that reach it under another name
ENTRY_OPERAND = {"vsom_bmu_cosine_x3_dots": {"x": "X", "W": "W"}, "vsom_bmu_cosine_x3_finalize": {"x": "X", "W": "W"},
                 "vsom_bmu_cosine_x3_planes_finalize": {"x": "X", "W": "W"}, "vsom_attention_q1_fwd": {"out": "o"},
                 "vsom_attention_q1_bwd": {"out": "o"}, "vsom_linear_bwd_input_ln": {"dy": "dY", "x": "X", "dx": "dX"}}

# entry -> (words of its comment in include/vitsom_hip.h that state the requirement; the comment is the one that ends last
# before the entry's declaration)
HEADER_WORDS = {
    "vsom_adamw_step": ["16-byte aligned", "VSOM_EALIGN"],
    "vsom_adamw_step_planes": ["16-byte aligned"],
    "vsom_attention_fwd": ["16-byte aligned", "VSOM_EALIGN"],
    "vsom_attention_bwd": ["16-byte aligned", "VSOM_EALIGN"],
    "vsom_attention_q1_fwd": ["16-byte aligned"],
    "vsom_attention_q1_bwd": ["16-byte aligned", "VSOM_EALIGN"],
    "vsom_tsne_repulsion": ["16-byte aligned"],
    "vsom_bmu_cosine_x3_dots": ["16-byte aligned", "VSOM_EALIGN"],
    "vsom_bmu_planes_from": ["16-byte aligned", "VSOM_EINVAL"],
    "vsom_linear_bwd_input_ln": ["16-byte aligned"],
    "vsom_augment_plan": ["16-byte aligned", "VSOM_EALIGN"],
    "vsom_augment_batch": ["16-byte aligned", "VSOM_EALIGN"],
    "vsom_randaug_plan": ["16-byte aligned", "VSOM_EALIGN"],
    "vsom_augment_batch_ra": ["16-byte aligned", "VSOM_EALIGN"],
    "vsom_augment_plan_ragged": ["16-byte aligned", "VSOM_EALIGN"],
    "vsom_augment_batch_ragged": ["16-byte aligned", "VSOM_EALIGN"],
}


# ------------------------------------------------------------------------------------------------------- variants
def variants(row):
    """[(label, {operand: (shift, pad)}, expected)] for one row: each operand alone at shift 1 and 2, each pitch alone at +1
    and +2, then everything at once (only where nothing refuses).  expected: SAME, ELEMENT or a REFUSED."""
    out = []
    size = {F32T: 4, F64T: 8, I32T: 4, I64T: 8, U8T: 1}
    for op in row.ops:
        for s in (1, 2):
            still_aligned = (s * size[op.dtype]) % 16 == 0
            out.append((f"{op.name}+{s}", {op.name: (s, 0)}, SAME if still_aligned else op.shifted))
    for op in row.ops:
        if op.ld:
            for pad in (1, 2):
                out.append((f"{op.name}.ld+{pad}", {op.name: (0, pad)}, op.pitched))
    kinds = [op.shifted for op in row.ops] + [op.pitched for op in row.ops if op.ld]
    if not any(isinstance(k, REFUSED) for k in kinds):
        out.append(("all+1", {op.name: (1, 1 if op.ld else 0) for op in row.ops}, ELEMENT if ELEMENT in kinds else SAME))
    return out
