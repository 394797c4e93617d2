"""Every pitched operand of the library with its last row gigabytes from its base, as data: one entry per (row, operand),
with what the SOURCE does when the row pitch alone grows until the last row starts past 2 GiB, past 4 GiB, or past 2^31
elements.  tests/test_far_pitch_cpu.py holds the table to the sources (the bounds, the windows, the header, every `long ld*`
parameter of include/vitsom_hip.h); tests/test_far_pitch_gpu.py runs every entry inside guarded arenas
(memcheck.GuardedFar).  tests/alignment.py is the sibling table for pitches of + 1 and + 2; its rows are reused here for
every operand it marks `ld=True`, and the rows below (NEW_ROWS, KNN_ROWS, PLAIN_ROWS) add the pitched operands it does not have.

The windows, named by where the last row starts -- byte offset (rows - 1) * ld * itemsize, element offset (rows - 1) * ld:
  signed    byte offset in [2^31 + 2^24, 2^32 - 2^28): negative as `int`, valid as `unsigned`.  Every extent stays below
            every 4 GB test in the sources, so the kernels of the contiguous call run -- the buffer-descriptor kernels
            with byte offsets whose top bit is set;
  wrapped   byte offset >= 2^32 + 2^24, element offset < 2^31: a 32-bit byte offset has wrapped.  The buffer paths must
            have been left (or the call refused);
  element   element offset >= 2^31 + 2^22: an `int` element index has wrapped too (about 8.6 GB for 4-byte types, 17 GB for
            8-byte ones).
`pitch_for` returns the smallest pitch of a window that is a multiple of 4 elements (the 16-byte decision of alignment.py
does not change) and no power of two.

What an operand does in (signed, wrapped, element), read from the dispatch conditions and the kernel bodies:
  PLAIN     (SAME, SAME, SAME): the operand's extent takes part in no dispatch and every access is pointer arithmetic
            with a 64-bit `row * ld`: the outputs are bit-identical to the contiguous call's in all three windows.
  BUFFER    (SAME, ELEMENT, ELEMENT): the operand is a buffer resource of the 16-byte path (launch_gemm, the weight-gradient
            tiles, pca_contract, the kNN family's FAST tiles).  Below 4 GB the same kernel runs; from 0xFFFF0000 bytes
            (kNN: OOB - 256) the host clears `fast` and the generic kernel runs with plain pointers.  That is the kernel
            alignment.py's `pitched` ELEMENT variant reaches (the 16-byte loads it may still use there feed the same values
            into the same arithmetic), so the bits equal that variant's.
  NO4GB     (SAME, REFUSED, REFUSED): the three-product BMU forms and the LayerNorm-fused input gradient have the buffer
            kernels only: VSOM_EUNSUPPORTED, "operand larger than 4 GB", before any launch.

The arenas: one far operand at a time, plus all of a row's pitched operands at once in `signed`.  Operands that share one
`ld` parameter move together (`tied`): in arenas of their own at one pitch (the probe's Z and Zp; the spectral product's
Y1, Y0 and Yout, which the entry forbids to overlap as byte ranges), or, `wide`, as adjacent column slices of one wide
matrix in one arena (the spectral V and W) -- the column slice of a large matrix is the case this table is about.  The front guard holds what a sign-extended 32-bit offset would reach (2 GiB for a byte offset;
2^31 elements in `element`), so the largest arena is an 8-byte operand in `element`: 16 GiB in front of 16 GiB + a little.
PEAK_BYTES bounds what a variant holds at 40 GiB and the CPU test asserts the host arithmetic.

Looked at and left out: LEFT_OUT below, each with its reason; WINDOW_LEFT_OUT for a single window of a covered parameter.
"""
import functools
import os
import re
from collections import namedtuple

import numpy as np
import torch

import alignment as A
from alignment import ELEMENT, EUNSUPPORTED, F32T, F64T, I32T, I64T, IN, INOUT, OUT, REFUSED, SAME, Op, Row, Spec, case, exact, ints, rnd

SIGNED, WRAPPED, ELEMENTW = "signed", "wrapped", "element"
WINDOWS = (SIGNED, WRAPPED, ELEMENTW)
GIB = 1 << 30
PEAK_BYTES = 40 * GIB
FRONT_MIN = 64 << 10

NO4 = REFUSED(EUNSUPPORTED)
PLAIN = (SAME, SAME, SAME)
BUFFER = (SAME, ELEMENT, ELEMENT)
NO4GB = (SAME, NO4, NO4)


def itemsize(dtype):
    return {F32T: 4, F64T: 8, I32T: 4, I64T: 8}[dtype]


def window_of(rows, ld, size):
    """The window the last row of a [rows, .] operand at pitch ld starts in, or None."""
    e = (rows - 1) * ld
    b = e * size
    if (1 << 31) + (1 << 24) <= b < (1 << 32) - (1 << 28):
        return SIGNED
    if b >= (1 << 32) + (1 << 24) and e < (1 << 31):
        return WRAPPED
    if e >= (1 << 31) + (1 << 22):
        return ELEMENTW
    return None


def pitch_for(rows, size, window):
    """The smallest pitch (in elements) of `window` for a [rows, .] operand of `size`-byte elements that is a multiple of 4
    and no power of two."""
    assert rows >= 2 and size in (4, 8) and window in WINDOWS
    start = {SIGNED: ((1 << 31) + (1 << 24)) // size, WRAPPED: ((1 << 32) + (1 << 24)) // size, ELEMENTW: (1 << 31) + (1 << 22)}[window]
    ld = -(-start // (rows - 1))
    ld = (ld + 3) // 4 * 4
    while ld & (ld - 1) == 0:
        ld += 4
    assert window_of(rows, ld, size) == window, (rows, size, window, ld)
    return ld


def front_for(size, window):
    """The front guard of a far arena: what a sign-extended 32-bit byte offset (2 GiB) or, in `element`, a sign-extended
    32-bit element index (2^31 elements) reaches in front of the base, plus the ordinary 64 KiB."""
    return FRONT_MIN + ((1 << 31) * size if window == ELEMENTW else (1 << 31))


def arena_bytes(rows, cols, size, window):
    ld = pitch_for(rows, size, window)
    return front_for(size, window) + ((rows - 1) * ld + cols) * size + (1 << 20) + 256


# ------------------------------------------------------------------------------------------------------- the bounds
# file, pattern with the bound's literals as groups, the value every group must have
Bound = namedtuple("Bound", "file pattern value")
BOUNDS = {
    "gemm": Bound("gemm_f32.hip", r"gemm_vec_extents\(a_kc, b_kc, g\.M, g\.N, g\.K\) && ab < (0x[0-9A-F]+)L && bb < (0x[0-9A-F]+)L;", 0xFFFF0000),
    "wgrad": Bound("gemm_f32.hip", r"lddy % 4 == 0 && ldx % 4 == 0 && ab < (0x[0-9A-F]+)L && bb < (0x[0-9A-F]+)L;", 0xFFFF0000),
    "ln": Bound("gemm_f32.hip", r"VSOM_REQUIRE\(ab < (0x[0-9A-F]+)L && \(long\)M \* K \* 4 < (0x[0-9A-F]+)L, VSOM_EUNSUPPORTED", 0xFFFF0000),
    "pca": Bound("pca.hip", r"\(!mean \|\| aligned16\(mean\)\) && ab < (0x[0-9A-F]+)L && bb < (0x[0-9A-F]+)L;", 0xFFFF0000),
    "x3": Bound("bmu_x3.hip", r"VSOM_REQUIRE\(xb < (0x[0-9A-F]+)L && wb < (0x[0-9A-F]+)L, VSOM_EUNSUPPORTED", 0xFFFF0000),
    "oob": Bound("gemm_f32.h", r"constexpr unsigned OOB = (0x[0-9A-F]+)u;", 0xFFFFFFF0),
    "knn": Bound("knn.hip", r"inline bool knn_buffer_extent\(size_t bytes\) \{ return bytes < \(size_t\)OOB - (\d+); \}", 256),
    "planes": Bound("bmu_x3.hip", r"return planes_image_bytes\(R, L\) < (0x[0-9A-F]+)UL; \}", 0x80000000),
}


def read_bound(key, csrc):
    """The bound as the source under `csrc` has it now (every literal of the pattern, which must agree)."""
    b = BOUNDS[key]
    found = re.findall(b.pattern, open(os.path.join(csrc, b.file)).read())
    assert len(found) == 1, f"{b.file}: {b.pattern!r} matches {len(found)} times"
    vals = {int(v, 0) for v in (found[0] if isinstance(found[0], tuple) else (found[0],))}
    assert len(vals) == 1, (key, vals)
    return vals.pop()


def limit_of(family, csrc):
    """The extent (bytes) from which `family` leaves the buffer path or refuses."""
    if family == "knn":
        return read_bound("oob", csrc) - read_bound("knn", csrc)
    return read_bound(family, csrc)


# The extent of an operand by the source's own formula
def extent_operand_bytes(rows, ld, cols):
    """gemm_f32.h: operand_bytes."""
    return ((rows - 1) * ld + cols) * 4


def extent_knn(rows, ld, cols):
    """knn.hip: `(size_t)N * ld * 4` (knn_search, knn_self_launch)."""
    return rows * ld * 4


def extent_x3(rows, ld, cols):
    """bmu_x3.hip: `((long)(B - 1) * ldx + L) * 4`."""
    return ((rows - 1) * ld + cols) * 4


EXTENT = {"gemm": extent_operand_bytes, "wgrad": extent_operand_bytes, "ln": extent_operand_bytes, "pca": extent_operand_bytes,
          "knn": extent_knn, "x3": extent_x3}
FAMILIES = tuple(EXTENT)


# ------------------------------------------------------------------------------------------------------- new rows
# The pitched operands alignment.ROWS does not have, at the same kind of shape: one full tile plus a ragged one (130 rows),
# inner extents multiples of 4 and not of 16, integer data wherever the operation is exact on it.  check() compares with an
# fp64 / exact torch or numpy evaluation (or the module's reference in tests/*_ref.py), never with a second run of the kernel.
def make_rows_add():
    src, dst = ints(130, 52, seed=50), ints(130, 52, seed=51)
    return case({"src": src, "dst": dst}, want=src.double() + dst.double())


def make_argmax_rows():
    x = ints(130, 52, seed=52, lo=-50, hi=50)
    return case({"x": x, "out": Spec((130,), I64T)}, want=x.double().argmax(1))           # torch: the first maximum, as the kernel


def near(name, got, want, tol):
    """|got - want| <= tol * max|want| (fp64 outputs whose summation order is the kernel's own: tol is a count of fp64
    roundings, written down at each use)."""
    err = float((got.double() - want.double()).abs().max()) / max(float(want.double().abs().max()), 1e-300)
    print(f"FARERR|{name}|rel err {err:.3e}|bound {tol:.3e}")
    return [] if err <= tol else [f"{name}: error {err:.3e} > {tol:.3e} relative to the largest reference value"]


N_, D_, L_ = 130, 52, 10                                                              # rows, row length, basis width


def make_pca_colstats():
    X = ints(N_, D_, seed=53)
    mean = (X.double().sum(0) / N_).float()                                           # an exact sum, divided and rounded once
    var = ((X.double() - mean.double()) ** 2).sum(0) / (N_ - 1)
    return case({"X": X, "mean": Spec((D_,), F32T), "var": Spec((D_,), F64T)}, mean=mean, var=var)


def check_pca_colstats(c, out):
    # var: N_ exact differences squared and added in fp64, in the kernel's order: at most N_ + 2 roundings of 2^-53 each
    return exact("mean", out["mean"], c.mean) + near("var", out["var"], c.var, (N_ + 2) * 2.0 ** -53)


def make_pca_gram():
    Zt, B = ints(L_, D_, seed=54), ints(L_, D_, seed=55)
    return case({"Zt": Zt, "B": B, "G": Spec((L_, L_), F64T), "H": Spec((L_, L_), F64T)}, G=Zt.double() @ Zt.double().T,
                H=B.double() @ Zt.double().T)


def make_pca_rotate():
    T, Zt = ints(6, L_, seed=56).double(), ints(L_, D_, seed=57)
    return case({"T": T, "Zt": Zt, "Bout": Spec((6, D_), F32T)}, want=T @ Zt.double())


def make_pca_reconstruct():
    Y, B, mean = ints(N_, L_, seed=58), ints(L_, D_, seed=59), ints(D_, seed=60)
    scale = 2.0 ** ints(L_, seed=61, lo=-1, hi=1)
    return case({"Y": Y, "scale": scale, "B": B, "mean": mean, "Xout": Spec((N_, D_), F32T)},
                want=(Y.double() * scale.double()) @ B.double() + mean.double())


def make_kmeanspp_dist():
    X = ints(N_, D_, seed=62)
    cand = torch.tensor([5, 129, 64])
    closest = ints(N_, seed=63, lo=100, hi=400)
    d2 = ((X.double()[None, :, :] - X.double()[cand][:, None, :]) ** 2).sum(-1)        # [T, N], integers
    dist = torch.minimum(d2, closest.double()[None, :])
    return case({"X": X, "candidates": cand, "closest": closest, "dist": Spec((3, N_), F32T), "pots": Spec((3,), F64T)},
                dist=dist, pots=dist.sum(1))


def make_kmeans_colvar():
    X = ints(N_, D_, seed=64)
    return case({"X": X, "out": Spec((1,), F64T)}, {"k": 5}, want=X.double().var(0, unbiased=False).mean().reshape(1))


def call_kmeans_colvar(ops, t, a):
    ws = torch.empty(ops.kmeans_workspace_bytes(N_, D_, a["k"]), dtype=torch.uint8, device=t["X"].device)
    ops.kmeans_colvar(t["X"], a["k"], t["out"], ws)


# ---- the kNN family's self contractions (knn.hip: knn_search with X as Q, knn_self_launch) and the matrix kernels beside them
KN, KD, KK = A.KNN_NB, A.KNN_D, A.KNN_K                                               # 130 rows: three 64-column tiles


@functools.lru_cache(maxsize=None)
def _self_distances():
    """X, and the distances the device computes from it, exactly: integer squared distances, correctly rounded roots."""
    X = ints(KN, KD, seed=65)
    d2 = ((X.double()[:, None, :] - X.double()[None, :, :]) ** 2).sum(-1)
    assert float(d2[~torch.eye(KN, dtype=torch.bool)].min()) > 0                       # no duplicate rows: a row is its own nearest
    D32 = np.sqrt(d2.numpy().astype(np.float32))
    eps = float(np.sort(D32[~np.eye(KN, dtype=bool)])[KN * (KN - 1) // 4])             # a distance some pair attains: `<=` matters
    return X, d2, D32, eps


def make_umap_knn():
    import knn_ref
    X, _, D32, _ = _self_distances()
    idx, dist = knn_ref.topk(D32.astype(np.float64), KK)
    assert np.array_equal(idx[:, 0], np.arange(KN))
    return case({"X": X, "knn_idx": Spec((KN, KK), I64T), "knn_dist": Spec((KN, KK), F32T)}, idx=torch.from_numpy(idx),
                dist=torch.from_numpy(dist))


def _graph_case(M, operand):
    import dbscan_ref as DR
    X, d2, D32, eps = _self_distances()
    words = DR.bit_matrix(D32, eps)
    count = DR.popcounts(words, KN)
    t = {operand: X if M is None else M, "adj": Spec((KN, DR.words(KN)), I64T), "count": Spec((KN,), I32T), "status": Spec((2,), I64T)}
    if M is None:
        t["sq"] = Spec((KN,), F32T)
    return case(t, {"eps": eps}, adj=torch.from_numpy(words.view(np.int64).copy()), count=torch.from_numpy(count),
                status=torch.tensor([0, int(count.sum())]), sq=(X.double() ** 2).sum(1))


def make_dbscan_neighbours():
    return _graph_case(None, "X")


def make_dbscan_threshold(dtype):
    return lambda: _graph_case(torch.from_numpy(_self_distances()[2]).to(dtype), "M")


def check_graph(c, out):
    bad = exact("adj", out["adj"], c.adj) + exact("count", out["count"], c.count) + exact("status", out["status"], c.status)
    return bad + (exact("sq", out["sq"], c.sq) if "sq" in out else [])


def call_matrix_entry(entry, pre, post):
    """A matrix entry through _lib.lib: the wrapper takes a float64 matrix only contiguous (ldm = N), the entry any pitch."""
    def call(ops, t, a):
        from vit_som_amd import _lib
        M = t["M"]
        _lib.check(getattr(_lib.lib, entry)(_lib.ptr(M), M.stride(0), KN, int(M.dtype == F64T), *pre(t, a), *[_lib.ptr(t[n]) for n in post],
                                            _lib.stream()), entry)
    return call


def _nearest_case(M, operand):
    """best[i] = the least (w, j) over the rows j of another component, w = max(core[i], core[j], d(i, j)) in float32, packed
    (bits of w) << 32 | j."""
    X, _, D32, _ = _self_distances()
    core = ints(KN, seed=66, lo=3, hi=9).numpy()
    comp = (np.arange(KN) % 3).astype(np.int32)
    w = np.maximum(np.maximum(core[:, None], core[None, :]), D32).astype(np.float32)
    w = np.where(comp[:, None] != comp[None, :], w, np.float32(np.inf))
    key = (w.view(np.uint32).astype(np.int64) << 32) | np.arange(KN, dtype=np.int64)[None, :]    # positive floats order as their bits
    t = {operand: X if M is None else M, "core": torch.from_numpy(core), "comp": torch.from_numpy(comp), "best": Spec((KN,), I64T),
         "record": torch.tensor([KN, 0, 0, 0], dtype=I32T)}
    if M is None:
        t["sq"] = Spec((KN,), F32T)
    return case(t, best=torch.from_numpy(key.min(1)), sq=(X.double() ** 2).sum(1), record=torch.tensor([KN, 0, 0, 0]))


def make_hdbscan_nearest():
    return _nearest_case(None, "X")


def make_hdbscan_nearest_matrix(dtype):
    return lambda: _nearest_case(torch.from_numpy(_self_distances()[2]).to(dtype), "M")


def check_nearest(c, out):
    bad = exact("best", out["best"], c.best) + exact("record", out["record"], c.record)
    return bad + (exact("sq", out["sq"], c.sq) if "sq" in out else [])


def make_agglo_distances():
    X, d2, _, _ = _self_distances()
    return case({"X": X, "out": Spec((KN, KN), F64T), "status": Spec((2,), I32T)}, want=d2, status=torch.tensor([0, 0]))


def call_agglo_distances(ops, t, a):
    """Through _lib.lib: the wrapper takes `out` only contiguous (ldo = N), the entry any pitch."""
    from vit_som_amd import _lib
    X, out = t["X"], t["out"]
    _lib.check(_lib.lib.vsom_agglo_distances(_lib.ptr(X), X.stride(0), KN, KD, ops.AGGLO_EUCLIDEAN, 1, _lib.ptr(out), out.stride(0),
                                             _lib.ptr(t["status"]), _lib.stream()), "vsom_agglo_distances")


# ---- linear_probe.hip, spectral.hip, tsne.hip, gmm.hip: plain pointers
PC = 12                                                                               # classes: a multiple of 4, not of 16


def make_probe_fold():
    Af, invstd = ints(PC, D_, seed=67).double(), (2.0 ** ints(D_, seed=68, lo=-2, hi=2)).double()
    return case({"A": Af, "invstd": invstd, "B": Spec((PC, D_), F32T)}, want=Af * invstd)


@functools.lru_cache(maxsize=None)
def _logits():
    g = torch.Generator().manual_seed(69)
    Z, Zp = rnd(N_, PC, seed=70) * 3, rnd(N_, PC, seed=71)
    y = torch.randint(0, PC, (N_,), generator=g)
    return Z, Zp, y, rnd(PC, seed=72).double(), rnd(PC, seed=73).double()


def make_probe_residual():
    import linear_probe_ref as LR
    Z, _, y, b, _ = _logits()
    R32, loss, gb, _, _ = LR.residual(Z.numpy(), b.numpy(), y.numpy())
    return case({"Z": Z, "b": b, "y": y, "R": Spec((N_, PC), F32T), "loss": Spec((1,), F64T), "gb": Spec((PC,), F64T),
                 "status": torch.zeros(1, dtype=I32T)},
                R=torch.from_numpy(R32), loss=torch.tensor([loss], dtype=F64T), gb=torch.from_numpy(np.asarray(gb)))


def check_probe_residual(c, out):
    """test_linear_probe_gpu.py::test_residual_against_fp64's bounds: R within 2^-23, loss and gb 1e-12 relative."""
    err = float((out["R"].double() - c.R.double()).abs().max())
    bad = [] if err <= 2.0 ** -23 else [f"R: {err:.3e} > 2^-23"]
    return bad + near("loss", out["loss"], c.loss, 1e-12) + near("gb", out["gb"], c.gb, 1e-12) + exact("status", out["status"], torch.zeros(1))


def make_probe_linesearch():
    import linear_probe_ref as LR
    Z, Zp, y, b, pb = _logits()
    phi = LR.ladder(Z.numpy(), Zp.numpy(), b.numpy(), pb.numpy(), y.numpy(), 0.75, 8)
    return case({"Z": Z, "Zp": Zp, "b": b, "pb": pb, "y": y, "alpha0": torch.tensor([0.75], dtype=F64T), "phi": Spec((8,), F64T)},
                phi=torch.from_numpy(phi))


def make_probe_step():
    """test_linear_probe_gpu.py's exact case: Z and Zp multiples of 2^-6, alpha_j = 2^-j, so Z + alpha Zp is exact in f32."""
    import linear_probe_ref as LR
    g = torch.Generator().manual_seed(74)
    Z = torch.randint(-512, 513, (N_, PC), generator=g).float() / 64
    Zp = torch.randint(-256, 257, (N_, PC), generator=g).float() / 64
    y = torch.randint(0, PC, (N_,), generator=g)
    n = PC * 7 + PC
    theta, p = rnd(n, seed=75).double(), rnd(n, seed=76).double()
    b, pb = theta[PC * 7:], p[PC * 7:]
    phi = LR.ladder(Z.numpy(), Zp.numpy(), b.numpy(), pb.numpy(), y.numpy(), 1.0, 8)
    f0, lam, pen, gtp = float(phi[3]) + 1.0, 0.01, np.array([3.0, -0.5, 2.0]), -1e-6
    alpha, status, F, j = LR.armijo(phi, 1.0, f0, pen, gtp, N_, lam)
    assert status == 0 and alpha > 0
    t = {"phi": torch.from_numpy(phi), "alpha0": torch.tensor([1.0], dtype=F64T), "f0": torch.tensor([f0], dtype=F64T),
         "pen": torch.from_numpy(pen), "gtp": torch.tensor([gtp], dtype=F64T), "Z": Z, "Zp": Zp, "theta": theta, "p": p,
         "s_new": Spec((n,), F64T), "rec": torch.zeros(16, dtype=F64T)}
    rec = torch.zeros(16, dtype=F64T)
    rec[12:16] = torch.tensor([alpha, status, F, j], dtype=F64T)
    return case(t, {"lam": lam}, Z=Z.double() + alpha * Zp.double(), theta=theta + alpha * p, s=alpha * p, rec=rec)


def make_probe_gradient():
    Zt, invstd = rnd(PC, D_, seed=77), torch.rand(D_, generator=torch.Generator().manual_seed(78)).double() + 0.5
    theta, gb = rnd(PC * D_ + PC, seed=79).double(), rnd(PC, seed=80).double()
    lam = 1.0 / (0.7 * 300)
    want = torch.cat([(Zt.double() * invstd / 300 + lam * theta[:PC * D_].view(PC, D_)).reshape(-1), gb / 300])
    return case({"Zt": Zt, "invstd": invstd, "theta": theta, "gb": gb, "g": Spec((PC * D_ + PC,), F64T)}, {"lam": lam}, want=want)


SL = 8                                                                                # columns of a spectral block


def make_spectral_rotate():
    V, T = ints(N_, SL, seed=81).double(), ints(SL, 4, seed=82).double()
    return case({"V": V, "T": T, "out": Spec((N_, 4), F64T)}, want=V @ T)


def make_spectral_embed():
    V, s = ints(N_, SL, seed=83).double(), (2.0 ** ints(N_, seed=84, lo=-2, hi=2)).double()
    Y = s[:, None] * V[:, 2:6]
    first_max = Y.abs().argmax(0)                                                     # torch: the first maximum, the smaller row
    sign = torch.sign(Y[first_max, torch.arange(4)])
    assert bool((sign != 0).all())
    return case({"V": V, "s": s, "E": Spec((N_, 4), F32T), "sign": Spec((4,), F64T)}, E=Y * sign, sign=sign)


TS_K, TS_PERP = 12, 3.0


def make_tsne_affinities():
    import knn_ref
    _, _, D32, _ = _self_distances()
    _, dist = knn_ref.topk(D32.astype(np.float64), TS_K)                              # the row itself first, as vsom_umap_knn leaves it
    dist = torch.from_numpy(np.ascontiguousarray(dist, dtype=np.float32))
    return case({"knn_dist": dist, "P": Spec((KN, TS_K - 1), F64T), "beta": Spec((KN,), F64T), "status": torch.zeros(1, dtype=I32T)})


def check_tsne_affinities(c, out):
    """test_tsne_gpu.py::test_affinities_follow_the_bisection: beta is the restated bisection's iterate at its stop (or the one
    next to it) to 1e-12, P the restated conditional probabilities at that beta to 1e-12 of the row maximum."""
    import tsne_ref as TR
    d = TR.squared_f32(c.t["knn_dist"].numpy()[:, 1:])
    betas, _, stop = TR.bisection_trace(d, TS_PERP)
    bg, Pg = out["beta"].numpy(), out["P"].numpy()
    bad = exact("status", out["status"], torch.zeros(1))
    for i in range(KN):
        near_stop = [betas[t, i] for t in (stop[i], stop[i] - 1, stop[i] + 1) if 0 <= t < TR.N_STEPS]
        if not any(abs(bg[i] - v) <= 1e-12 * v for v in near_stop):
            bad.append(f"beta[{i}] = {bg[i]!r} is none of the iterates around the stop")
            break
    if not bad:
        want = TR.conditional_p_at(d, bg)
        err = float((np.abs(Pg - want) / want.max(axis=1, keepdims=True)).max())
        if not err <= 1e-12:
            bad.append(f"P: {err:.3e} of the row maximum")
    return bad


GMK = 5


def make_gmm_mstep():
    import gmm_ref as GR
    X, means, _, _ = GR.mixture_case(N_, D_, GMK, "diag")
    resp = np.random.RandomState(5).dirichlet(np.ones(GMK), size=N_).astype(np.float32)
    nk, mu, cov = GR.mstep64(X, resp, 1e-6, "diag")
    nk32, mu32, cov32 = GR.mstep32(X, resp, 1e-6, "diag")
    return case({"X": torch.from_numpy(np.ascontiguousarray(X)).float(), "resp": torch.from_numpy(resp),
                 "means_old": torch.from_numpy(np.ascontiguousarray(means)).float()},
                ref=dict(means=mu, cov=cov, weights=nk / nk.sum()), y32=dict(means=mu32, cov=cov32, weights=nk32 / nk32.sum()))


def call_gmm_mstep(ops, t, a):
    """The M-step's partial sums have no layout of their own to check: vsom_gmm_params turns them into parameters."""
    dev = t["X"].device
    new = lambda shape, dtype: torch.empty(*shape, dtype=dtype, device=dev)          # noqa: E731
    part = new((ops.gmm_parts(N_, D_, GMK, ops.GMM_MSTEP),), F64T)
    means, cov, prec = new((GMK, D_), F32T), new((GMK, D_), F64T), new((GMK, D_), F32T)
    weights, logc, record = new((GMK,), F64T), new((GMK,), F64T), new((ops.GMM_RECORD,), F64T)
    ops.gmm_mstep(t["X"], t["resp"], t["means_old"], part)
    ops.gmm_params(part, N_, t["means_old"], 1e-6, False, 0, None, means, cov, prec, weights, logc, record)
    return {"means": means, "cov": cov, "weights": weights}


def check_gmm_mstep(c, out):
    """test_gmm_gpu.py::test_mstep_and_params_against_fp64: max(FLOOR, 4 e32) relative to the largest reference value."""
    import gmm_ref as GR
    bad = []
    for key in ("means", "cov", "weights"):
        e_k, lim = GR.err(out[key].numpy(), c.ref[key]), GR.bound(GR.FLOOR, GR.err(c.y32[key], c.ref[key]))
        print(f"FARERR|gmm_mstep {key}|e_k={e_k:.3e}|bound={lim:.3e}")
        if not e_k <= lim:
            bad.append(f"{key}: error {e_k:.3e} > {lim:.3e}")
    return bad


KMK = 5


def make_kmeans_relocate():
    """Cluster 4's centre lies far from every row, so vsom_kmeans_update leaves it empty; the host's move gives it the LAST
    row of X (the row a far pitch puts furthest from the base).  Integer data: the cluster sums are exact in float32, and a
    centre is sum * (1.0f / count), restated in numpy float32."""
    X = ints(N_, D_, seed=85)
    C = torch.cat([ints(KMK - 1, D_, seed=86), torch.full((1, D_), 100.0)])
    d2 = ((X.double()[:, None, :] - C.double()[None, :, :]) ** 2).sum(-1)
    labels = d2.argmin(1)
    far = N_ - 1
    old = int(labels[far])
    sums = torch.zeros(KMK, D_, dtype=F64T).index_add_(0, labels, X.double())
    counts = torch.bincount(labels, minlength=KMK)
    assert int(counts[KMK - 1]) == 0 and int(counts.min(0).values) == 0 and int(counts[old]) > 1 and int((counts == 0).sum()) == 1
    sums[old] -= X[far].double()
    sums[KMK - 1] = X[far].double()
    counts[KMK - 1], counts[old] = 1, counts[old] - 1
    new = sums.numpy().astype(np.float32) * (np.float32(1.0) / counts.numpy().astype(np.float32))[:, None]
    shift = ((new.astype(np.float64) - C.double().numpy()) ** 2).sum()
    return case({"X": X, "centers": C, "moves": torch.tensor([[KMK - 1, far]]), "centers_new": Spec((KMK, D_), F32T),
                 "counts": Spec((KMK,), I64T), "status": Spec((4,), F64T)}, new=torch.from_numpy(new), counts=counts,
                shift=torch.tensor([shift], dtype=F64T))


def call_kmeans_relocate(ops, t, a):
    """vsom_kmeans_assign and vsom_kmeans_update on a contiguous copy of X fill the workspace (the alignment table's
    kmeans_assign row moves their X); vsom_kmeans_relocate alone reads the operand under test."""
    X, dev = t["X"], t["X"].device
    ws = torch.empty(ops.kmeans_workspace_bytes(N_, D_, KMK), dtype=torch.uint8, device=dev)
    labels, prev = torch.empty(N_, dtype=I64T, device=dev), torch.zeros(N_, dtype=I64T, device=dev)
    mind, mid = torch.empty(N_, dtype=F32T, device=dev), torch.empty(KMK, D_, dtype=F32T, device=dev)
    ops.kmeans_assign(X.contiguous().clone(), t["centers"], labels, prev, mind, ws)
    ops.kmeans_update(t["centers"], mid, N_, mind, t["counts"], t["status"], ws)
    ops.kmeans_relocate(X, labels, t["moves"], t["centers"], t["centers_new"], t["counts"], t["status"], ws)


def check_kmeans_relocate(c, out):
    # status[1]: k D squares of exact differences added in fp64 in the kernel's order; status[2]: no cluster is left empty
    return (exact("centers_new", out["centers_new"], c.new) + exact("counts", out["counts"], c.counts) +
            near("center shift", out["status"][1:2], c.shift, (KMK * D_ + 2) * 2.0 ** -53) + exact("empty", out["status"][2:3], torch.zeros(1)))


@functools.lru_cache(maxsize=None)
def _graph():
    """A sparse symmetric integer matrix with a diagonal (which the operator skips) as CSR, and s = powers of two: with
    integer blocks every product and sum of the spectral kernels is exact in fp64, whatever its order."""
    g = torch.Generator().manual_seed(87)
    Ad = (torch.rand(N_, N_, generator=g) < 0.08).double() * torch.randint(1, 4, (N_, N_), generator=g).double()
    Ad = torch.triu(Ad, 1)
    Ad[0, N_ - 1] = 2.0                                                               # the last row has a neighbour and is one
    Ad = Ad + Ad.T + torch.eye(N_, dtype=F64T)
    at = Ad.nonzero()                                                                 # row-major: CSR order
    indptr = torch.cat([torch.zeros(1, dtype=I64T), torch.bincount(at[:, 0], minlength=N_).cumsum(0)])
    s = (2.0 ** ints(N_, seed=88, lo=-1, hi=1)).double()
    off = Ad - torch.diag(torch.diag(Ad))
    return indptr, at[:, 1].contiguous(), Ad[at[:, 0], at[:, 1]].contiguous(), s, off


def make_spectral_spmm():
    indptr, indices, data, s, off = _graph()
    Y1, Y0 = ints(N_, SL, seed=89).double(), ints(N_, SL, seed=90).double()
    want = 2.0 * (s[:, None] * (off @ (s[:, None] * Y1)) - 1.0 * Y1) - 1.0 * Y0
    return case({"indptr": indptr, "indices": indices, "data": data, "s": s, "Y1": Y1, "Y0": Y0, "out": Spec((N_, SL), F64T)}, want=want)


def make_spectral_gram():
    V, W = ints(N_, SL, seed=91).double(), ints(N_, SL, seed=92).double()
    return case({"V": V, "W": W, "G": Spec((SL, SL), F64T), "H": Spec((SL, SL), F64T)}, G=V.T @ V, H=V.T @ W)


def make_spectral_residual():
    V, W, theta = ints(N_, SL, seed=93).double(), ints(N_, SL, seed=94).double(), ints(SL, seed=95).double()
    return case({"V": V, "W": W, "theta": theta, "out": Spec((SL,), F64T)}, want=((W - V * theta) ** 2).sum(0))


def _pitched(name, dtype=F32T, role=IN, kind=SAME):
    return Op(name, dtype, role, ld=True, pitched=kind)


def _f64(*names, role=IN):
    return [Op(n, F64T, role) for n in names]


PLAIN_ROWS = [
    Row("probe_fold", "probe_fold", "vsom_probe_fold", make_probe_fold, lambda ops, t, a: ops.probe_fold(t["A"], t["invstd"], t["B"]),
        _f64("A", "invstd") + [_pitched("B", role=OUT)], lambda c, out: exact("B", out["B"], c.want.float())),
    Row("probe_residual", "probe_residual", "vsom_probe_residual", make_probe_residual,
        lambda ops, t, a: ops.probe_residual(t["Z"], t["b"], t["y"], t["R"], t["loss"], t["gb"], t["status"]),
        [_pitched("Z"), Op("b", F64T, IN), Op("y", I64T, IN), _pitched("R", role=OUT), Op("loss", F64T, OUT), Op("gb", F64T, OUT),
         Op("status", I32T, INOUT)], check_probe_residual),
    # Z and Zp share one pitch (ldz): they move together
    Row("probe_linesearch", "probe_linesearch", "vsom_probe_linesearch", make_probe_linesearch,
        lambda ops, t, a: ops.probe_linesearch(t["Z"], t["Zp"], t["b"], t["pb"], t["y"], t["alpha0"], 8, t["phi"]),
        [_pitched("Z"), _pitched("Zp"), Op("b", F64T, IN), Op("pb", F64T, IN), Op("y", I64T, IN), Op("alpha0", F64T, IN),
         Op("phi", F64T, OUT)], lambda c, out: near("phi", out["phi"], c.phi, 1e-12)),       # test_linesearch_ladder_against_fp64
    Row("probe_step", "probe_step", "vsom_probe_step", make_probe_step,
        lambda ops, t, a: ops.probe_step(t["phi"], t["alpha0"], t["f0"], t["pen"], t["gtp"], a["lam"], 1e-4, t["Z"], t["Zp"], t["theta"],
                                         t["p"], t["s_new"], t["rec"]),
        _f64("phi", "alpha0", "f0", "pen", "gtp") + [_pitched("Z", role=INOUT), _pitched("Zp"), Op("theta", F64T, INOUT), Op("p", F64T, IN),
                                                      Op("s_new", F64T, OUT), Op("rec", F64T, INOUT)],
        lambda c, out: (exact("Z", out["Z"], c.Z) + exact("theta", out["theta"], c.theta) + exact("s_new", out["s_new"], c.s) +
                        exact("rec", out["rec"], c.rec))),
    Row("probe_gradient", "probe_gradient", "vsom_probe_gradient", make_probe_gradient,
        lambda ops, t, a: ops.probe_gradient(t["Zt"], t["invstd"], t["theta"], t["gb"], 300, a["lam"], t["g"]),
        [_pitched("Zt")] + _f64("invstd", "theta", "gb") + [Op("g", F64T, OUT)],
        lambda c, out: near("g", out["g"], c.want, 2.0 ** -48)),                             # test_fold_and_gradient: a handful of roundings
    Row("spectral_rotate", "spectral_rotate", "vsom_spectral_rotate", make_spectral_rotate,
        lambda ops, t, a: ops.spectral_rotate(t["V"], t["T"], t["out"]),
        [_pitched("V", F64T), Op("T", F64T, IN), _pitched("out", F64T, OUT)], lambda c, out: exact("out", out["out"], c.want)),
    Row("spectral_embed", "spectral_embed", "vsom_spectral_embed", make_spectral_embed,
        lambda ops, t, a: ops.spectral_embed(t["V"], t["s"], 2, t["E"], t["sign"]),
        [_pitched("V", F64T), Op("s", F64T, IN), _pitched("E", role=OUT), Op("sign", F64T, OUT)],
        lambda c, out: exact("E", out["E"], c.E) + exact("sign", out["sign"], c.sign)),
    # Y1, Y0 and out share one ld and may not overlap as byte ranges (the entry refuses it): three arenas at one pitch
    Row("spectral_spmm", "spectral_spmm", "vsom_spectral_spmm", make_spectral_spmm,
        lambda ops, t, a: ops.spectral_spmm(t["indptr"], t["indices"], t["data"], t["s"], t["Y1"], t["Y0"], t["out"], alpha=2.0, c=1.0, beta=1.0),
        [Op("indptr", I64T, IN), Op("indices", I64T, IN), Op("data", F64T, IN), Op("s", F64T, IN), _pitched("Y1", F64T), _pitched("Y0", F64T),
         _pitched("out", F64T, OUT)], lambda c, out: exact("out", out["out"], c.want)),
    # V and W share one ld: adjacent column slices of one wide matrix
    Row("spectral_gram", "spectral_gram", "vsom_spectral_gram", make_spectral_gram,
        lambda ops, t, a: ops.spectral_gram(t["V"], t["W"], t["G"], t["H"], slabs=3),
        [_pitched("V", F64T), _pitched("W", F64T), Op("G", F64T, OUT), Op("H", F64T, OUT)],
        lambda c, out: exact("G", out["G"], c.G) + exact("H", out["H"], c.H)),
    Row("spectral_residual", "spectral_residual", "vsom_spectral_residual", make_spectral_residual,
        lambda ops, t, a: ops.spectral_residual(t["V"], t["W"], t["theta"], t["out"], slabs=3),
        [_pitched("V", F64T), _pitched("W", F64T), Op("theta", F64T, IN), Op("out", F64T, OUT)],
        lambda c, out: exact("out", out["out"], c.want)),
    Row("kmeans_relocate", "kmeans_relocate", "vsom_kmeans_relocate", make_kmeans_relocate, call_kmeans_relocate,
        [_pitched("X"), Op("centers", F32T, IN), Op("moves", I64T, IN), Op("centers_new", F32T, OUT), Op("counts", I64T, OUT),
         Op("status", F64T, OUT)], check_kmeans_relocate),
    Row("tsne_affinities", "tsne_affinities", "vsom_tsne_affinities", make_tsne_affinities,
        lambda ops, t, a: ops.tsne_affinities(t["knn_dist"], TS_PERP, t["P"], t["beta"], t["status"]),
        [_pitched("knn_dist"), Op("P", F64T, OUT), Op("beta", F64T, OUT), Op("status", I32T, INOUT)], check_tsne_affinities),
    Row("gmm_mstep", "gmm_mstep", "vsom_gmm_mstep", make_gmm_mstep, call_gmm_mstep,
        [_pitched("X"), _pitched("resp"), Op("means_old", F32T, IN)], check_gmm_mstep),
]


_GRAPH_OUT = [Op("adj", I64T, OUT), Op("count", I32T, OUT), Op("status", I64T, OUT)]
_NEAREST_REST = [Op("core", F32T, IN), Op("comp", I32T, IN), Op("best", I64T, OUT), Op("record", I32T, INOUT)]

KNN_ROWS = [
    Row("umap_knn", "umap_knn", "vsom_umap_knn", make_umap_knn,
        lambda ops, t, a: ops.umap_knn(t["X"], KK, ops.DIST_EUCLIDEAN, t["knn_idx"], t["knn_dist"]),
        [_pitched("X", kind=ELEMENT), Op("knn_idx", I64T, OUT), Op("knn_dist", F32T, OUT)],
        lambda c, out: exact("knn_idx", out["knn_idx"], c.idx) + exact("knn_dist", out["knn_dist"], c.dist)),
    Row("dbscan_neighbours", "dbscan_neighbours", "vsom_dbscan_neighbours", make_dbscan_neighbours,
        lambda ops, t, a: ops.dbscan_neighbours(t["X"], ops.DIST_EUCLIDEAN, a["eps"], t["sq"], t["adj"], t["count"], t["status"]),
        [_pitched("X", kind=ELEMENT), Op("sq", F32T, OUT)] + _GRAPH_OUT, check_graph),
    Row("dbscan_threshold-f32", "dbscan_threshold", "vsom_dbscan_threshold", make_dbscan_threshold(F32T),
        lambda ops, t, a: ops.dbscan_threshold(t["M"], a["eps"], t["adj"], t["count"], t["status"]),
        [_pitched("M")] + _GRAPH_OUT, check_graph),
    Row("dbscan_threshold-f64", "lib", "vsom_dbscan_threshold", make_dbscan_threshold(F64T),
        call_matrix_entry("vsom_dbscan_threshold", lambda t, a: (a["eps"],), ("adj", "count", "status")),
        [_pitched("M", F64T)] + _GRAPH_OUT, check_graph),
    Row("hdbscan_nearest", "hdbscan_nearest", "vsom_hdbscan_nearest", make_hdbscan_nearest,
        lambda ops, t, a: ops.hdbscan_nearest(t["X"], ops.DIST_EUCLIDEAN, t["core"], t["comp"], t["sq"], t["best"], t["record"]),
        [_pitched("X", kind=ELEMENT), Op("sq", F32T, OUT)] + _NEAREST_REST, check_nearest),
    Row("hdbscan_nearest_matrix-f32", "hdbscan_nearest_matrix", "vsom_hdbscan_nearest_matrix", make_hdbscan_nearest_matrix(F32T),
        lambda ops, t, a: ops.hdbscan_nearest_matrix(t["M"], t["core"], t["comp"], t["best"], t["record"]),
        [_pitched("M")] + _NEAREST_REST, check_nearest),
    Row("hdbscan_nearest_matrix-f64", "lib", "vsom_hdbscan_nearest_matrix", make_hdbscan_nearest_matrix(F64T),
        call_matrix_entry("vsom_hdbscan_nearest_matrix", lambda t, a: (), ("core", "comp", "best", "record")),
        [_pitched("M", F64T)] + _NEAREST_REST, check_nearest),
    # agglomerative.hip: the direct form in fp64, exact on integers when squared
    Row("agglo_distances", "lib", "vsom_agglo_distances", make_agglo_distances, call_agglo_distances,
        [_pitched("X"), _pitched("out", F64T, OUT), Op("status", I32T, OUT)],
        lambda c, out: exact("out", out["out"], c.want) + exact("status", out["status"], c.status)),
]


NEW_ROWS = [
    Row("rows_add", "rows_add", "vsom_rows_add", make_rows_add, lambda ops, t, a: ops.rows_add(t["src"], t["dst"]),
        [_pitched("src"), _pitched("dst", role=INOUT)], lambda c, out: exact("dst", out["dst"], c.want)),
    Row("argmax_rows", "argmax_rows", "vsom_argmax_rows", make_argmax_rows, lambda ops, t, a: ops.argmax_rows(t["x"], t["out"]),
        [_pitched("x"), Op("out", I64T, OUT)], lambda c, out: exact("out", out["out"], c.want)),
    # ---- pca.hip beyond project / backproject: plain pointers, `(long)row * ld`
    Row("pca_colstats", "pca_colstats", "vsom_pca_colstats", make_pca_colstats,
        lambda ops, t, a: ops.pca_colstats(t["X"], t["mean"], t["var"]),
        [_pitched("X"), Op("mean", F32T, OUT), Op("var", F64T, OUT)], check_pca_colstats),
    Row("pca_gram", "pca_gram", "vsom_pca_gram", make_pca_gram, lambda ops, t, a: ops.pca_gram(t["Zt"], t["G"], t["B"], t["H"]),
        [_pitched("Zt"), _pitched("B"), Op("G", F64T, OUT), Op("H", F64T, OUT)],
        lambda c, out: exact("G", out["G"], c.G) + exact("H", out["H"], c.H)),
    Row("pca_rotate", "pca_rotate", "vsom_pca_rotate", make_pca_rotate, lambda ops, t, a: ops.pca_rotate(t["T"], t["Zt"], t["Bout"]),
        [Op("T", F64T, IN), _pitched("Zt"), _pitched("Bout", role=OUT)], lambda c, out: exact("Bout", out["Bout"], c.want)),
    Row("pca_reconstruct", "pca_reconstruct", "vsom_pca_reconstruct", make_pca_reconstruct,
        lambda ops, t, a: ops.pca_reconstruct(t["Y"], t["scale"], t["B"], t["mean"], t["Xout"]),
        [_pitched("Y"), Op("scale", F32T, IN), _pitched("B"), Op("mean", F32T, IN), _pitched("Xout", role=OUT)],
        lambda c, out: exact("Xout", out["Xout"], c.want)),
    # ---- kmeans.hip beyond assign
    Row("kmeanspp_dist", "kmeanspp_dist", "vsom_kmeanspp_dist", make_kmeanspp_dist,
        lambda ops, t, a: ops.kmeanspp_dist(t["X"], t["candidates"], t["closest"], t["dist"], t["pots"]),
        [_pitched("X"), Op("candidates", I64T, IN), Op("closest", F32T, IN), Op("dist", F32T, OUT), Op("pots", F64T, OUT)],
        lambda c, out: exact("dist", out["dist"], c.dist) + exact("pots", out["pots"], c.pots)),
    # the column sums and sums of squares are exact integers in fp64; the variance and the mean over D_ columns round a few times
    Row("kmeans_colvar", "kmeans_colvar", "vsom_kmeans_colvar", make_kmeans_colvar, call_kmeans_colvar,
        [_pitched("X"), Op("out", F64T, OUT)], lambda c, out: near("colvar", out["out"], c.want, (D_ + 8) * 2.0 ** -53 * 4)),
]

ROWS = list(A.ROWS) + NEW_ROWS + KNN_ROWS + PLAIN_ROWS
ROW_BY_ID = {r.id: r for r in ROWS}
assert len(ROW_BY_ID) == len(ROWS)


# ------------------------------------------------------------------------------------------------------- the table
# row id; operand; what it does in (signed, wrapped, element); the (entry, parameter) pairs of include/vitsom_hip.h it
# covers; family: whose bound its extent crosses (None for PLAIN); tied: the operands that share its `ld` parameter and move
# with it, at the same pitch -- in arenas of their own, or (wide) as adjacent column slices of one wide matrix in one arena.
# An expectation of None: the window is not run, and WINDOW_LEFT_OUT says why
Far = namedtuple("Far", "row op expect covers family tied wide", defaults=(None, (), False))


def _gemm_x(row, entry, op="x", ld="ldx"):
    return Far(row, op, BUFFER, [(entry, ld)], "gemm")


TABLE = [
    # ---- launch_gemm: A / B are buffer resources of the FAST kernels (init_kc / load_kc_fast, init_ks / load_ks_fast, gemm_x6.h),
    # `fast` needs both extents below 0xFFFF0000; C, C2 and R are plain pointers in gemm_epilogue
    _gemm_x("linear_fwd", "vsom_linear_fwd"), Far("linear_fwd", "out", PLAIN, [("vsom_linear_fwd", "ldy")]),
    _gemm_x("linear_gelu_fwd", "vsom_linear_gelu_fwd"),
    _gemm_x("linear_relu_fwd", "vsom_linear_relu_fwd"),
    _gemm_x("linear_residual_fwd", "vsom_linear_residual_fwd"),
    Far("linear_residual_fwd", "R", PLAIN, [("vsom_linear_residual_fwd", "ldr")]),
    Far("linear_residual_fwd", "out", PLAIN, [("vsom_linear_residual_fwd", "ldy")]),
    _gemm_x("linear_bwd_input", "vsom_linear_bwd_input", "dy", "lddy"), Far("linear_bwd_input", "dx", PLAIN, [("vsom_linear_bwd_input", "lddx")]),
    _gemm_x("linear_bwd_input_t", "vsom_linear_bwd_input_t", "dy", "lddy"),
    Far("linear_bwd_input_t", "dx", PLAIN, [("vsom_linear_bwd_input_t", "lddx")]),
    # the generic weight-gradient GEMM (TN: both operands k-strided) at this shape, the 192 x 64 tiles (gemm_x6_tn.h) at the
    # other: `vec` (gemm_f32.hip) sends an operand of 0xFFFF0000 bytes or more to launch_gemm, which leaves FAST by its own test
    Far("linear_bwd_weight", "dy", BUFFER, [("vsom_linear_bwd_weight", "lddy")], "gemm"),
    Far("linear_bwd_weight", "x", BUFFER, [("vsom_linear_bwd_weight", "ldx")], "gemm"),
    Far("linear_bwd_weight-tiles", "dy", BUFFER, [("vsom_linear_bwd_weight", "lddy")], "wgrad"),
    Far("linear_bwd_weight-tiles", "x", BUFFER, [("vsom_linear_bwd_weight", "ldx")], "wgrad"),
    # X is the k-strided B of the gW GEMM and the plain R of the gX one
    _gemm_x("som_bwd", "vsom_som_bwd"), Far("som_bwd", "gX", PLAIN, [("vsom_som_bwd", "ldgx")]),
    _gemm_x("bmu_euclid_fwd-70x15x256", "vsom_bmu_euclid_fwd"), _gemm_x("bmu_euclid_fwd-33x100x48", "vsom_bmu_euclid_fwd"),
    _gemm_x("bmu_cosine_fwd-70x15x256", "vsom_bmu_cosine_dots"), _gemm_x("bmu_cosine_fwd-33x100x48", "vsom_bmu_cosine_dots"),
    # reduce_slabs_body: `slabs + s * stride` in 64 bits; the parameter is `stride`, no `ld`
    Far("reduce_slabs", "slabs", PLAIN, []),
    # ---- bmu_x3.hip: one rule for the family (x3_operands_fit)
    Far("bmu_cosine_x3_fwd-70x15x256", "x", NO4GB, [("vsom_bmu_cosine_x3_dots", "ldx"), ("vsom_bmu_cosine_x3_finalize", "ldx")], "x3"),
    Far("bmu_cosine_x3_fwd-33x100x48", "x", NO4GB, [("vsom_bmu_cosine_x3_dots", "ldx"), ("vsom_bmu_cosine_x3_finalize", "ldx")], "x3"),
    Far("bmu_cosine_x3_planes_fwd-192x15x256", "x", NO4GB, [("vsom_bmu_cosine_x3_planes_finalize", "ldx")], "x3"),
    # planes_kernel reads `q.src + (long)row * q.ld + k`; the 2 GB bound is on the image (R, L), which a pitch does not change
    Far("bmu_planes_from", "src", PLAIN, [("vsom_bmu_planes_from", "ld")]),
    Far("linear_bwd_input_ln", "dy", NO4GB, [("vsom_linear_bwd_input_ln", "lddy")], "ln"),
    # ---- plain pointers
    Far("row_inv_norm", "x", PLAIN, [("vsom_row_inv_norm", "ldx")]), Far("row_sqnorm", "x", PLAIN, [("vsom_row_sqnorm", "ldx")]),
    Far("bmu_manhattan_fwd-70x15x256", "x", PLAIN, [("vsom_bmu_manhattan_fwd", "ldx")]),
    Far("bmu_manhattan_fwd-33x100x48", "x", PLAIN, [("vsom_bmu_manhattan_fwd", "ldx")]),
    Far("som_bwd_manhattan", "x", PLAIN, [("vsom_som_bwd_manhattan", "ldx")]),
    Far("som_bwd_manhattan", "gX", PLAIN, [("vsom_som_bwd_manhattan", "ldgx")]),
    # ---- pca_contract: A and B as launch_gemm's; the output leaves through pca_reduce_kernel (`out[m * ldo + n]`, m long)
    Far("pca_project", "X", BUFFER, [("vsom_pca_project", "ldx")], "pca"), Far("pca_project", "B", BUFFER, [("vsom_pca_project", "ldb")], "pca"),
    Far("pca_project", "Y", PLAIN, [("vsom_pca_project", "ldy")]),
    Far("pca_backproject", "Y", BUFFER, [("vsom_pca_backproject", "ldy")], "pca"),
    Far("pca_backproject", "X", BUFFER, [("vsom_pca_backproject", "ldx")], "pca"),
    Far("pca_backproject", "Zt", PLAIN, [("vsom_pca_backproject", "ldz")]),
    # ---- the kNN family's tiles through F32Operand: extent N * ld * 4 against OOB - 256
    Far("knn_query", "Q", BUFFER, [("vsom_knn_query", "ldq")], "knn"), Far("knn_query", "X", BUFFER, [("vsom_knn_query", "ldx")], "knn"),
    Far("knn_ranks", "A", BUFFER, [("vsom_knn_ranks", "lda")], "knn"),
    Far("silhouette", "X", BUFFER, [("vsom_silhouette", "ldx")], "knn"),
    # ---- plain pointers again
    Far("som_batch_accumulate", "X", PLAIN, [("vsom_som_batch_accumulate", "ldx")]),
    Far("som_batch_update", "W_out", PLAIN, [("vsom_som_batch_update", "ldw")]),
    Far("kmeans_assign", "X", PLAIN, [("vsom_kmeans_assign", "ldx")]),
    Far("gmm_estep", "X", PLAIN, [("vsom_gmm_estep", "ldx")]), Far("gmm_estep", "resp", PLAIN, [("vsom_gmm_estep", "ldr")]),
    # ---- NEW_ROWS
    Far("rows_add", "src", PLAIN, [("vsom_rows_add", "lds")]), Far("rows_add", "dst", PLAIN, [("vsom_rows_add", "ldd")]),
    Far("argmax_rows", "x", PLAIN, [("vsom_argmax_rows", "ldx")]),
    Far("pca_colstats", "X", PLAIN, [("vsom_pca_colstats", "ldx")]),
    Far("pca_gram", "Zt", PLAIN, [("vsom_pca_gram", "ldz")]), Far("pca_gram", "B", PLAIN, [("vsom_pca_gram", "ldb")]),
    Far("pca_rotate", "Zt", PLAIN, [("vsom_pca_rotate", "ldz")]), Far("pca_rotate", "Bout", PLAIN, [("vsom_pca_rotate", "ldo")]),
    Far("pca_reconstruct", "Y", PLAIN, [("vsom_pca_reconstruct", "ldy")]), Far("pca_reconstruct", "B", PLAIN, [("vsom_pca_reconstruct", "ldb")]),
    Far("pca_reconstruct", "Xout", PLAIN, [("vsom_pca_reconstruct", "ldo")]),
    Far("kmeanspp_dist", "X", PLAIN, [("vsom_kmeanspp_dist", "ldx")]),
    Far("kmeans_colvar", "X", PLAIN, [("vsom_kmeans_colvar", "ldx")]),
    # ---- KNN_ROWS: the self contractions are F32Operand tiles (BUFFER, extent N * ld * 4); the matrix kernels read
    # `M + (size_t)i * ldm`, the direct distances `X + i * ldx` and `out + i * ldo` with 64-bit i
    Far("umap_knn", "X", BUFFER, [("vsom_umap_knn", "ldx")], "knn"),
    Far("dbscan_neighbours", "X", BUFFER, [("vsom_dbscan_neighbours", "ldx")], "knn"),
    Far("dbscan_threshold-f32", "M", PLAIN, [("vsom_dbscan_threshold", "ldm")]),
    Far("dbscan_threshold-f64", "M", PLAIN, [("vsom_dbscan_threshold", "ldm")]),
    Far("hdbscan_nearest", "X", BUFFER, [("vsom_hdbscan_nearest", "ldx")], "knn"),
    Far("hdbscan_nearest_matrix-f32", "M", PLAIN, [("vsom_hdbscan_nearest_matrix", "ldm")]),
    Far("hdbscan_nearest_matrix-f64", "M", PLAIN, [("vsom_hdbscan_nearest_matrix", "ldm")]),
    Far("agglo_distances", "X", PLAIN, [("vsom_agglo_distances", "ldx")]), Far("agglo_distances", "out", PLAIN, [("vsom_agglo_distances", "ldo")]),
    # ---- PLAIN_ROWS: `Z + i * ldz` and the like with 64-bit i throughout (linear_probe.hip, spectral.hip, tsne.hip, gmm.hip)
    Far("probe_fold", "B", PLAIN, [("vsom_probe_fold", "ldb")]),
    Far("probe_residual", "Z", PLAIN, [("vsom_probe_residual", "ldz")]), Far("probe_residual", "R", PLAIN, [("vsom_probe_residual", "ldr")]),
    Far("probe_linesearch", "Z", PLAIN, [("vsom_probe_linesearch", "ldz")], None, ("Zp",)),
    Far("probe_step", "Z", PLAIN, [("vsom_probe_step", "ldz")], None, ("Zp",)),
    Far("probe_gradient", "Zt", PLAIN, [("vsom_probe_gradient", "ldz")]),
    Far("spectral_rotate", "V", PLAIN, [("vsom_spectral_rotate", "ldv")]), Far("spectral_rotate", "out", PLAIN, [("vsom_spectral_rotate", "ldo")]),
    Far("spectral_embed", "V", PLAIN, [("vsom_spectral_embed", "ldv")]), Far("spectral_embed", "E", PLAIN, [("vsom_spectral_embed", "lde")]),
    Far("spectral_spmm", "Y1", (SAME, SAME, None), [("vsom_spectral_spmm", "ld")], None, ("Y0", "out")),
    Far("spectral_gram", "V", PLAIN, [("vsom_spectral_gram", "ld")], None, ("W",), True),
    Far("spectral_residual", "V", PLAIN, [("vsom_spectral_residual", "ld")], None, ("W",), True),
    Far("kmeans_relocate", "X", PLAIN, [("vsom_kmeans_relocate", "ldx")]),
    Far("tsne_affinities", "knn_dist", PLAIN, [("vsom_tsne_affinities", "ldk")]),
    Far("gmm_mstep", "X", PLAIN, [("vsom_gmm_mstep", "ldx")]), Far("gmm_mstep", "resp", PLAIN, [("vsom_gmm_mstep", "ldr")]),
]

FAR_BY_ROW = {}
for _f in TABLE:
    FAR_BY_ROW.setdefault(_f.row, []).append(_f)
FAR_ROWS = [ROW_BY_ID[i] for i in FAR_BY_ROW]


def op_of(row, name):
    return next(op for op in row.ops if op.name == name)


def shape_of(row, name):
    """(rows, cols, itemsize) of the operand `name` of `row`."""
    v = _case(row.id).t[name]
    return v.shape[0], v.shape[1], itemsize(v.dtype)


@functools.lru_cache(maxsize=None)
def _case(row_id):
    return ROW_BY_ID[row_id].make()


def variants(row):
    """[(label, {operand: window}, expected)]: each pitched operand alone in signed, wrapped, element, in that order, then all
    of them at once in signed (SAME: below every bound)."""
    out = []
    for f in FAR_BY_ROW[row.id]:
        for w, e in zip(WINDOWS, f.expect):
            if e is None:
                continue
            out.append((f"{f.op}@{w}", {n: w for n in (f.op,) + tuple(f.tied)}, e))
    if len(FAR_BY_ROW[row.id]) > 1:
        out.append((f"all@{SIGNED}", {n: SIGNED for f in FAR_BY_ROW[row.id] for n in (f.op,) + tuple(f.tied)}, SAME))
    return out


def arenas(row, moved):
    """[(operands, rows, columns, itemsize, window)]: the far arenas of a variant that moves `moved` = {operand: window} --
    one per operand, or one for a whole `wide` group, its columns side by side."""
    out = []
    for f in FAR_BY_ROW[row.id]:
        if f.op not in moved:
            continue
        names = (f.op,) + tuple(f.tied)
        if f.wide:
            rows, _, size = shape_of(row, f.op)
            assert all(shape_of(row, n)[0] == rows and shape_of(row, n)[2] == size for n in names)
            out.append((names, rows, sum(shape_of(row, n)[1] for n in names), size, moved[f.op]))
        else:
            out += [((n,),) + shape_of(row, n) + (moved[f.op],) for n in names]
    return out


def peak_bytes(row):
    """The largest sum of far arenas that a variant of `row` holds at once."""
    return max(sum(arena_bytes(r, c, size, w) for _, r, c, size, w in arenas(row, moved)) for _, moved, _ in variants(row))


# ------------------------------------------------------------------------------------------------------- left out
# (entry, parameter) -> why no row of the table moves it far away
LEFT_OUT = {
    ("vsom_bmu_cosine_form", "ldx"): "a host query of the launch plan: ldx enters `ldx % 4` only, no memory is touched",
    ("vsom_bmu_cosine_fwd", "ldx"): "vsom_bmu_cosine_dots followed by vsom_bmu_cosine_finalize in one call (som.hip), with no wrapper of "
                                    "its own: the bmu_cosine_fwd rows run the two entries it forwards to",
    ("vsom_linear_bwd_input_ln_partial", "lddy"): "the same host function (linear_bwd_input_ln_launch) and kernels as "
                                                  "vsom_linear_bwd_input_ln, which the table runs; its refusal is called on the host by "
                                                  "test_far_pitch_cpu.py",
}


# (entry, parameter, window) -> why that window alone is not run
WINDOW_LEFT_OUT = {
    ("vsom_spectral_spmm", "ld", ELEMENTW): "Y1, Y0 and Yout share one ld and the entry refuses blocks that overlap as byte ranges, so they cannot be "
                                            "column slices of one matrix: in `element` each block alone spans 16 GiB and the three, with "
                                            "their front guards, 96 GiB against the 40 GiB of the table (48 GiB with no guard at all)",
}


# ------------------------------------------------------------------------------------------------------- host refusals
P = 4096
REFUSING = [("vsom_bmu_cosine_x3_dots", "X"), ("vsom_bmu_cosine_x3_finalize", "X"), ("vsom_bmu_cosine_x3_planes_finalize", "X"),
            ("vsom_linear_bwd_input_ln", "dY"), ("vsom_linear_bwd_input_ln_partial", "dY")]


def host_refusals(L):
    """-> {(entry, operand): (code, words the message holds, rows, itemsize, cols, call(ld))}: every NO4GB operand as a call
    of the C entry with stand-in pointers and the row's own shape.  A refused call launches nothing: the refusal precedes
    every launch.  call(cols), the contiguous pitch, must not answer `code` -- and therefore goes on to launch, so the CPU
    test makes that call only where there is no device.  (The LayerNorm-fused entries want a split GEMM mode.)"""
    r = {}
    B, K, Ld = 70, 15, 256
    ws3 = L.vsom_bmu_cosine_x3_workspace_bytes(B, K, Ld)
    r[("vsom_bmu_cosine_x3_dots", "X")] = (EUNSUPPORTED, "4 GB", B, 4, Ld, lambda ld: L.vsom_bmu_cosine_x3_dots(P, ld, P, B, K, Ld, P, ws3, None))
    r[("vsom_bmu_cosine_x3_finalize", "X")] = (EUNSUPPORTED, "4 GB", B, 4, Ld,
                                                lambda ld: L.vsom_bmu_cosine_x3_finalize(P, ld, P, P, ws3, P, P, P, P, None, B, K, Ld, None))
    B2 = 192
    wsp = L.vsom_bmu_cosine_x3_planes_workspace_bytes(B2, K, Ld)
    r[("vsom_bmu_cosine_x3_planes_finalize", "X")] = (
        EUNSUPPORTED, "4 GB", B2, 4, Ld,
        lambda ld: L.vsom_bmu_cosine_x3_planes_finalize(P, ld, P, P, P, P, wsp, P, P, P, P, None, B2, K, Ld, None))
    M, N, Kk = 2048, 64, 192
    nb = 1 << 30
    r[("vsom_linear_bwd_input_ln", "dY")] = (
        EUNSUPPORTED, "4 GB", M, 4, N,
        lambda ld: L.vsom_linear_bwd_input_ln(P, ld, P, M, N, Kk, P, P, P, P, None, P, P, P, P, nb, None))
    r[("vsom_linear_bwd_input_ln_partial", "dY")] = (
        EUNSUPPORTED, "4 GB", M, 4, N,
        lambda ld: L.vsom_linear_bwd_input_ln_partial(P, ld, P, M, N, Kk, P, P, P, P, None, P, P, nb, None))
    return r


def planes_refusals(L):
    """The plane entries' 2 GB image bound: (entry) -> call(R) with L = 256; the image of R rows is cdiv(R, 32) * 32 KiB.  Stand-in
    pointers: a call that is refused launches nothing, one that is not would."""
    big = 1 << 40
    return {
        "vsom_bmu_planes_from": lambda R: L.vsom_bmu_planes_from(P, 256, R, 256, P, big, None),
        "vsom_adamw_step_planes": lambda R: L.vsom_adamw_step_planes(P, P, P, P, P, 1 << 32, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, 1, 0, R, 256, P,
                                                                     big, None),
    }


# entry -> words its comment in include/vitsom_hip.h must hold (the comment that ends last before the declaration)
HEADER_REFUSES = {
    "vsom_bmu_cosine_x3_dots": ["4 GB", "VSOM_EUNSUPPORTED", "vsom_bmu_cosine_x3_finalize"],
    "vsom_bmu_planes_from": ["2 GB", "4 GB", "VSOM_EUNSUPPORTED", "vsom_bmu_cosine_x3_planes_finalize"],
    "vsom_linear_bwd_input_ln": ["4 GB", "VSOM_EUNSUPPORTED"],
}
FALLBACK_WORDS = "4 GB or more take the element-wise loads"
# entry that falls back -> the entry whose comment says so (its own, or one that names it with the sentence)
_GEMM_ENTRIES = ["vsom_linear_fwd", "vsom_linear_gelu_fwd", "vsom_linear_relu_fwd", "vsom_linear_residual_fwd", "vsom_linear_bwd_input",
                 "vsom_linear_bwd_input_t", "vsom_linear_bwd_weight", "vsom_som_bwd", "vsom_bmu_cosine_dots", "vsom_bmu_euclid_fwd"]
HEADER_FALLS_BACK = {**{e: "vsom_linear_fwd" for e in _GEMM_ENTRIES}, "vsom_pca_project": "vsom_pca_project",
                     "vsom_pca_backproject": "vsom_pca_backproject", "vsom_knn_query": "vsom_knn_query",
                     "vsom_knn_ranks": "vsom_knn_ranks", "vsom_silhouette": "vsom_silhouette", "vsom_umap_knn": "vsom_umap_knn",
                     "vsom_dbscan_neighbours": "vsom_dbscan_neighbours", "vsom_hdbscan_nearest": "vsom_hdbscan_nearest"}
