"""Inputs at the numerical edges of the evaluation kernels -- the kNN search in both modes, the neighbour ranks, the
softmax vote, the k-means steps and the linear probe's residual -- in the conventions of numeric_edges.py, whose helpers
(make_case, bound, accepts, FACTOR, E32_MAX) are used here: a case holds inp, ref (fp64), y32 (plain fp32 torch), e32 and
prop, and a kernel's error passes when it is <= max(FLOOR, FACTOR * e32), FLOOR being the tolerance the entry point's
own GPU test uses on N(0, 1) data.  Pure torch / numpy on the CPU: tests/test_eval_edges_cpu.py checks the cases and
that the comparisons reject three deliberately wrong formulations, tests/test_eval_edges_gpu.py runs the cases through
vit_som_amd.ops.

What model outputs bring that N(0, 1) rows do not: a large common offset (rows = 1000 + noise), wide latents (euclidean
distances in the hundreds), rows scaled by powers of two, and a few BAD rows -- a NaN, an infinity, or finite elements
whose squared norm overflows fp32.  The bad-row contract ("kNN"): a pair with a bad row has no distance, so
a bad bank row is in nobody's list, a bad query's list is empty, and every other list is bit for bit that of the call
with the bad rows deleted."""
import functools
import math

import numpy as np
import torch

import knn_checks as KC
import knn_ref as R
from numeric_edges import CE_KINDS, E32_MAX, FACTOR, accepts, bound, ce_case, make_case, max_abs, rnd  # noqa: F401  (re-exported)

METRICS = ("cosine", "euclidean")
METRIC_ID = {"cosine": R.COSINE, "euclidean": R.EUCLIDEAN}
BAD_KINDS = ["nan", "inf", "overflow", "mixed"]
OVERFLOW_SCALE = 1e20                            # finite elements, a squared norm far above 3.4e38
# the tolerances of the entry points' own GPU tests (none is taken from the code under test)
FLOOR = {"knn": KC.FLOOR,                        # test_knn_gpu.py::test_query_against_fp64 (see knn_checks.FLOOR)
         "vote": 1e-12,                          # test_vote_softmax: relative to the scores
         "kmeans": 1e-5,                         # test_assign_update_against_oracle: mind (rtol + atol * max) and the inertia
         "probe_R": 2.0 ** -23,                  # test_residual_against_fp64
         "probe_loss": 1e-12}


def _f32(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32)


def poison_rows(M, rows, kind, seed=0):
    """Turn `rows` of M (in place) into bad rows of `kind`; `mixed` cycles through nan, inf and overflow."""
    for n, r in enumerate(rows):
        which = kind if kind != "mixed" else ("nan", "inf", "overflow")[n % 3]
        col = (seed + 7 * n) % M.shape[1]
        if which == "nan":
            M[r, col] = math.nan
        elif which == "inf":
            M[r, col] = math.inf if n % 2 == 0 else -math.inf
        else:
            M[r] = M[r] * OVERFLOW_SCALE
    return M


def rows_are_bad(M):
    """fp32 view of a row set: the rows whose squared norm, summed in fp32, is not a finite number."""
    return ~torch.isfinite((M * M).sum(1))


# ------------------------------------------------------------------------------------------------------------ kNN search
# (Nq, Nb, D, k).  tiles: two query row blocks with a ragged second one, five 64-column tiles with a 1-column tail, several
# column chunks into the merge, a k-loop tail (D = 40 = 32 + 8).  elementwise: D = 3 takes the element-wise loads.
KNN_SHAPES = {"tiles": (130, 257, 40, 20), "elementwise": (130, 257, 3, 2)}
UMAP_N, UMAP_D, UMAP_K = 257, 40, 20
OFFSET = 1000.0
N_COPIES = 8


def bad_rows(Nq, Nb):
    """(bad query rows, bad bank rows): the first and last query; bank rows at both ends and on both sides of a tile edge."""
    return [0, Nq - 1], [0, 63, 64, Nb - 1]


def distance_eval(Q, X, metric, dtype):
    """The checked quantity (knn_checks.FLOOR) in `dtype`: the squared euclidean distance as |q|^2 + |x|^2 - 2 q.x, the
    cosine distance as 1 - q.x / (|q| |x|); with the two squared norms."""
    Ql, Xl = Q.to(dtype), X.to(dtype)
    sqq, sqx = (Ql * Ql).sum(1), (Xl * Xl).sum(1)
    G = Ql @ Xl.T
    if metric == "euclidean":
        return (sqq[:, None] + sqx[None, :] - 2.0 * G).clamp_min(0.0), sqq, sqx
    return 1.0 - G / (sqq.sqrt()[:, None] * sqx.sqrt()[None, :]), sqq, sqx


def matrix_error(metric, sqq, sqx):
    """The error of a whole distance matrix in the unit of the tolerance (euclidean: relative to |q|^2 + |x|^2)."""
    scale = (sqq[:, None] + sqx[None, :]).double().clamp_min(1e-300) if metric == "euclidean" else 1.0

    def err(a, ref):
        return float(((torch.as_tensor(a).double() - ref).abs() / scale).max())
    return err


def _search_case(name, Q, X, k, metric, bad_q, bad_x, self_mode, extra_inp=None, extra_prop=None):
    """The case of one search: ref / y32 hold the distance matrix of the GOOD rows (queries `good`, bank rows `keep`)."""
    good = torch.ones(Q.shape[0], dtype=torch.bool)
    good[bad_q] = False
    keep = torch.ones(X.shape[0], dtype=torch.bool)
    keep[bad_x] = False
    Qg, Xk = Q[good].contiguous(), X[keep].contiguous()
    d64, sqq, sqx = distance_eval(Qg, Xk, metric, torch.float64)
    d32, _, _ = distance_eval(Qg, Xk, metric, torch.float32)
    clear, _ = KC.clear_rows(d64, sqq, sqx, k, metric)
    prop = {"bad_rows_are_exactly_the_bad_rows": bool(torch.equal(rows_are_bad(X), ~keep) and torch.equal(rows_are_bad(Q), ~good)),
            "good_rows_are_finite": bool(torch.isfinite(d64).all()),
            "bank_exceeds_k": int(keep.sum()) > k}
    prop.update(extra_prop or {})
    inp = {"Q": Q, "X": X, "k": k, "metric": metric, "bad_q": list(bad_q), "bad_x": list(bad_x), "good": good, "keep": keep,
           "Qg": Qg, "Xk": Xk, "self_mode": self_mode}
    inp.update(extra_inp or {})
    c = make_case(name, inp, {"d": d64}, {"d": d32}, {"d": matrix_error(metric, sqq, sqx)}, prop)
    c.clear_share = float(clear.double().mean())
    return c


@functools.lru_cache(maxsize=None)
def knn_bad_case(shape, kind, metric):
    Nq, Nb, D, k = KNN_SHAPES[shape]
    bad_q, bad_x = bad_rows(Nq, Nb)
    Q, X = poison_rows(rnd(Nq, D, seed=1), bad_q, kind, seed=3), poison_rows(rnd(Nb, D, seed=2), bad_x, kind, seed=5)
    return _search_case(f"knn-{shape}-{kind}-{metric}", Q, X, k, metric, bad_q, bad_x, False)


@functools.lru_cache(maxsize=None)
def umap_bad_case(kind, metric):
    _, bad = bad_rows(UMAP_N, UMAP_N)
    X = poison_rows(rnd(UMAP_N, UMAP_D, seed=3), bad, kind, seed=5)
    return _search_case(f"umap-{kind}-{metric}", X, X, UMAP_K, metric, bad, bad, True)


def _offset_dup(Nq, Nb, D, self_mode):
    """rows = 1000 + N(0, 1); N_COPIES bank rows that are bitwise copies of queries (self mode: of other rows); two
    pairs of identical bank rows, the first of them a pair of copies of one query."""
    X = OFFSET + rnd(Nb, D, seed=12)
    Q = X if self_mode else OFFSET + rnd(Nq, D, seed=11)
    g = torch.Generator().manual_seed(13)
    qs = (torch.randperm(Nq, generator=g)[:N_COPIES] if not self_mode else torch.arange(3, 3 + 5 * N_COPIES, 5)).tolist()
    bs = [65 + 23 * n for n in range(N_COPIES)]                      # 65 .. 226: distinct, none of them a query row in self mode
    assert len(set(qs)) == N_COPIES and max(bs) < Nb - 2 and not (self_mode and set(bs) & set(qs))
    for q, b in zip(qs, bs):
        X[b] = Q[q]
    pairs = [(bs[0], bs[0] + 1), (10, 200)]                          # X[66] := X[65] (both copies of query qs[0]); X[200] := X[10]
    for p0, p1 in pairs:
        X[p1] = X[p0]
    return Q, X, list(zip(qs, bs)), pairs


@functools.lru_cache(maxsize=None)
def offset_dup_case(metric, self_mode=False):
    Nq, Nb, D, k = (UMAP_N, UMAP_N, UMAP_D, UMAP_K) if self_mode else KNN_SHAPES["tiles"]
    Q, X, copies, pairs = _offset_dup(Nq, Nb, D, self_mode)
    prop = {"offset": float(X.mean()) > 990 and float(Q.mean()) > 990,
            "copies_are_bitwise": all(torch.equal(X[b], Q[q]) for q, b in copies),
            "pairs_are_bitwise": all(torch.equal(X[p0], X[p1]) for p0, p1 in pairs)}
    return _search_case(f"{'umap' if self_mode else 'knn'}-offset_dup-{metric}", Q, X, k, metric, [], [], self_mode,
                        {"copies": copies, "pairs": pairs}, prop)


@functools.lru_cache(maxsize=None)
def pow2_case(self_mode=False):
    """Cosine only: every row scaled by 2^e, e in [-40, 40].  Products, sums, square roots and the quotient all scale
    exactly, so lists and distances are those of the unscaled rows bit for bit."""
    Nq, Nb, D, k = (UMAP_N, UMAP_N, UMAP_D, UMAP_K) if self_mode else KNN_SHAPES["tiles"]
    g = torch.Generator().manual_seed(17)
    X0 = rnd(Nb, D, seed=2)
    ex = torch.randint(-40, 41, (Nb,), generator=g)
    X = X0 * torch.exp2(ex.float())[:, None]
    if self_mode:
        Q0, Q = X0, X
    else:
        Q0 = rnd(Nq, D, seed=1)
        Q = Q0 * torch.exp2(torch.randint(-40, 41, (Nq,), generator=g).float())[:, None]
    plain, _, _ = distance_eval(Q0, X0, "cosine", torch.float64)
    scaled, _, _ = distance_eval(Q, X, "cosine", torch.float64)
    sq = (X.double() ** 2).sum(1)
    prop = {"scaling_is_exact_in_fp64": bool(torch.equal(plain, scaled)),
            "exponents_span_the_range": int(ex.min()) <= -38 and int(ex.max()) >= 38,
            "norms_inside_fp32": float(sq.max()) < 3e38 and float(sq.min()) > 1.2e-38}
    return _search_case(f"{'umap' if self_mode else 'knn'}-pow2", Q, X, k, "cosine", [], [], self_mode, {"Q0": Q0, "X0": X0}, prop)


# The search restated in fp32 torch, for test_eval_edges_cpu.py: knn.hip's knn_distance and the (distance, index) lists.
def kernel_distance32(Q, X, metric, clamp_swallows_nan=False, self_mode=False):
    """knn_distance in fp32 -> [Nq, Nb], NaN where a pair has no distance.  clamp_swallows_nan=True: the defect, the clamp
    fmaxf(x, 0) applied to a NaN (it answers 0) with no test before it."""
    # every pair summed over D in one fixed order, whatever the sizes of the two sets (a BLAS matmul does not promise that)
    G = torch.zeros(Q.shape[0], X.shape[0])
    sqq, sqx = torch.zeros(Q.shape[0]), torch.zeros(X.shape[0])
    for j in range(Q.shape[1]):
        G += Q[:, j, None] * X[None, :, j]
        sqq += Q[:, j] * Q[:, j]
        sqx += X[:, j] * X[:, j]
    nan = torch.full_like(G, math.nan)

    def fmaxf0(t):                               # fmaxf(t, 0): the number when the other operand is a NaN
        return torch.where(torch.isnan(t), torch.zeros_like(t), t.clamp_min(0.0))
    if metric == "euclidean":
        d2 = sqq[:, None] + sqx[None, :] - 2.0 * G
        d = fmaxf0(d2).sqrt() if clamp_swallows_nan else torch.where(d2.abs() < math.inf, d2.clamp_min(0.0).sqrt(), nan)
    else:
        c = 1.0 - G / (sqq.sqrt()[:, None] * sqx.sqrt()[None, :])
        zq, zx = (sqq == 0)[:, None], (sqx == 0)[None, :]
        if clamp_swallows_nan:
            d = fmaxf0(c)
        else:
            ok = torch.isfinite(sqq)[:, None] & torch.isfinite(sqx)[None, :] & (G.abs() < math.inf)
            d = torch.where(ok, c.clamp_min(0.0), nan)
            zq, zx = zq & ok, zx & ok
        d = torch.where(zq & zx, torch.zeros_like(d), torch.where(zq | zx, torch.ones_like(d), d))
    same = (Q[:, None, :] == X[None, :, :]).all(-1)                  # identical finite rows: exactly 0 (the shared summation order)
    d = torch.where(same, torch.zeros_like(d), d)
    if self_mode:
        d.fill_diagonal_(-1.0)                   # row i first in its own list; written out as 0
    return d


def lists32(d, k, list_inf=False):
    """The k smallest of every row by (distance, index) -> (idx int64, dist f32); a NaN is never listed and, unless
    list_inf (the merge before the fix: +inf carried a real index), neither is +inf; empty slots are (-1, +inf)."""
    key = torch.where(torch.isnan(d), torch.full_like(d, math.inf), d)
    order = torch.argsort(key, dim=1, stable=True)[:, :k]
    dist = d.gather(1, order)
    empty = torch.isnan(dist) | (torch.isinf(dist) & (not list_inf))
    idx = torch.where(empty, torch.full_like(order, -1), order)
    dist = torch.where(empty, torch.full_like(dist, math.inf), dist.clamp_min(0.0))
    return idx, dist


def restated_search(Q, X, k, metric, self_mode=False, clamp_swallows_nan=False):
    d = kernel_distance32(Q, X, metric, clamp_swallows_nan, self_mode)
    return lists32(d, k, list_inf=clamp_swallows_nan)


def bits_equal(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def bad_row_contract(idx, dist, idx_del, dist_del, inp):
    """The bad-row contract of a search's lists (idx, dist) over all queries and the whole bank, given the lists
    (idx_del, dist_del) of the good queries over the bank with the bad rows deleted -> the violated clauses (none: kept)."""
    idx, dist, idx_del, dist_del = idx.cpu(), dist.cpu(), idx_del.cpu(), dist_del.cpu()
    broken = []
    listed = (idx >= 0) & torch.isfinite(dist) & (dist >= 0)
    empty = (idx == -1) & (dist == math.inf)
    if not bool((listed | empty).all()):
        broken.append("an entry is neither (index >= 0, finite distance >= 0) nor the empty slot (-1, +inf)")
    bad_x = torch.tensor(inp["bad_x"], dtype=torch.int64)
    hit = torch.isin(idx, bad_x)
    for i in inp["bad_q"]:
        row_ok = bool((idx[i] == -1).all() and (dist[i] == math.inf).all())
        if inp["self_mode"]:
            hit[i, 0] = False                    # the row itself, which self mode puts first at 0
            row_ok = int(idx[i, 0]) == i and float(dist[i, 0]) == 0.0 and bool((idx[i, 1:] == -1).all() and (dist[i, 1:] == math.inf).all())
        if not row_ok:
            broken.append(f"bad query {i} has a list")
    if bool(hit.any()):
        broken.append(f"a bad bank row is listed ({int(hit.sum())} times)")
    ids = torch.nonzero(inp["keep"]).squeeze(1)
    mapped = torch.where(idx_del >= 0, ids[idx_del.clamp_min(0)], torch.full_like(idx_del, -1))
    if not (torch.equal(idx[inp["good"]], mapped) and bits_equal(dist[inp["good"]], dist_del)):
        broken.append("a good query's list differs from the call with the bad rows deleted")
    return broken


def offset_dup_violations(idx, dist, inp):
    """offset_dup's exact clauses -> (the violated ones, the number of lists that hold both rows of an identical pair): a
    query's copies come first, in index order, at distance exactly 0 (self mode: after the row itself), and nothing else
    is at 0; identical bank rows stand next to each other, lower index first, at the same distance bit for bit."""
    idx, dist = idx.cpu(), dist.cpu()
    broken, together = [], 0
    heads = {}
    for q, b in inp["copies"]:
        heads.setdefault(q, []).append(b)
    for p0, p1 in inp["pairs"]:
        for bs in heads.values():
            if p0 in bs:
                bs.append(p1)
    for q, bs in heads.items():
        want = ([q] if inp["self_mode"] else []) + sorted(bs)
        n = len(want)
        if idx[q, :n].tolist() != want or bool((dist[q, :n] != 0).any()) or not float(dist[q, n]) > 0:
            broken.append(f"query {q}: the list begins {idx[q, :n + 1].tolist()} at {dist[q, :n + 1].tolist()}, wanted {want} at 0")
    for p0, p1 in inp["pairs"]:
        for i in range(idx.shape[0]):
            if inp["self_mode"] and i in (p0, p1):
                continue                         # the row itself goes first, whatever its index
            row = idx[i].tolist()
            a, b = (row.index(p) if p in row else -1 for p in (p0, p1))
            if a < 0 and b < 0:
                continue
            # at an offset of 1000 the fp32 distances are coarse and other rows tie with the pair: they may stand between
            # the two, or cut the second one off at the end of the list -- at the pair's distance, never at another
            if a >= 0 and b >= 0:
                ok = a < b and bits_equal(dist[i, a:a + 1], dist[i, b:b + 1])
                together += ok
            else:
                ok = a >= 0 and bits_equal(dist[i, a:a + 1], dist[i, -1:])
            if not ok:
                broken.append(f"query {i}: identical rows {p0}, {p1} are not listed in index order at one distance")
    return broken, together


# ------------------------------------------------------------------------------------------------------------ neighbour ranks
RANKS_N, RANKS_D, RANKS_K = 257, 12288, 15       # test_embedding_quality_gpu.py::test_ranks_against_fp64


@functools.lru_cache(maxsize=None)
def ranks_case(kind):
    """That test's rows and neighbour table (from a random 2-D embedding) with bad rows; nbr_del: the table of the set with
    the bad rows deleted -- its rows renumbered, a slot that named a bad row empty."""
    import embedding_quality_ref as Q
    rng = np.random.default_rng(1)
    X = _f32(rng.standard_normal((RANKS_N, RANKS_D)))
    E = rng.standard_normal((RANKS_N, 2))
    nbr = torch.as_tensor(Q.neighbours(np.sqrt(((E[:, None] - E[None]) ** 2).sum(-1)), RANKS_K), dtype=torch.int64)
    _, bad = bad_rows(RANKS_N, RANKS_N)
    poison_rows(X, bad, kind, seed=5)
    keep = torch.ones(RANKS_N, dtype=torch.bool)
    keep[bad] = False
    new_id = torch.cumsum(keep.long(), 0) - 1
    names_good = keep[nbr]                                           # [N, k]: the slot names a good row
    nbr_del = torch.where(names_good, new_id[nbr], torch.full_like(nbr, -1))[keep].contiguous()
    prop = {"bad_rows_are_exactly_the_bad_rows": bool(torch.equal(rows_are_bad(X), ~keep)),
            "good_rows_name_bad_rows": bool((~names_good[keep]).any()),
            "most_slots_remain": float(names_good[keep].double().mean()) > 0.9}
    return make_case(f"ranks-{kind}", {"X": X, "nbr": nbr, "keep": keep, "bad": bad, "names_good": names_good, "nbr_del": nbr_del,
                                       "Xk": X[keep].contiguous()}, {}, {}, {}, prop)


# ------------------------------------------------------------------------------------------------------------ softmax vote
VOTE_NQ, VOTE_K, VOTE_CLASSES, VOTE_BANK, VOTE_T = 130, 20, 10, 500, 0.07
VOTE_RANGES = {"euclidean_range": (90.0, 160.0), "cosine_control": (0.0, 2.0)}
VOTE_PRED_GAP = 1e-9


def vote_eval(idx, dist, labels, T, dtype, shift=True):
    """Softmax vote -> (normalised scores [Nq, C], raw scores).  shift=False: exp(-d / T) as it stands."""
    d = dist.to(dtype)
    T = torch.tensor(T, dtype=torch.float32).to(dtype)
    z = -(d - d.min(1, keepdim=True).values) / T if shift else -d / T
    w = z.exp()
    raw = torch.zeros(idx.shape[0], VOTE_CLASSES, dtype=dtype).scatter_add_(1, labels[idx], w)
    return raw / raw.sum(1, keepdim=True), raw


@functools.lru_cache(maxsize=None)
def vote_case(kind):
    lo, hi = VOTE_RANGES[kind]
    g = torch.Generator().manual_seed(23)
    idx = torch.stack([torch.randperm(VOTE_BANK, generator=g)[:VOTE_K] for _ in range(VOTE_NQ)])
    dist = (lo + (hi - lo) * torch.rand(VOTE_NQ, VOTE_K, generator=g)).sort(1).values          # stored f32 distances
    labels = torch.randint(0, VOTE_CLASSES, (VOTE_BANK,), generator=g)
    ref, raw = vote_eval(idx, dist, labels, VOTE_T, torch.float64)
    y32, _ = vote_eval(idx, dist, labels, VOTE_T, torch.float32)
    top = ref.sort(1).values
    clear = (top[:, -1] - top[:, -2]) > VOTE_PRED_GAP
    plain = vote_eval(idx, dist, labels, VOTE_T, torch.float64, shift=False)[1]
    prop = {"distances_in_range": float(dist.min()) >= lo and float(dist.max()) <= hi,
            "most_queries_are_decided": float(clear.double().mean()) >= 0.9,
            "several_classes_win": len(set(ref.argmax(1).tolist())) >= 5,
            "unshifted_weights_underflow": kind != "euclidean_range" or bool((plain == 0).all()),
            "nearest_neighbour_weighs_one": bool((raw.max(1).values >= 1.0).all())}
    return make_case(f"vote-{kind}", {"idx": idx, "dist": dist, "labels": labels, "clear": clear},
                     {"scores": ref, "pred": ref.argmax(1)}, {"scores": y32}, {"scores": max_abs}, prop)


# ------------------------------------------------------------------------------------------------------------ k-means
# (N, D, k) of test_kmeans_gpu.py::test_assign_update_against_oracle: D = 784 takes the 16-byte loads, D = 10 the element path
KMEANS_SHAPES = [(2000, 784, 10), (777, 10, 7)]
KMEANS_KINDS = ["offset", "nan", "overflow"]
# 1000 separates the two forms at both shapes: the fp32 expansion |x|^2 + |c|^2 - 2 x.c carries ulp(D 1e6) -- 64 at D = 784,
# 1 at D = 10 -- against squared distances of 1e3 and 1e1, ten thousand times the bound; the differences x - c are exact
KMEANS_OFFSET = 1000.0
KMEANS_CLEAR = 1e-4                              # test_kmeans_gpu._check_iteration: gap > 1e-4 mind


def kmeans_data(seed, N, D, k):
    """test_kmeans_gpu._data."""
    g = torch.Generator().manual_seed(seed)
    means = torch.randn(k, D, generator=g) * 2.0
    X = means[torch.randint(0, k, (N,), generator=g)] + torch.randn(N, D, generator=g)
    return X, torch.randperm(N, generator=g)[:k]


def kmeans_bad_rows(N):
    """One in the first workgroup's row range, one in the last's."""
    return [1, N - 2]


def kmeans_eval(X, C, cand, closest, dtype, expansion=False):
    """Squared distances [N, k] as sums of squared differences (the kernel's documented form; expansion=True: as
    |x|^2 + |c|^2 - 2 x.c), the k-means++ distances / potentials of the candidate rows, mean(var(X, axis=0))."""
    Xl, Cl = X.to(dtype), C.to(dtype)
    if expansion:
        d = ((Xl * Xl).sum(1)[:, None] + (Cl * Cl).sum(1)[None, :] - 2.0 * (Xl @ Cl.T)).clamp_min(0.0)
    else:
        d = torch.stack([((Xl - Cl[j]) ** 2).sum(1) for j in range(C.shape[0])], dim=1)
    pp = torch.stack([torch.minimum(closest.to(dtype), ((Xl - Xl[t]) ** 2).sum(1)) for t in cand.tolist()])
    return {"d": d, "pp": pp, "pots": pp.double().sum(1), "colvar": Xl.var(0, unbiased=False).mean().double().reshape(1)}


def mind_error(a, ref):
    """_check_iteration's allclose(mind, own, rtol, atol = rtol max(own)) as one number: |a - ref| / (|ref| + max |ref|)."""
    a, ref = torch.as_tensor(a).double(), torch.as_tensor(ref).double()
    return float(((a - ref).abs() / (ref.abs() + ref.abs().max()).clamp_min(1e-300)).max())


def rel_max(a, ref):
    a, ref = torch.as_tensor(a).double(), torch.as_tensor(ref).double()
    return float(((a - ref).abs() / ref.abs().clamp_min(1e-300)).max())


def kmeans_labels(d):
    """(first argmin, its distance, the gap to the runner-up) of a distance matrix."""
    two = torch.topk(d.double(), min(2, d.shape[1]), dim=1, largest=False).values
    gap = two[:, 1] - two[:, 0] if d.shape[1] > 1 else torch.full((d.shape[0],), math.inf, dtype=torch.float64)
    lab = d.argmin(1)
    return lab, d.gather(1, lab[:, None]).squeeze(1), gap


@functools.lru_cache(maxsize=None)
def kmeans_case(i, kind):
    N, D, k = KMEANS_SHAPES[i]
    X, rows = kmeans_data(N + D + k, N, D, k)
    if kind == "offset":
        X = X + KMEANS_OFFSET
    C = X[rows].clone()                                              # centres are rows of the data, offset included
    bad = [] if kind == "offset" else kmeans_bad_rows(N)
    X_good = X.clone()
    poison_rows(X, bad, kind, seed=5)
    cand = torch.tensor([0, N // 2, N - 3], dtype=torch.int64)
    closest = ((X_good - X_good[5]) ** 2).sum(1)                     # the running minimum after one centre (row 5)
    ref = kmeans_eval(X_good, C, cand, closest, torch.float64)
    y32 = kmeans_eval(X_good, C, cand, closest, torch.float32)
    lab, mind, gap = kmeans_labels(ref["d"])
    ref.update(labels=lab, mind=mind)
    y32["mind"] = y32["d"].gather(1, lab[:, None]).squeeze(1)       # the same question: the distance to the fp64 centre
    clear = gap > KMEANS_CLEAR * mind.clamp_min(1e-30)
    prop = {"centres_are_rows": bool(torch.equal(C, X_good[rows])), "no_centre_is_a_bad_row": not set(rows.tolist()) & set(bad),
            "candidates_are_good_rows": not set(cand.tolist()) & set(bad)}
    if kind == "offset":
        prop["offset"] = float(X.mean()) > 990
    else:
        prop["bad_rows_are_exactly_the_bad_rows"] = rows_are_bad(X).nonzero().squeeze(1).tolist() == bad
    c = make_case(f"kmeans-{N}x{D}x{k}-{kind}", {"X": X, "X_good": X_good, "C": C, "cand": cand, "closest": closest, "bad": bad,
                                                 "clear": clear}, ref, y32,
                  {"mind": mind_error, "pp": mind_error, "pots": rel_max, "colvar": rel_max}, prop)
    c.clear_share = float(clear.double().mean())
    return c


# ------------------------------------------------------------------------------------------------------------ linear probe
PROBE_CLASSES = [10, 65]


@functools.lru_cache(maxsize=None)
def probe_case(C, kind):
    """numeric_edges.ce_case(C, 0.0, kind) as the logits Z of vsom_probe_residual with a zero intercept: the summed cross
    entropy, R = softmax - onehot, and the first argmax."""
    ce = ce_case(C, 0.0, kind)
    z, y = ce.inp["z"], ce.inp["y"]
    pred = torch.as_tensor(np.argmax(z.double().numpy(), axis=1))    # numpy: the FIRST maximum
    ref = {"loss": ce.ref["loss"], "R": ce.ref["dlogits"], "pred": pred}
    y32 = {"loss": ce.y32["loss"], "R": ce.y32["dlogits"]}
    prop = dict(ce.prop)
    prop["rows_of_R_sum_to_zero"] = float(ref["R"].sum(1).abs().max()) < 1e-12
    return make_case(f"probe-C{C}-{kind}", {"Z": z, "y": y, "b": torch.zeros(C, dtype=torch.float64)}, ref, y32,
                     {"loss": rel_max, "R": max_abs}, prop)
