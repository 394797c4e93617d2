"""On-device HDBSCAN (csrc/knn.hip's HDBSCAN section, vit_som_amd/hdbscan.py) at the smallest shapes at which the kernels can
still go wrong: the spanning tree edge for edge and bit for bit against Kruskal / Prim under (w, lo, hi) on integer data,
where the device's fp32 distances are exact and ties abound; tile, word and chunk edges; real-valued fixtures against fp64
and sklearn; hand-built cases, invariances, guarded buffers and misaligned operands, bad rows, precomputed input and the
evaluation path."""
import copy
import math
import signal

import numpy as np
import pytest
import torch

import dbscan_ref
import hdbscan_ref as R
import memcheck
import silhouette_ref as SR
from helpers import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COSINE, EUCLIDEAN = R.COSINE, R.EUCLIDEAN
NAMES = {COSINE: "cosine", EUCLIDEAN: "euclidean"}
SHAPES = [(257, 12288), (333, 1003), (130, 3)]        # two row blocks + 1 and 16-byte loads; element-wise loads; tiny D
UNTIED = {(257, 12288, COSINE), (333, 1003, EUCLIDEAN), (130, 3, EUCLIDEAN)}     # test_two_fits_row_order_and_scaling: measured
FLOOR = 1e-5          # knn_checks.FLOOR: cosine absolute on the distance; euclidean on the squared distance, relative to the norms


@pytest.fixture(autouse=True)
def time_limit(request):
    """A limit of its own (seconds) for every test here, as in test_dbscan_gpu.py: a SIGALRM handler ends a test whose
    host side is slow or loops."""
    limit = 300 if "driver" in request.node.name or "ranks" in request.node.name else 120

    def expired(signum, frame):
        raise TimeoutError(f"{request.node.name}: no result after {limit} s")
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(limit)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _fit(X, mcs=5, ms=None, metric="euclidean", **kw):
    from vit_som_amd import HDBSCAN
    X = X if isinstance(X, torch.Tensor) else _dev(X)
    return HDBSCAN(min_cluster_size=mcs, min_samples=ms, metric=metric, **kw).fit(X)


def _edges(hd):
    """(lo int64, hi int64, w float32) of a fitted estimator, in the order (w, lo, hi)."""
    t = hd.minimum_spanning_tree_
    assert t.dtype == np.float64 and t.shape == (len(t), 3)
    w = t[:, 2].astype(np.float32)
    assert np.array_equal(w.astype(np.float64), t[:, 2])             # the weights are fp32 values
    return t[:, 0].astype(np.int64), t[:, 1].astype(np.int64), w


def _same_edges(got, want):
    """Edge for edge, weight bit for bit."""
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[2].dtype == want[2].dtype == np.float32 and np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32))


def _exact_tree(X, ms):
    """(the exact fp32 distances of integer rows, their core distances, the tree of their mutual reachability)."""
    D32, _ = SR.exact_euclidean32(X)
    W, core = R.mutual_reachability(D32, ms)
    assert W.dtype == np.float32
    return D32, core, R.prim(W)


def _check_exact(X, ms, mcs=5, **kw):
    D32, core, want = _exact_tree(X, ms)
    hd = _fit(X, mcs, ms, **kw)
    assert np.array_equal(hd.core_distances_.cpu().numpy(), core)
    _same_edges(_edges(hd), want)
    N = X.shape[0]
    assert 1 <= hd.n_rounds_ <= max(1, math.ceil(math.log2(N)))
    naive = R.naive_hdbscan(*want, N, mcs, allow_single_cluster=kw.get("allow_single_cluster", False))
    assert np.array_equal(hd.labels_.cpu().numpy(), naive[0])
    assert np.abs(hd.probabilities_.cpu().numpy() - naive[1]).max() <= 2.0 ** -24
    return hd


# ------------------------------------------------------------------ (4) exact on integer data
@pytest.mark.parametrize("ms", [2, 5])
@pytest.mark.parametrize("N,D", SHAPES)
def test_exact_on_integer_data(N, D, ms):
    """Every squared distance is an integer exact in fp32 and sqrtf is correctly rounded: the device's distances ARE
    exact_euclidean32's and ties abound.  core_distances_ is the sorted-row column of the exact matrix, and the N - 1 edges are
    those of the restatement under (w, lo, hi), edge for edge, weight bit for bit: this pins the order and cycle-freedom."""
    from test_silhouette_gpu import _integers
    hd = _check_exact(_integers(N, D, 5), ms)
    lo, hi, w = _edges(hd)
    assert R.is_spanning_tree(lo, hi, N)
    assert hd.labels_.dtype == torch.int64 and hd.probabilities_.dtype == torch.float32 and hd.n_features_in_ == D
    assert hd.single_linkage_tree_.shape == (N - 1, 4) and hd.condensed_tree_.dtype.names == ("parent", "child", "value", "cluster_size")
    assert hd.n_clusters_ == int(hd.labels_.max()) + 1 == len(hd.cluster_persistence_) and hd.n_noise_ == int((hd.labels_ < 0).sum())


# ------------------------------------------------------------------ (5) tile, word and chunk edges
@pytest.mark.parametrize("N", [2, 64, 65, 128, 129, 191, 3000, 4300])
def test_tile_word_and_chunk_edges(N):
    """Tile edges (N = 2 .. 191) and the two chunk regimes test_dbscan_gpu.py names: N = 3000 runs one tile per chunk,
    N = 4300 is the first size range at which a chunk holds more than one.  D = 8 takes the 16-byte loads."""
    X = np.random.default_rng(N).integers(0, 32, (N, 8))
    hd = _check_exact(X, 1 if N == 2 else 2, mcs=2 if N == 2 else 5)
    assert N < 3000 or len(np.unique(_edges(hd)[2])) < (N - 1) // 2      # coordinates in 0 .. 31: the tree's weights tie


# ------------------------------------------------------------------ (6) real-valued fixtures
def _fp64_and_e32(X, metric, ms):
    """(fp64 mutual reachability W64, the pairs' units U, the power, e32, e32 in the one unit max U): the checked quantity is
    knn_checks.FLOOR's -- the cosine distance itself (unit 1), the euclidean distance squared relative to the two rows'
    squared norms.  A weight is the largest of three distances -- d(i, j), core_i = d(i, its ms-th nearest row) and core_j --
    and the error of a maximum is at most the largest of its terms' errors, so a pair's unit is the largest of the three
    terms' units: |x_i|^2 + |x_j|^2, |x_i|^2 + |x_n(i)|^2 and |x_j|^2 + |x_n(j)|^2, n(.) the ms-th nearest row in fp64.
    e32 is the largest error, in the pairs' units, of the mutual reachability of plain fp32 torch (norms + matmul, its own
    core distances) against fp64 over all pairs."""
    X64 = X.astype(np.float64)
    n = X.shape[0]
    D64 = dbscan_ref.distances64(X64, metric)                       # fp64: the direct form in column blocks / normalised rows
    W64, _ = R.mutual_reachability(D64, ms)
    T = torch.from_numpy(X)
    G, sq = T @ T.t(), (T * T).sum(1)
    if metric == EUCLIDEAN:
        D32 = torch.sqrt(torch.clamp(sq[:, None] + sq[None, :] - 2.0 * G, min=0.0))
    else:
        D32 = torch.clamp(1.0 - G / (torch.sqrt(sq)[:, None] * torch.sqrt(sq)[None, :]), min=0.0)
    D32 = D32.numpy()
    np.fill_diagonal(D32, 0.0)
    W32, _ = R.mutual_reachability(D32, ms)
    if metric == EUCLIDEAN:
        sq64 = (X64 * X64).sum(1)
        kth = np.argsort(D64, axis=1, kind="stable")[:, ms - 1]
        core_unit = sq64 + sq64[kth]
        U = np.maximum(sq64[:, None] + sq64[None, :], np.maximum(core_unit[:, None], core_unit[None, :]))
    else:
        U = np.ones((n, n))
    power = 2 if metric == EUCLIDEAN else 1
    off = ~np.eye(n, dtype=bool)
    err = np.abs(W32.astype(np.float64) ** power - W64 ** power)
    return W64, U, power, float((err / U)[off].max()), float(err[off].max() / U.max())


@pytest.mark.parametrize("metric", [EUCLIDEAN, COSINE])
@pytest.mark.parametrize("mcs,ms", R.PARAMS)
@pytest.mark.parametrize("offset", R.OFFSETS)
@pytest.mark.parametrize("N,D", R.SHAPES)
def test_real_valued_fixtures(N, D, offset, mcs, ms, metric):
    """The edges form a spanning tree; every weight equals fp64's max(core_i, core_j, d_ij) within max(FLOOR, 4 e32) in its
    pair's unit (_fp64_and_e32); so does the sorted weight vector -- the same for every minimum spanning tree of a graph -- against scipy's fp64 tree.
    Euclidean: the noise set of sklearn and adjusted Rand index 1.0.  Cosine: the labels of the naive restatement on the
    device's own edges (fp32 and fp64 cosine trees differ in near-ties, so sklearn is not the yardstick there)."""
    from scipy.sparse.csgraph import minimum_spanning_tree
    X = R.blobs(N, D, offset)
    k = ms or mcs
    hd = _fit(X, mcs, ms, NAMES[metric])
    lo, hi, w = _edges(hd)
    assert R.is_spanning_tree(lo, hi, N)
    W64, U, power, e32, e32_sup = _fp64_and_e32(X, metric, k)
    bound, bound_sup = max(FLOOR, 4 * e32), max(FLOOR, 4 * e32_sup)
    e_edges = float((np.abs(w.astype(np.float64) ** power - W64[lo, hi] ** power) / U[lo, hi]).max())
    # the sorted weights of a minimum spanning tree move by at most the largest change of any pair's weight: one unit, max U
    ref = np.sort(minimum_spanning_tree(np.triu(W64 + 1.0, 1)).data - 1.0)        # + 1: scipy reads a zero as no edge
    e_sorted = float(np.abs(np.sort(w.astype(np.float64)) ** power - ref ** power).max()) / float(U.max())
    print(f"({N}, {D}) offset {offset} {NAMES[metric]} ({mcs}, {ms}): edge error {e_edges:.3e} (plain fp32 {e32:.3e}, bound {bound:.3e}), "
          f"sorted weights {e_sorted:.3e} (plain fp32 {e32_sup:.3e}, bound {bound_sup:.3e}); {hd.n_clusters_} clusters, "
          f"{hd.n_noise_} noise, {hd.n_rounds_} rounds")
    assert e_edges <= bound and e_sorted <= bound_sup
    labels = hd.labels_.cpu().numpy()
    naive = R.naive_hdbscan(lo, hi, w, N, mcs)
    assert np.array_equal(labels, naive[0]) and np.abs(hd.probabilities_.cpu().numpy() - naive[1]).max() <= 2.0 ** -24
    if metric == EUCLIDEAN:
        from sklearn.cluster import HDBSCAN
        sk = HDBSCAN(min_cluster_size=mcs, min_samples=ms, algorithm="brute").fit(X.astype(np.float64))
        assert np.array_equal(labels < 0, sk.labels_ < 0) and R.rand_index_is_one(sk.labels_, labels)


# ------------------------------------------------------------------ (7) hand-built cases
def test_shuffled_chain_takes_log_rounds():
    """Equally spaced points on a line, shuffled: every weight is 1, all ties, and the components can at best double per
    round -- the worst case for the number of rounds, which stays within ceil(log2 N)."""
    N = 1500
    chain = np.zeros((N, 3))
    chain[:, 0] = np.arange(N)
    chain = chain[np.random.default_rng(3).permutation(N)]
    hd = _check_exact(chain, 2, allow_single_cluster=True)
    assert set(_edges(hd)[2].tolist()) == {1.0} and 2 <= hd.n_rounds_ <= math.ceil(math.log2(N))
    assert hd.labels_.tolist() == [0] * N and hd.n_clusters_ == 1
    print(f"shuffled chain of {N}: {hd.n_rounds_} rounds")


def test_duplicates():
    """Zero distances: edges of weight 0, infinite lambda, probability 1."""
    X = np.repeat(np.random.default_rng(3).integers(0, 6, (40, 8)), 3, axis=0)
    hd = _check_exact(X, 2, mcs=3)
    w = _edges(hd)[2]
    assert (w == 0).sum() >= 80 and np.isinf(hd.condensed_tree_["value"]).any()
    assert hd.n_clusters_ >= 2 and bool((hd.probabilities_[hd.labels_ >= 0] == 1).any())
    same = np.ones((50, 4))
    hd = _check_exact(same, 5, allow_single_cluster=True)            # every row the same: one cluster at lambda = inf
    assert hd.labels_.tolist() == [0] * 50 and hd.probabilities_.tolist() == [1.0] * 50


def test_two_densities_and_a_bridge():
    """A dense blob (a 10 x 10 lattice of spacing 1), a sparse one (8 x 8, spacing 3) and a bridge of points 5 apart between
    them: no single eps separates the two without dissolving the sparse one (DBSCAN at eps 1 finds one cluster and 70
    noise rows); HDBSCAN keeps each blob whole, in a cluster of its own."""
    g = np.stack(np.meshgrid(np.arange(10), np.arange(10)), -1).reshape(-1, 2)
    s = np.stack(np.meshgrid(np.arange(8), np.arange(8)), -1).reshape(-1, 2) * 3 + np.array([40, 0])
    bridge = np.stack([np.arange(14, 40, 5), np.full(6, 4)], 1)
    P = np.concatenate([g, s, bridge])
    perm = np.random.default_rng(1).permutation(len(P))
    hd = _check_exact(P[perm], 4, mcs=8)
    labels = hd.labels_.cpu().numpy()[np.argsort(perm)]
    assert hd.n_clusters_ == 2 and len(set(labels[:100])) == 1 and len(set(labels[100:164])) == 1 and labels[0] != labels[100] and labels[0] >= 0


def test_fewer_rows_than_a_cluster_and_single_cluster():
    X = np.random.default_rng(5).integers(0, 9, (4, 3))
    hd = _check_exact(X, 2, mcs=5)
    assert hd.labels_.tolist() == [-1] * 4 and hd.probabilities_.tolist() == [0.0] * 4 and hd.n_clusters_ == 0 and hd.n_noise_ == 4
    blob = R.blobs(130, 3, centers=1)
    off, on = _fit(blob, 12, 4), _fit(blob, 12, 4, allow_single_cluster=True)
    assert np.array_equal(_edges(off)[0], _edges(on)[0]) and on.n_clusters_ == 1
    for hd, single in ((off, False), (on, True)):
        naive = R.naive_hdbscan(*_edges(hd), 130, 12, allow_single_cluster=single)
        assert np.array_equal(hd.labels_.cpu().numpy(), naive[0])
    with pytest.raises(ValueError, match=r"min_samples \(30\) must be at most the number of samples in X \(8\)"):
        _fit(np.zeros((8, 2)), 5, 30)
    with pytest.raises(ValueError, match="n_samples=1 while HDBSCAN requires more than one sample"):
        _fit(np.zeros((1, 2)))
    with pytest.raises(ValueError, match="not supported"):
        _fit(np.zeros((8, 2)), 8)                                    # min_samples = N: the neighbour list is shorter than the set


# ------------------------------------------------------------------ (8) invariances and memory
@pytest.mark.parametrize("metric", [COSINE, EUCLIDEAN])
@pytest.mark.parametrize("N,D", SHAPES)
def test_two_fits_row_order_and_scaling(N, D, metric):
    """Two fits are bitwise equal.  A row permutation leaves the sorted weights bit for bit (a pair's weight does not depend on
    its place) and, where the tree's weights are untied, permutes edges and labels consistently: with min_samples = 1 mutual
    reachability is the distance itself, which real-valued rows do not tie (with min_samples > 1 it always ties, and which of
    two tied edges merges first follows the row order by design; measured on an MI355X: untied at (257, 12288) cosine and at
    (333, 1003) and (130, 3) euclidean, tied by fp32 rounding in the other three cases, where only the weights are compared).
    Scaling X by a power of two changes no edge: euclidean weights scale exactly, cosine weights do not move."""
    X = R.blobs(N, D)
    a, b = _fit(X, 5, None, NAMES[metric]), _fit(X, 5, None, NAMES[metric])
    assert np.array_equal(a.minimum_spanning_tree_.view(np.int64), b.minimum_spanning_tree_.view(np.int64))
    assert torch.equal(a.labels_, b.labels_) and torch.equal(a.probabilities_, b.probabilities_)
    assert torch.equal(a.core_distances_, b.core_distances_) and a.n_rounds_ == b.n_rounds_
    perm = np.random.default_rng(N).permutation(N)
    c = _fit(X[perm], 5, None, NAMES[metric])
    assert np.array_equal(np.sort(_edges(c)[2]).view(np.uint32), np.sort(_edges(a)[2]).view(np.uint32))
    a1, c1 = _fit(X, 5, 1, NAMES[metric]), _fit(X[perm], 5, 1, NAMES[metric])
    assert np.array_equal(_edges(c1)[2].view(np.uint32), _edges(a1)[2].view(np.uint32))
    untied = len(np.unique(_edges(a1)[2])) == N - 1
    print(f"({N}, {D}) {NAMES[metric]}: the min_samples = 1 tree is {'untied' if untied else 'tied'}")
    assert untied or (N, D, metric) not in UNTIED, "the weights of a tree that was untied now tie: the partition check would be lost"
    if untied:
        pairs = lambda lo, hi: {(min(x, y), max(x, y)) for x, y in zip(lo.tolist(), hi.tolist())}      # noqa: E731
        assert pairs(perm[_edges(c1)[0]], perm[_edges(c1)[1]]) == pairs(_edges(a1)[0], _edges(a1)[1])
        assert R.same_partition(c1.labels_.cpu().numpy(), a1.labels_.cpu().numpy()[perm])
        assert torch.equal(c1.probabilities_.cpu(), a1.probabilities_.cpu()[torch.from_numpy(perm)])
    for e in (20, -20):
        s = _fit(X * np.float32(2.0 ** e), 5, None, NAMES[metric])
        assert np.array_equal(_edges(s)[0], _edges(a)[0]) and np.array_equal(_edges(s)[1], _edges(a)[1])
        scale = np.float32(2.0 ** e) if metric == EUCLIDEAN else np.float32(1)
        assert np.array_equal(_edges(s)[2], _edges(a)[2] * scale) and torch.equal(s.labels_, a.labels_)


def _rounds_in_guarded_buffers(x, metric, core, what, matrix=False):
    """The device side of a fit with every buffer between guard bands at its exact size, poisoned -> the sorted edges."""
    from vit_som_amd import ops
    from vit_som_amd.hdbscan import round_limit, sort_edges
    N = x.shape[0]
    bufs = {"comp": memcheck.guarded((N,), torch.int32, DEV), "edges": memcheck.guarded((N, 3), torch.int32, DEV),
            "record": memcheck.guarded((4,), torch.int32, DEV), "best": memcheck.guarded((N,), torch.int64, DEV),
            "work": memcheck.guarded((ops.hdbscan_work(N),), torch.int64, DEV)}
    if not matrix:
        bufs["sq"] = memcheck.guarded((N,), torch.float32, DEV)
    v = {k: b[0] for k, b in bufs.items()}
    ops.hdbscan_init(v["comp"], v["edges"], v["record"])
    for _ in range(round_limit(N)):
        if matrix:
            ops.hdbscan_nearest_matrix(x, core, v["comp"], v["best"], v["record"])
        else:
            ops.hdbscan_nearest(x, metric, core, v["comp"], v["sq"], v["best"], v["record"])
        ops.hdbscan_merge(v["best"], v["comp"], v["edges"], v["work"], v["record"])
        if v["record"].tolist()[0] == 1:
            break
    torch.cuda.synchronize()
    for k, (_, h) in bufs.items():
        h.all_written(f"{what}: {k}")
        h.check(f"{what}: {k}")
    rec = v["record"].tolist()
    assert rec[:3] == [1, N - 1, 0] and 1 <= rec[3] <= math.ceil(math.log2(N)), what
    assert v["comp"].unique().numel() == 1, what
    e = v["edges"].cpu().numpy()
    assert (e[:, 0] < 0).sum() == 1 and int(np.flatnonzero(e[:, 0] < 0)[0]) == int(v["comp"][0]), what      # only the last root's slot is empty
    e = e[e[:, 0] >= 0]
    lo, hi, w = sort_edges(e[:, 0], e[:, 1], np.ascontiguousarray(e[:, 2]).view(np.float32))
    return lo, hi, w.astype(np.float32)


def test_every_output_is_written_exactly_and_misaligned_rows_change_no_edge():
    """Every output sits between guard bands at its exact size, poisoned: all of it is written, nothing beside it.  X with a
    row stride, with its base moved by 4 bytes, with a stride that is no multiple of 4 and with D % 4 != 0 (the last column
    of the fixture is zero, so dropping it changes no sum): the edges are those of the aligned dense copy."""
    N, D = 200, 52
    X = np.random.default_rng(4).integers(-9, 10, (N, D)).astype(np.float32)
    X[:, -1] = 0
    D32, core, want = _exact_tree(X, 4)
    dense = _dev(X)
    assert dense.data_ptr() % 16 == 0
    variants = {
        "dense": dense,
        "row stride": memcheck.guarded_copy(dense, ld=D + 4)[0],
        "base + 4 bytes": memcheck.guarded_copy(dense, shift=1)[0],
        "stride 53": memcheck.guarded_copy(dense, ld=D + 1)[0],
        "D % 4 != 0": memcheck.guarded_copy(dense, ld=D + 4)[0][:, :D - 1],
    }
    assert variants["base + 4 bytes"].data_ptr() % 16 == 4 and variants["stride 53"].stride(0) == 53
    for what, x in variants.items():
        _same_edges(_rounds_in_guarded_buffers(x, EUCLIDEAN, _dev(core), what), want)
    m32 = memcheck.guarded_copy(_dev(D32), ld=N + 3)[0]              # a precomputed matrix between guard bands, with a row stride
    _same_edges(_rounds_in_guarded_buffers(m32, None, _dev(core), "matrix", matrix=True), want)


# ------------------------------------------------------------------ (9) bad rows, precomputed input, evaluation
def test_bad_rows():
    from vit_som_amd import HDBSCAN, ops
    X = R.blobs(333, 1003)
    for metric in (COSINE, EUCLIDEAN):
        for value in (float("nan"), float("inf"), 1e30):             # 1e30: the squared norm overflows
            bad = X.copy()
            bad[5, 17], bad[200, 1000] = value, value
            hd = HDBSCAN(metric=NAMES[metric])
            with pytest.raises(ValueError, match="2 rows of X are not finite"):
                hd.fit(_dev(bad))
            assert not any(hasattr(hd, a) for a in ("labels_", "probabilities_", "n_features_in_", "minimum_spanning_tree_"))
    # straight to the entry: the bad rows are counted, offer nothing and receive nothing
    bad = X.copy()
    bad[5, 17], bad[200, 1000] = float("nan"), 1e30
    N = 333
    new = lambda dtype, *shape: torch.empty(*shape, dtype=dtype, device=DEV)      # noqa: E731
    comp, edges, record, best, sq = new(torch.int32, N), new(torch.int32, N, 3), new(torch.int32, 4), new(torch.int64, N), new(torch.float32, N)
    ops.hdbscan_init(comp, edges, record)
    assert record.tolist() == [N, 0, 0, 0] and comp.tolist() == list(range(N)) and bool((edges == -1).all())
    ops.hdbscan_nearest(_dev(bad), EUCLIDEAN, torch.ones(N, device=DEV), comp, sq, best, record)
    b = best.cpu().numpy()
    assert record.tolist()[2] == 2 and b[5] == b[200] == -1 and (np.delete(b, [5, 200]) >= 0).all()
    assert not np.isin(b & 0xffffffff, [5, 200]).any()


@pytest.mark.parametrize("N,D", SHAPES)
def test_precomputed_input_equals_the_tile_path(N, D):
    """On integer data the float32 and the float64 matrix give the edges of the contraction, bit for bit; so does the fp64
    direct form of ops.agglo_distances."""
    from test_silhouette_gpu import _integers
    from vit_som_amd import ops
    X = _integers(N, D, 5)
    D32, _, want = _exact_tree(X, 5)
    tile = _fit(X, 5)
    _same_edges(_edges(tile), want)
    for M in (_dev(D32), _dev(D32.astype(np.float64), np.float64)):
        hd = _fit(M, 5, None, "precomputed")
        _same_edges(_edges(hd), want)
        assert torch.equal(hd.labels_, tile.labels_) and torch.equal(hd.core_distances_, tile.core_distances_) and hd.n_features_in_ == N
    out, st = torch.empty(N, N, dtype=torch.float64, device=DEV), torch.empty(2, dtype=torch.int32, device=DEV)
    ops.agglo_distances(_dev(X), ops.AGGLO_EUCLIDEAN, False, out, st)
    _same_edges(_edges(_fit(out, 5, None, "precomputed")), want)     # fp64 roots of exact integers round to the fp32 roots


def test_precomputed_class_equals_sklearn():
    from sklearn.cluster import HDBSCAN
    X = R.blobs(333, 1003)
    D64 = R.distances64(X, EUCLIDEAN)
    sk = HDBSCAN(min_cluster_size=12, min_samples=4, metric="precomputed").fit(D64.copy())
    for M in (_dev(D64, np.float64), _dev(D64)):
        hd = _fit(M, 12, 4, "precomputed")
        labels = hd.labels_.cpu().numpy()
        assert np.array_equal(labels < 0, sk.labels_ < 0) and R.rand_index_is_one(sk.labels_, labels)
        assert np.abs(hd.probabilities_.cpu().numpy() - sk.probabilities_).max() <= 1e-5
    with pytest.raises(ValueError, match="Precomputed matrix must be square"):
        _fit(_dev(D64[:, :300]), 5, None, "precomputed")
    with pytest.raises(ValueError, match="Negative values"):
        _fit(_dev(-D64), 5, None, "precomputed")
    D64[4, 9] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        _fit(_dev(D64), 5, None, "precomputed")


def _report_arrays(rep):
    return dict(labels=rep.labels.cpu().numpy(), probabilities=rep.probabilities.cpu().numpy(), sizes=rep.cluster_sizes,
                persistence=rep.cluster_persistence, noise_per_class=rep.noise_per_class,
                scalars=np.array([rep.min_cluster_size, rep.min_samples, rep.n_clusters, rep.n_noise, rep.coverage, rep.mean_probability,
                                  rep.purity, rep.nmi, rep.n_rounds, rep.n_samples], dtype=np.float64))


@pytest.mark.parametrize("name", ["ref_cluster_tiny", "ref_hexa_euclid_tiny"])
def test_evaluate_hdbscan_on_the_tiny_fixtures(name, tmp_path):
    from test_knn_gpu import _loaders, _model
    from test_silhouette_gpu import _spread_map
    from vit_som_amd import HDBSCAN, HDBSCANReport, evaluate_hdbscan
    from vit_som_amd.evaluation import _som_latents, _Table, _umap_embed, nmi_from_table, purity_from_table
    m, cfg = _model(name)
    train, _ = _loaders(cfg, 4)                                    # 96 samples in batches of 10
    _spread_map(m, cfg, train)
    metric = m.som_layer.distance_fcn
    assert metric in ("cosine", "euclidean")
    X, _ = _som_latents(m, cfg, train, "test")
    y = torch.cat([b[1] for b in train]).to(DEV).long()
    rep = evaluate_hdbscan(m, cfg, train)
    assert isinstance(rep, HDBSCANReport) and (rep.metric, rep.space, rep.n_samples) == (metric, "latent", 96)
    assert rep.min_cluster_size == 5 and rep.min_samples == 5     # the stated rule: max(5, 96 // (20 classes))
    hd = HDBSCAN(min_cluster_size=5, min_samples=5, metric=metric).fit(X)
    assert torch.equal(rep.labels, hd.labels_) and torch.equal(rep.probabilities, hd.probabilities_)
    assert (rep.n_clusters, rep.n_noise, rep.n_rounds) == (hd.n_clusters_, hd.n_noise_, hd.n_rounds_)
    assert rep.coverage == (96 - rep.n_noise) / 96 and np.array_equal(rep.cluster_persistence, hd.cluster_persistence_)
    labels = hd.labels_.cpu().numpy()
    assert np.array_equal(rep.cluster_sizes, np.bincount(labels[labels >= 0], minlength=rep.n_clusters))
    if rep.n_clusters:
        t = _Table(rep.n_clusters, 256, DEV)
        t.add(hd.labels_[hd.labels_ >= 0], y[hd.labels_ >= 0])
        assert rep.purity == purity_from_table(t.numpy()) and rep.nmi == nmi_from_table(t.numpy())
        assert rep.mean_probability == float(hd.probabilities_[hd.labels_ >= 0].double().mean())
    else:
        assert np.isnan(rep.purity) and np.isnan(rep.nmi) and np.isnan(rep.mean_probability)
    assert np.array_equal(rep.noise_per_class, np.bincount(y.cpu().numpy()[labels < 0], minlength=len(rep.noise_per_class)))
    assert rep.noise_per_class.sum() == rep.n_noise
    print(f"{name}: {rep.n_clusters} clusters, {rep.n_noise} noise, purity {rep.purity:.3f}, nmi {rep.nmi:.3f}, {rep.n_rounds} rounds")
    given = evaluate_hdbscan(m, cfg, train, min_cluster_size=8, min_samples=3, metric="euclidean")
    want = HDBSCAN(min_cluster_size=8, min_samples=3, metric="euclidean").fit(X)
    assert torch.equal(given.labels, want.labels_) and given.metric == "euclidean" and (given.min_cluster_size, given.min_samples) == (8, 3)
    planar = evaluate_hdbscan(m, cfg, train, space="umap")         # the 2-D embedding, euclidean whatever the SOM's metric
    want = HDBSCAN(min_cluster_size=5, min_samples=5).fit(_umap_embed(X)[1].contiguous())
    assert torch.equal(planar.labels, want.labels_) and (planar.space, planar.metric) == ("umap", "euclidean")
    nothing = evaluate_hdbscan(m, cfg, train, min_cluster_size=97, min_samples=5)
    assert nothing.n_clusters == 0 and nothing.n_noise == 96 and np.isnan(nothing.purity) and nothing.coverage == 0.0
    with pytest.raises(ValueError, match="metric must be"):
        evaluate_hdbscan(m, cfg, train, metric="manhattan")
    with pytest.raises(ValueError, match="space must be"):
        evaluate_hdbscan(m, cfg, train, space="pca")
    from vit_som_amd import visualize_hdbscan
    emb, drawn = visualize_hdbscan(m, cfg, train, output_dir=str(tmp_path))
    assert emb.shape == (96, 2) and emb.dtype == np.float32 and np.array_equal(drawn, labels)


def _dp_worker(rank, world, port, out):
    import torch.distributed as dist
    from test_knn_gpu import _loaders, _model
    from test_silhouette_gpu import _spread_map
    from vit_som_amd import evaluate_hdbscan
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    m, cfg = _model("ref_cluster_tiny")
    train, _ = _loaders(cfg, 4)
    _spread_map(m, cfg, train)                                   # as one process: before the model learns of the ranks
    m.world_size, m.rank = world, rank
    rep = evaluate_hdbscan(m, cfg, [b for i, b in enumerate(train) if i % world == rank])
    np.savez(f"{out}.{rank}.npz", **_report_arrays(rep))
    dist.barrier()
    dist.destroy_process_group()


def test_evaluate_hdbscan_two_ranks(tmp_path):
    """Both ranks gather all rows (50 + 46, rank 0's first) and return bit-identical reports: that of one process over the
    rows in that order."""
    import torch.multiprocessing as mp
    from test_distributed import _free_port
    from test_knn_gpu import _loaders, _model
    from test_silhouette_gpu import _spread_map
    from vit_som_amd import evaluate_hdbscan
    out = str(tmp_path / "hdbscan")
    mp.spawn(_dp_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    r0, r1 = np.load(f"{out}.0.npz"), np.load(f"{out}.1.npz")
    m, cfg = _model("ref_cluster_tiny")
    train, _ = _loaders(cfg, 4)
    _spread_map(m, cfg, train)
    single = _report_arrays(evaluate_hdbscan(m, cfg, train[0::2] + train[1::2]))
    assert set(r0.files) == set(r1.files) == set(single)
    for key, want in single.items():
        assert r0[key].tobytes() == r1[key].tobytes() == want.tobytes(), key


def test_driver_reports_hdbscan(tmp_path):
    from vit_som_amd.train import main, synthetic_loaders
    _, cfg = load_golden("ref_cluster_tiny")
    cfg = copy.deepcopy(cfg)
    cfg["hyperparameters"]["batch_size"] = 16
    logs = []
    loaders = lambda c, r, w: synthetic_loaders(c, r, w, n_train=64, n_val=16, n_test=16)      # noqa: E731
    today = {"accuracy", "precision", "recall", "f1", "purity", "nmi", "run_duration", "inference_time"}
    met = main(cfg, n_runs=1, max_epochs=1, make_loaders=loaders, model_states_dir=str(tmp_path / "a"), log=logs.append,
               hdbscan_eval=True)
    assert set(met) == today | {"hdbscan_clusters", "hdbscan_noise", "hdbscan_purity", "hdbscan_nmi"}
    assert all(len(met[k]) == 1 for k in ("hdbscan_clusters", "hdbscan_noise", "hdbscan_purity", "hdbscan_nmi"))
    assert 0 <= met["hdbscan_noise"][0] <= 64 and met["hdbscan_clusters"][0] >= 0
    print([l for l in logs if "HDBSCAN" in l])
    assert any(l.startswith("HDBSCAN:") for l in logs)
