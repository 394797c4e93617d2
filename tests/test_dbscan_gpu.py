"""On-device DBSCAN (csrc/knn.hip's DBSCAN section, vit_som_amd/dbscan.py) at the smallest shapes at which the kernels can
still go wrong: the bit matrix word for word against the restatement on integer data, labels equal to sklearn's on lattice
fixtures whose distances keep clear of eps, hand-built cases, invariances, guarded buffers and misaligned operands, bad
rows, precomputed input and the evaluation path."""
import copy
import signal

import numpy as np
import pytest
import torch

import dbscan_ref as R
import memcheck
import silhouette_ref as SR
from helpers import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COSINE, EUCLIDEAN = R.COSINE, R.EUCLIDEAN
NAMES = {COSINE: "cosine", EUCLIDEAN: "euclidean"}
SHAPES = [(257, 12288), (333, 1003), (130, 3)]        # two row blocks + 1 and 16-byte loads; element-wise loads; tiny D
LATTICE_SHAPES = SHAPES + [(700, 64)]
CASES = [(EUCLIDEAN, 0.0), (EUCLIDEAN, 0.05), (COSINE, 0.05), (COSINE, 0.10)]


@pytest.fixture(autouse=True)
def time_limit(request):
    """A limit of its own (seconds) for every test here, as in test_silhouette_gpu.py: a SIGALRM handler ends a test whose
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


def _graph(X, metric, eps):
    """One ops.dbscan_neighbours call -> (words uint64 [N, W], count int32 [N], sq f32 [N], status [2]) as host arrays."""
    from vit_som_amd import ops
    X = X if isinstance(X, torch.Tensor) else _dev(X)
    N = X.shape[0]
    new = lambda dtype, *shape: torch.empty(*shape, dtype=dtype, device=DEV)      # noqa: E731
    sq, adj, count, status = new(torch.float32, N), new(torch.int64, N, ops.dbscan_words(N)), new(torch.int32, N), new(torch.int64, 2)
    ops.dbscan_neighbours(X, metric, eps, sq, adj, count, status)
    return adj.cpu().numpy().view(np.uint64), count.cpu().numpy(), sq.cpu().numpy(), status.tolist()


def _threshold(M, eps):
    from vit_som_amd import ops
    N = M.shape[0]
    new = lambda dtype, *shape: torch.empty(*shape, dtype=dtype, device=DEV)      # noqa: E731
    adj, count, status = new(torch.int64, N, ops.dbscan_words(N)), new(torch.int32, N), new(torch.int64, 2)
    ops.dbscan_threshold(M, eps, adj, count, status)
    return adj.cpu().numpy().view(np.uint64), count.cpu().numpy(), status.tolist()


def _check_graph(got, D32, eps, bad=()):
    """The device's words are the restatement's, word for word; count the popcounts; status the bad rows and the set bits;
    symmetry, the set diagonal and zero tail bits."""
    words, count, _, status = got
    N = D32.shape[0]
    want = R.bit_matrix(D32, eps)
    assert words.shape == want.shape and np.array_equal(words, want)
    assert np.array_equal(count, R.popcounts(want, N))
    assert status == [len(bad), int(count.sum())]
    R.check_structure(words, N, bad)


def _attained(D32, q):
    """A distance some pair attains, near the q quantile of the off-diagonal ones, and the double just below it."""
    off = np.sort(D32[~np.eye(D32.shape[0], dtype=bool)])
    d = float(off[int(q * (off.size - 1))])
    assert d > 0
    return d, float(np.nextafter(d, 0.0))


def _sklearn(D64, eps, min_samples):
    from sklearn.cluster import DBSCAN
    sk = DBSCAN(eps=eps, min_samples=min_samples, metric="precomputed").fit(D64)
    return sk.labels_, sk.core_sample_indices_


def _fit(X, eps, min_samples, metric="euclidean", keep_graph=True):
    from vit_som_amd import DBSCAN
    X = X if isinstance(X, torch.Tensor) else _dev(X)
    return DBSCAN(eps=eps, min_samples=min_samples, metric=metric).fit(X, keep_graph=keep_graph)


def _host(db):
    return db.labels_.cpu().numpy(), db.core_sample_indices_.cpu().numpy()


# ------------------------------------------------------------------ (a) exact on integer data
@pytest.mark.parametrize("N,D", SHAPES)
def test_exact_on_integer_data(N, D):
    """Every squared distance is an integer exact in fp32 and sqrtf is correctly rounded: the device's distances ARE
    exact_euclidean32's.  At an attained distance <= is inclusive and those pairs are in; at the double just below they are out."""
    from test_silhouette_gpu import _integers
    X = _integers(N, D, 5)
    D32, _ = SR.exact_euclidean32(X)
    for q in (0.1, 0.5):
        eps, below = _attained(D32, q)
        got = _graph(X, EUCLIDEAN, eps)
        _check_graph(got, D32, eps)
        under = _graph(X, EUCLIDEAN, below)
        _check_graph(under, D32, below)
        moved = R.unpack(got[0], N)[:, :N] & ~R.unpack(under[0], N)[:, :N]
        assert moved.any() and np.array_equal(moved, D32 == np.float32(eps))
    sq = (X.astype(np.int64) ** 2).sum(1)
    assert np.array_equal(got[2], sq.astype(np.float32))


@pytest.mark.parametrize("N", [2, 64, 65, 128, 129, 191, 3000, 4300])
def test_word_tile_and_chunk_edges(N):
    """Word and tile edges (N = 2 .. 191) and the two chunk regimes test_silhouette_gpu.py names: N = 3000 runs one tile per
    chunk, N = 4300 is the first size range at which a chunk holds more than one.  D = 8 takes the 16-byte loads."""
    X = np.random.default_rng(N).integers(0, 32, (N, 8))
    D32, _ = SR.exact_euclidean32(X)
    eps, below = _attained(D32, 0.05 if N > 2 else 0.0)
    _check_graph(_graph(X, EUCLIDEAN, eps), D32, eps)
    _check_graph(_graph(X, EUCLIDEAN, below), D32, below)


# ------------------------------------------------------------------ (b) labels equal sklearn's
@pytest.mark.parametrize("metric,offset", CASES)
@pytest.mark.parametrize("N,D", LATTICE_SHAPES)
def test_labels_equal_sklearns_on_lattice_fixtures(N, D, metric, offset):
    """labels_, core_sample_indices_ and components_ equal sklearn's on its fp64 distances, label for label.  The condition is
    asserted on the host before the device is called: no pair's fp64 distance lies within 4 x e32 of eps, e32 the largest
    error of plain-fp32 torch against fp64 over the pairs with distance in [eps / 2, 2 eps] (the project's e32 rule)."""
    X, _ = R.lattice(N, D, offset, metric)
    if metric == EUCLIDEAN:
        eps = 0.5295                                                 # between two lattice distances, 2/4 and sqrt(5)/4
        e32, D64 = R.e32_error(X, metric, eps)
    else:
        eps = R.cosine_eps(R.distances64(X, metric))
        e32, D64 = R.e32_error(X, metric, eps)
    gap = R.margin(D64, eps)
    print(f"({N}, {D}) {NAMES[metric]} offset {offset}: eps {eps:.6g}, margin {gap:.3e}, e32 {e32:.3e}, margin / e32 {gap / max(e32, 1e-300):.1f}")
    assert gap >= 4 * e32, "the fixture breaks the condition"
    want, want_core = _sklearn(D64, eps, 5)
    assert want.max() >= 1 and (want < 0).any()
    db = _fit(X, eps, 5, NAMES[metric])
    labels, core = _host(db)
    assert np.array_equal(labels, want) and np.array_equal(core, want_core)
    assert torch.equal(db.components_, _dev(X)[db.core_sample_indices_]) and db.n_features_in_ == D
    # The bit matrix itself equals fp64's where the format guarantees it.  The contraction sums a pair's D products in one
    # fp32 chain: each of <x, x>, <y, y>, <x, y> is off by at most g max|x|^2 with g = D 2^-24 (the worst case of a chain), so
    # d^2 = s_i + s_j - 2 dot by at most 4 g max|x|^2 and the cosine by at most 3 g (plus a few ulp of the quotient).  Where
    # that bound is below the fixture's gap the words must agree; elsewhere (the wide fixtures) only the labels are asserted.
    g = D * 2.0 ** -24
    if metric == EUCLIDEAN:
        off = ~np.eye(N, dtype=bool)
        guaranteed = 4 * g * float((X.astype(np.float64) ** 2).sum(1).max()) < float(np.abs(D64[off] ** 2 - eps ** 2).min())
    else:
        guaranteed = 3 * g + 8 * 2.0 ** -24 < gap
    same_words = np.array_equal(db.neighbourhoods_.cpu().numpy().view(np.uint64), R.bit_matrix(D64, eps))
    print(f"    fp32 chain bound below the gap: {guaranteed}; device words equal fp64's: {same_words}")
    assert same_words or not guaranteed
    assert guaranteed or D > 64                                      # the narrow fixtures are always within the bound
    border =int((want >= 0).sum()) - want_core.size
    assert (db.n_clusters_, db.n_core_, db.n_border_, db.n_noise_) == (want.max() + 1, want_core.size, border, int((want < 0).sum()))
    print(f"    clusters / core / border / noise {db.n_clusters_, db.n_core_, db.n_border_, db.n_noise_}, round calls {db.n_round_calls_}")


# ------------------------------------------------------------------ (c) hand-built cases
@pytest.mark.parametrize("name", ["border_between_two", "chain_interleaved", "chain_reversed", "chain_shuffled", "duplicates"])
def test_hand_built_cases(name):
    from test_dbscan_cpu import _hand_built
    from vit_som_amd.dbscan import ROUNDS_PER_CALL
    X, eps, min_samples = _hand_built()[name]
    want, want_core = _sklearn(R.distances64(X, EUCLIDEAN), eps, min_samples)
    db = _fit(X, eps, min_samples)
    labels, core = _host(db)
    print(f"{name}: {db.n_clusters_} clusters, {db.n_round_calls_} dbscan_round calls of {ROUNDS_PER_CALL} rounds")
    assert np.array_equal(labels, want) and np.array_equal(core, want_core)
    if name == "border_between_two":
        assert labels.tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1, -1]    # within eps of cores of both: the smaller label
    if name.startswith("chain"):
        assert (labels == 0).all() and db.n_clusters_ == 1
    if name == "duplicates":
        assert db.n_noise_ == 0 and np.array_equal(labels[0::3], labels[1::3]) and np.array_equal(labels[0::3], labels[2::3])


def test_parameter_edges():
    rng = np.random.default_rng(9)
    X = rng.integers(0, 9, (150, 8)).astype(np.float64)
    X[10], X[77] = X[3], X[3]                                         # three identical rows
    D64 = R.distances64(X, EUCLIDEAN)
    db = _fit(X, 3.0, 151)                                           # min_samples > N: all noise
    assert (db.n_clusters_, db.n_core_, db.n_noise_) == (0, 0, 150) and (_host(db)[0] == -1).all() and db.core_sample_indices_.numel() == 0
    assert db.components_.shape == (0, 8)
    smallest = D64[D64 > 0].min()
    db = _fit(X, float(smallest) / 2, 1)                             # below the smallest non-zero distance: exact duplicates only
    A = R.unpack(db.neighbourhoods_.cpu().numpy(), 150)[:, :150]
    assert np.array_equal(A, D64 == 0) and A.sum() > 150
    labels, core = _host(db)
    want, want_core = _sklearn(D64, float(smallest) / 2, 1)
    assert np.array_equal(labels, want) and np.array_equal(core, want_core) and labels[3] == labels[10] == labels[77]
    db = _fit(X, 1e6, 5)                                             # a huge eps: one cluster
    assert (db.n_clusters_, db.n_core_, db.n_noise_) == (1, 150, 0) and (_host(db)[0] == 0).all()
    same = np.tile(rng.integers(1, 9, (1, 8)).astype(np.float64), (90, 1))
    for metric in ("euclidean", "cosine"):                           # all rows identical: every distance exactly 0
        db = _fit(same, 1e-12, 90, metric)
        assert (db.n_clusters_, db.n_core_, db.n_noise_) == (1, 90, 0)
        assert (db.neighbourhoods_.cpu().numpy().view(np.uint64) == R.bit_matrix(np.zeros((90, 90)), 0.0)).all()
    one = _fit(same[:1], 0.5, 1)                                     # a single row: its own cluster, or noise
    assert one.labels_.tolist() == [0] and _fit(same[:1], 0.5, 2).labels_.tolist() == [-1]


# ------------------------------------------------------------------ (d) invariances
@pytest.mark.parametrize("metric", [COSINE, EUCLIDEAN])
@pytest.mark.parametrize("N,D", SHAPES)
def test_two_runs_and_row_order(N, D, metric):
    X, _ = R.lattice(N, D, 0.05, metric)
    eps = 0.5295 if metric == EUCLIDEAN else R.cosine_eps(R.distances64(X, metric))
    a, b = _fit(X, eps, 5, NAMES[metric]), _fit(X, eps, 5, NAMES[metric])
    assert torch.equal(a.neighbourhoods_, b.neighbourhoods_) and torch.equal(a.labels_, b.labels_)
    assert torch.equal(a.core_sample_indices_, b.core_sample_indices_)
    perm = np.random.default_rng(N).permutation(N)
    c = _fit(X[perm], eps, 5, NAMES[metric])
    A = R.unpack(a.neighbourhoods_.cpu().numpy(), N)[:, :N]
    Ap = R.unpack(c.neighbourhoods_.cpu().numpy(), N)[:, :N]
    assert np.array_equal(Ap, A[perm][:, perm])                      # a pair's bit does not depend on where it falls in a tile
    labels = c.labels_.cpu().numpy()
    assert R.same_partition(labels, a.labels_.cpu().numpy()[perm])
    assert np.array_equal(labels, R.labels_from_adjacency(Ap, 5)[0])  # the numbering follows the rule in the new order


@pytest.mark.parametrize("N,D", SHAPES[1:])
def test_power_of_two_scaling_changes_no_word(N, D):
    X, _ = R.lattice(N, D, 0.05, EUCLIDEAN)
    base = _graph(X, EUCLIDEAN, 0.5295)
    for e in (20, -20):
        s = np.float32(2.0 ** e)
        got = _graph(X * s, EUCLIDEAN, 0.5295 * 2.0 ** e)
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1]) and got[3] == base[3]


# ------------------------------------------------------------------ (e) memory and alignment
def test_every_output_is_written_exactly_and_misaligned_rows_change_no_word():
    """Every output sits between guard bands at its exact size, poisoned: all of it is written, nothing beside it.  X with a
    row stride, with its base moved by 4 bytes, with a stride that is no multiple of 4 and with D % 4 != 0 (the last column
    of the fixture is zero, so dropping it changes no sum): the words are those of the aligned dense copy."""
    from vit_som_amd import ops
    N, D = 200, 52
    X = np.random.default_rng(4).integers(-9, 10, (N, D)).astype(np.float32)
    X[:, -1] = 0
    D32, _ = SR.exact_euclidean32(X)
    eps, _ = _attained(D32, 0.1)
    dense = _dev(X)
    assert dense.data_ptr() % 16 == 0
    want = R.bit_matrix(D32, eps)
    W = ops.dbscan_words(N)
    variants = {
        "dense": dense,
        "row stride": memcheck.guarded_copy(dense, ld=D + 4)[0],
        "base + 4 bytes": memcheck.guarded_copy(dense, shift=1)[0],
        "stride 53": memcheck.guarded_copy(dense, ld=D + 1)[0],
        "D % 4 != 0": memcheck.guarded_copy(dense, ld=D + 4)[0][:, :D - 1],
    }
    assert variants["base + 4 bytes"].data_ptr() % 16 == 4 and variants["stride 53"].stride(0) == 53
    for what, x in variants.items():
        bufs = {"sq": memcheck.guarded((N,), torch.float32, DEV), "adj": memcheck.guarded((N, W), torch.int64, DEV),
                "count": memcheck.guarded((N,), torch.int32, DEV), "status": memcheck.guarded((2,), torch.int64, DEV),
                "core": memcheck.guarded((N,), torch.uint8, DEV), "root": memcheck.guarded((N,), torch.int32, DEV),
                "changed": memcheck.guarded((1,), torch.int32, DEV), "labels": memcheck.guarded((N,), torch.int64, DEV),
                "record": memcheck.guarded((4,), torch.int32, DEV)}
        v = {k: b[0] for k, b in bufs.items()}
        ops.dbscan_neighbours(x, EUCLIDEAN, eps, v["sq"], v["adj"], v["count"], v["status"])
        ops.dbscan_init(v["count"], 5, v["core"], v["root"])
        for _ in range(64):
            ops.dbscan_round(v["adj"], v["core"], v["root"], 2, v["changed"])
            if not int(v["changed"].item()):
                break
        ops.dbscan_finish(v["adj"], v["core"], v["root"], v["labels"], v["record"])
        torch.cuda.synchronize()
        for k, (_, h) in bufs.items():
            h.all_written(f"{what}: {k}")
            h.check(f"{what}: {k}")
        assert np.array_equal(v["adj"].cpu().numpy().view(np.uint64), want), what
        labels, core, record = R.labels_from_adjacency(R.adjacency(D32, eps), 5)
        assert np.array_equal(v["labels"].cpu().numpy(), labels) and np.array_equal(v["core"].cpu().numpy().astype(bool), core), what
        assert v["record"].tolist() == record and v["status"].tolist() == [0, int(R.popcounts(want, N).sum())], what
    # a precomputed matrix between guard bands, with a row stride
    m32 = memcheck.guarded_copy(_dev(D32), ld=N + 3)[0]
    t = {"adj": memcheck.guarded((N, W), torch.int64, DEV), "count": memcheck.guarded((N,), torch.int32, DEV),
         "status": memcheck.guarded((2,), torch.int64, DEV)}
    ops.dbscan_threshold(m32, eps, t["adj"][0], t["count"][0], t["status"][0])
    torch.cuda.synchronize()
    for k, (_, h) in t.items():
        h.all_written(f"threshold: {k}")
        h.check(f"threshold: {k}")
    assert np.array_equal(t["adj"][0].cpu().numpy().view(np.uint64), want)


# ------------------------------------------------------------------ (f) bad rows
def test_bad_rows():
    from vit_som_amd import DBSCAN
    X, _ = R.lattice(333, 1003, 0.05, EUCLIDEAN)
    for metric in (COSINE, EUCLIDEAN):
        eps = 0.5295 if metric == EUCLIDEAN else R.cosine_eps(R.distances64(X, metric))
        keep = np.ones(333, dtype=bool)
        keep[[5, 200]] = False
        clean = _graph(X[keep], metric, eps)
        A_clean = R.unpack(clean[0], 331)[:, :331]
        for value in (float("nan"), float("inf"), 1e30):             # 1e30: the squared norm overflows
            bad = X.copy()
            bad[5, 17], bad[200, 1000] = value, value
            words, count, _, status = _graph(bad, metric, eps)       # straight to the entry
            assert status[0] == 2 and status[1] == count.sum()
            A = R.check_structure(words, 333, bad=(5, 200))
            assert not A[[5, 200]].any() and not A[:, [5, 200]].any() and count[5] == count[200] == 0
            assert np.array_equal(A[keep][:, keep], A_clean)         # every other row as if they were absent
            with pytest.raises(ValueError, match="not finite"):
                DBSCAN(eps=eps, metric=NAMES[metric]).fit(_dev(bad))


# ------------------------------------------------------------------ (g) precomputed input
@pytest.mark.parametrize("N,D", SHAPES)
def test_precomputed_input(N, D):
    from test_silhouette_gpu import _integers
    from vit_som_amd import ops
    X = _integers(N, D, 5)
    D32, _ = SR.exact_euclidean32(X)
    eps, _ = _attained(D32, 0.1)
    want = _graph(X, EUCLIDEAN, eps)
    for M in (_dev(D32), _dev(D32.astype(np.float64), np.float64)):  # float32 and float64 give the words of (a)
        words, count, status = _threshold(M, eps)
        assert np.array_equal(words, want[0]) and np.array_equal(count, want[1]) and status == [0, int(count.sum())]
    # the fp64 direct form of agglo_distances, thresholded, equals the contraction's words: small integers, eps the root of
    # a half-integer, where fp64's and fp32's roots of the neighbouring integers both keep clear of it
    S = np.random.default_rng(D).integers(0, 4, (N, D))
    S32, _ = SR.exact_euclidean32(S)
    k = int(np.median((S32.astype(np.float64) ** 2)[~np.eye(N, dtype=bool)]).round())
    eps = float(np.sqrt(k + 0.5))
    out, st = torch.empty(N, N, dtype=torch.float64, device=DEV), torch.empty(2, dtype=torch.int32, device=DEV)
    ops.agglo_distances(_dev(S), ops.AGGLO_EUCLIDEAN, False, out, st)
    words, count, status = _threshold(out, eps)
    graph = _graph(S, EUCLIDEAN, eps)
    assert np.array_equal(words, graph[0]) and np.array_equal(count, graph[1]) and 0 < count.sum() - N < N * N - N
    # a NaN entry clears its bit and is counted; the diagonal is set whatever it holds
    M = D32.copy()
    M[3, 7] = M[7, 3] = M[11, 11] = np.nan
    big = float(D32.max()) + 1.0
    words, count, status = _threshold(_dev(M), big)
    A = R.unpack(words, N)
    assert status[0] == 3 and not A[3, 7] and not A[7, 3] and A[11, 11] and A[:, :N].sum() == N * N - 2 and not A[:, N:].any()


def test_precomputed_class_equals_sklearn():
    X, _ = R.lattice(333, 1003, 0.0, EUCLIDEAN)
    D64 = R.distances64(X, EUCLIDEAN)
    want, want_core = _sklearn(D64, 0.5295, 5)
    for M in (_dev(D64, np.float64), _dev(D64)):
        db = _fit(M, 0.5295, 5, "precomputed")
        assert np.array_equal(_host(db)[0], want) and np.array_equal(_host(db)[1], want_core) and db.n_features_in_ == 333
    with pytest.raises(ValueError, match="Precomputed matrix must be square"):
        _fit(_dev(D64[:, :300]), 0.5, 5, "precomputed")
    with pytest.raises(ValueError, match="Negative values"):
        _fit(_dev(-D64), 0.5, 5, "precomputed")
    D64[4, 9] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        _fit(_dev(D64), 0.5, 5, "precomputed")


def test_k_distances():
    from vit_som_amd import k_distances
    X = np.random.default_rng(2).integers(0, 32, (300, 8))
    D32, _ = SR.exact_euclidean32(X)
    for k in (1, 4, 63):
        want = np.sort(np.sort(D32, axis=1)[:, k])                   # column 0 is the row itself
        assert np.array_equal(k_distances(_dev(X), k).cpu().numpy(), want)
    with pytest.raises(ValueError, match="k must be"):
        k_distances(_dev(X), 64)
    with pytest.raises(ValueError, match="below the number of rows"):
        k_distances(_dev(X[:5]), 4)


# ------------------------------------------------------------------ (h) the evaluation path
def _report_arrays(rep):
    return dict(labels=rep.labels.cpu().numpy(), curve=rep.k_distances.cpu().numpy(), sizes=rep.cluster_sizes,
                noise_per_class=rep.noise_per_class,
                scalars=np.array([rep.eps, rep.min_samples, rep.n_clusters, rep.n_core, rep.n_border, rep.n_noise, rep.coverage,
                                  rep.purity, rep.nmi, rep.n_samples], dtype=np.float64))


@pytest.mark.parametrize("name", ["ref_cluster_tiny", "ref_hexa_euclid_tiny"])
def test_evaluate_dbscan_on_the_tiny_fixtures(name, tmp_path):
    from test_knn_gpu import _loaders, _model
    from test_silhouette_gpu import _spread_map
    from vit_som_amd import DBSCAN, DBSCANReport, evaluate_dbscan, k_distances
    from vit_som_amd.evaluation import _som_latents, _Table, nmi_from_table, purity_from_table
    m, cfg = _model(name)
    train, _ = _loaders(cfg, 4)                                    # 96 samples in batches of 10
    _spread_map(m, cfg, train)
    metric = m.som_layer.distance_fcn
    assert metric in ("cosine", "euclidean")
    X, _ = _som_latents(m, cfg, train, "test")
    y = torch.cat([b[1] for b in train]).to(DEV).long()
    rep = evaluate_dbscan(m, cfg, train)
    assert isinstance(rep, DBSCANReport) and (rep.metric, rep.min_samples, rep.n_samples) == (metric, 5, 96)
    curve = k_distances(X, 4, metric)                                # the eps=None rule, reproduced
    assert torch.equal(rep.k_distances, curve) and rep.eps == float(curve[48])
    db = DBSCAN(eps=rep.eps, min_samples=5, metric=metric).fit(X)
    assert torch.equal(rep.labels, db.labels_)
    assert (rep.n_clusters, rep.n_core, rep.n_border, rep.n_noise) == (db.n_clusters_, db.n_core_, db.n_border_, db.n_noise_)
    assert rep.n_core >= 49 and rep.n_core + rep.n_border + rep.n_noise == 96 and rep.coverage == (96 - rep.n_noise) / 96
    labels = db.labels_.cpu().numpy()
    assert np.array_equal(rep.cluster_sizes, np.bincount(labels[labels >= 0], minlength=rep.n_clusters))
    assert rep.n_clusters >= 1
    t = _Table(rep.n_clusters, 256, DEV)
    t.add(db.labels_[db.labels_ >= 0], y[db.labels_ >= 0])
    assert rep.purity == purity_from_table(t.numpy()) and rep.nmi == nmi_from_table(t.numpy())
    assert np.array_equal(rep.noise_per_class, np.bincount(y.cpu().numpy()[labels < 0], minlength=len(rep.noise_per_class)))
    assert rep.noise_per_class.sum() == rep.n_noise
    print(f"{name}: eps {rep.eps:.6g}, {rep.n_clusters} clusters, core / border / noise {rep.n_core, rep.n_border, rep.n_noise}, "
          f"purity {rep.purity:.3f}, nmi {rep.nmi:.3f}")
    given = evaluate_dbscan(m, cfg, train, eps=rep.eps * 0.5, min_samples=3, metric="euclidean")
    want = DBSCAN(eps=rep.eps * 0.5, min_samples=3, metric="euclidean").fit(X)
    assert torch.equal(given.labels, want.labels_) and given.metric == "euclidean" and given.eps == rep.eps * 0.5
    nothing = evaluate_dbscan(m, cfg, train, eps=1e-30, min_samples=96)
    assert nothing.n_clusters == 0 and nothing.n_noise == 96 and np.isnan(nothing.purity) and np.isnan(nothing.nmi)
    assert nothing.cluster_sizes.size == 0 and nothing.coverage == 0.0
    with pytest.raises(ValueError, match="metric must be"):
        evaluate_dbscan(m, cfg, train, metric="manhattan")


def _dp_worker(rank, world, port, out):
    import torch.distributed as dist
    from test_knn_gpu import _loaders, _model
    from test_silhouette_gpu import _spread_map
    from vit_som_amd import evaluate_dbscan
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    m, cfg = _model("ref_cluster_tiny")
    train, _ = _loaders(cfg, 4)
    _spread_map(m, cfg, train)                                   # as one process: before the model learns of the ranks
    m.world_size, m.rank = world, rank
    rep = evaluate_dbscan(m, cfg, [b for i, b in enumerate(train) if i % world == rank])
    np.savez(f"{out}.{rank}.npz", **_report_arrays(rep))
    dist.barrier()
    dist.destroy_process_group()


def test_evaluate_dbscan_two_ranks(tmp_path):
    """Both ranks gather all rows (50 + 46, rank 0's first) and return bit-identical reports: that of one process over the
    rows in that order."""
    import torch.multiprocessing as mp
    from test_distributed import _free_port
    from test_knn_gpu import _loaders, _model
    from test_silhouette_gpu import _spread_map
    from vit_som_amd import evaluate_dbscan
    out = str(tmp_path / "dbscan")
    mp.spawn(_dp_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    r0, r1 = np.load(f"{out}.0.npz"), np.load(f"{out}.1.npz")
    m, cfg = _model("ref_cluster_tiny")
    train, _ = _loaders(cfg, 4)
    _spread_map(m, cfg, train)
    single = _report_arrays(evaluate_dbscan(m, cfg, train[0::2] + train[1::2]))
    assert set(r0.files) == set(r1.files) == set(single)
    for key, want in single.items():
        assert r0[key].tobytes() == r1[key].tobytes() == want.tobytes(), key


def test_driver_reports_dbscan(tmp_path):
    from vit_som_amd.train import main, synthetic_loaders
    _, cfg = load_golden("ref_cluster_tiny")
    cfg = copy.deepcopy(cfg)
    cfg["hyperparameters"]["batch_size"] = 16
    logs = []
    loaders = lambda c, r, w: synthetic_loaders(c, r, w, n_train=64, n_val=16, n_test=16)      # noqa: E731
    today = {"accuracy", "precision", "recall", "f1", "purity", "nmi", "run_duration", "inference_time"}
    met = main(cfg, n_runs=1, max_epochs=1, make_loaders=loaders, model_states_dir=str(tmp_path / "a"), log=logs.append,
               dbscan_eval=True)
    assert set(met) == today | {"dbscan_clusters", "dbscan_noise", "dbscan_purity", "dbscan_nmi"}
    assert all(len(met[k]) == 1 for k in ("dbscan_clusters", "dbscan_noise", "dbscan_purity", "dbscan_nmi"))
    assert 0 <= met["dbscan_noise"][0] <= 64 and met["dbscan_clusters"][0] >= 0
    print([l for l in logs if "DBSCAN" in l])
    assert any(l.startswith("DBSCAN:") for l in logs)
