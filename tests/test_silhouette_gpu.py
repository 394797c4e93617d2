"""Silhouette on the MI355X: vsom_silhouette and silhouette.py against the restatement (silhouette_ref.py) on integer data
where fp32 decides exactly, against sklearn in fp64, bit for bit under permutations of the rows, at the edges of the
cluster count, under power-of-two scaling and on bad input; evaluate_silhouette, visualize_silhouette_map and the driver
on the tiny fixtures."""
import copy
import os
import signal

import numpy as np
import pytest
import torch

import silhouette_ref as R
from helpers import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COSINE, EUCLIDEAN = R.COSINE, R.EUCLIDEAN
NAMES = {COSINE: "cosine", EUCLIDEAN: "euclidean"}
SHAPES = [(257, 12288), (333, 1003), (130, 3)]        # two row blocks + 1 and 16-byte loads; element-wise loads; tiny D
FIELDS = ("sil", "a", "b", "nearest", "counts", "cluster_mean", "score")


@pytest.fixture(autouse=True)
def time_limit(request):
    """A limit of its own (seconds) for every test here, as in test_randaug_gpu.py: a SIGALRM handler ends a test whose
    host side is slow or loops."""
    limit = 300 if "driver" in request.node.name or "ranks" in request.node.name else 120

    def expired(signum, frame):
        raise TimeoutError(f"{request.node.name}: no result after {limit} s")
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(limit)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _lab(y):
    return torch.from_numpy(np.ascontiguousarray(y, dtype=np.int64)).to(DEV)


def _run(X, y, metric, C, sums=False):
    """One ops.silhouette call -> dict of host arrays (and the int64 sums [N, C] when asked)."""
    from vit_som_amd import ops
    X = X if isinstance(X, torch.Tensor) else _dev(X)
    ws = ops.silhouette_workspace(X.shape[0], C, DEV) if sums else None
    r = ops.silhouette(X, _lab(y), metric, C, ws=ws)
    out = {k: getattr(r, k).cpu().numpy() for k in FIELDS}
    out["score"], out["status"] = float(out["score"][0]), r.status
    if sums:
        out["sums"] = r.sums.cpu().numpy()
    return out


def _same(a, b, rows=None):
    """Bit for bit: every field of two runs (`rows`: b's rows are a's in that order)."""
    for k in FIELDS:
        x, y = a[k], b[k]
        if rows is not None and k in ("sil", "a", "b", "nearest"):
            x = x[rows]
        assert np.array_equal(np.asarray(x).view(np.int64), np.asarray(y).view(np.int64)), k
    assert a["status"] == b["status"]


def _integers(N, D, seed):
    """Integer rows whose dot products and norms stay below 2^23."""
    hi = int(np.sqrt(2 ** 23 / D))
    return np.random.default_rng(seed).integers(-hi, hi + 1, (N, D))


def _labels(N, C, seed):
    y = np.random.default_rng(seed).integers(0, C, N)
    y[:C] = np.arange(C)
    return y


def _blobs(N, D, C, seed):
    rng = np.random.default_rng(seed)
    y = _labels(N, C, seed + 1)
    return ((rng.standard_normal((C, D)) * 0.5)[y] + rng.standard_normal((N, D))).astype(np.float32), y


def _close(got, want, tol, what):
    """|got - want| <= tol relative to max(1, |want|): sil is in [-1, 1], a and b scale with the data."""
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"{what}: largest error {err.max():.3e} (bound {tol:.3e})")
    assert err.max() <= tol, what


# ------------------------------------------------------------------ (a) exact, euclidean
@pytest.mark.parametrize("N,D", SHAPES)
def test_exact_on_integer_data(N, D):
    """Every squared distance is an integer exact in fp32 and sqrtf is correctly rounded: the device's int64 sums ARE the
    restatement's; sil, a and b are then at most three correctly rounded fp64 operations each, 1e-15.  Against sklearn in
    fp64 the only difference is the rounding of sqrtf, 2^-24 relative per distance, carried through a, b and the
    quotient: 4 x 2^-24."""
    from sklearn.metrics import silhouette_samples
    X, y, C = _integers(N, D, 5), _labels(N, 7, 6), 7
    D32, M = R.exact_euclidean32(X)
    S, want = R.device_restatement(D32, y, C, M, EUCLIDEAN)
    got = _run(X, y, EUCLIDEAN, C, sums=True)
    assert np.array_equal(got["sums"], S)
    for k in ("sil", "a", "b"):
        _close(got[k], want[k], 1e-15, f"({N}, {D}) {k} against the restatement")
    assert np.array_equal(got["nearest"], want["nearest"]) and np.array_equal(got["counts"], want["counts"])
    assert np.array_equal(got["cluster_mean"], want["cluster_mean"]) and got["score"] == want["score"]
    assert got["status"] == want["status"] == [0, 0, 7, 0]
    s64, a64, b64 = R.silhouette_fp64(R.distances(X, EUCLIDEAN), y)
    assert np.abs(s64 - silhouette_samples(X.astype(np.float64), y)).max() <= 1e-12
    for k, ref in (("sil", s64), ("a", a64), ("b", b64)):
        _close(got[k], ref, 4 * 2.0 ** -24, f"({N}, {D}) {k} against fp64")


@pytest.mark.parametrize("N", [3000, 4300])
def test_many_column_chunks_equal_the_restatement(N):
    """Several column chunks, combined by integer atomics: N = 3000 runs 47 chunks of one tile, N = 4300 is the first size
    range at which a chunk holds more than one tile.  D = 8 takes the 16-byte loads."""
    X, y, C = np.random.default_rng(N).integers(0, 32, (N, 8)), _labels(N, 7, N), 7
    D32, M = R.exact_euclidean32(X)
    got = _run(X, y, EUCLIDEAN, C, sums=True)
    assert np.array_equal(got["sums"], R.fixed_sums(D32, y, C, R.bound_exponent(M, EUCLIDEAN)))
    assert got["status"] == [0, 0, 7, 0]


@pytest.mark.parametrize("N,D", [(200, 132), (150, 300), (200, 133), (140, 257)])
def test_segment_tails(N, D):
    """Dot products and norms are summed in segments of 128 k-values.  D = 132 and 300 take the 16-byte loads with a last
    segment of 4 and of 44 values (no multiple of the 32-wide k-tile), 133 and 257 the element-wise loads with one of 5 and
    of 1.  Integer data: every product is counted exactly once, so the sums are the restatement's.  One real-valued row
    repeated N times: a pair's segments are bit for bit the norms' segments, every distance is exactly 0, both metrics."""
    X, y, C = _integers(N, D, D), _labels(N, 5, D), 5
    D32, M = R.exact_euclidean32(X)
    got = _run(X, y, EUCLIDEAN, C, sums=True)
    assert np.array_equal(got["sums"], R.fixed_sums(D32, y, C, R.bound_exponent(M, EUCLIDEAN)))
    assert got["status"] == [0, 0, 5, 0]
    row = np.random.default_rng(D).standard_normal((1, D)).astype(np.float32)
    for metric in (EUCLIDEAN, COSINE):
        same = _run(np.tile(row, (N, 1)), np.arange(N) % 2, metric, 2, sums=True)
        assert not same["sums"].any() and (same["sil"] == 0).all() and (same["a"] == 0).all() and (same["b"] == 0).all()
        assert same["status"] == [0, 0, 2, 0]


# ------------------------------------------------------------------ (b) the order of the rows
@pytest.mark.parametrize("metric", [COSINE, EUCLIDEAN])
@pytest.mark.parametrize("N,D", SHAPES)
def test_row_order_changes_no_bit(N, D, metric):
    """Interleaved labels (i % C: no two adjacent columns share one, every lane is a run head), the same rows sorted by
    label (long runs) and shuffled: every output is bit for bit the same after un-permuting, and two consecutive calls
    are bit for bit equal.  C = 300 exceeds some N: clusters of one and empty clusters."""
    rng = np.random.default_rng(N + metric)
    X = rng.standard_normal((N, D)).astype(np.float32)
    Xd = _dev(X)
    for C in (2, 7, 300):
        y = np.arange(N) % C
        base = _run(Xd, y, metric, C)
        _same(base, _run(Xd, y, metric, C))
        assert base["status"][:2] == [0, 0] and np.isfinite(base["sil"]).all()
        for rows in (np.argsort(y, kind="stable"), rng.permutation(N)):
            _same(base, _run(Xd[torch.from_numpy(rows).to(DEV)].contiguous(), y[rows], metric, C), rows)


def test_wrapper_sorts_rows_or_not_with_the_same_result():
    from vit_som_amd import SilhouetteReport, cluster_silhouette, silhouette_samples, silhouette_score
    X, y = _blobs(333, 1003, 7, 3)
    Xd, yd = _dev(X), _lab(np.array([5, -2, 10 ** 12, 44, 45, 46, 900])[y])         # labels need not be dense
    a, b = cluster_silhouette(Xd, yd, sort_rows=True), cluster_silhouette(Xd, yd, sort_rows=False)
    assert isinstance(a, SilhouetteReport) and a.per_sample.dtype == torch.float64 and a.per_sample.is_cuda
    assert torch.equal(a.per_sample, b.per_sample) and torch.equal(a.nearest_cluster, b.nearest_cluster) and a.score == b.score
    assert np.array_equal(a.per_cluster, b.per_cluster) and np.array_equal(a.counts, b.counts)
    assert (a.n_clusters, a.n_samples, a.metric) == (7, 333, "euclidean")
    assert np.array_equal(a.labels_, [-2, 5, 44, 45, 46, 900, 10 ** 12]) and np.array_equal(a.counts, np.bincount(y)[[1, 0, 3, 4, 5, 6, 2]])
    assert torch.equal(silhouette_samples(Xd, yd), a.per_sample) and silhouette_score(Xd, yd) == a.score
    # the entry without its optional outputs
    from vit_som_amd import ops
    dense = _lab(np.array([1, 0, 6, 2, 3, 4, 5])[y])
    lean, full = ops.silhouette(Xd, dense, EUCLIDEAN, 7, details=False), ops.silhouette(Xd, dense, EUCLIDEAN, 7)
    assert lean.a is None and lean.b is None and lean.nearest is None
    assert torch.equal(lean.sil, full.sil) and torch.equal(full.sil, a.per_sample) and torch.equal(lean.score, full.score)
    # sample_size: sklearn's draw
    rows = np.random.RandomState(4).permutation(333)[:100]
    sub = cluster_silhouette(_dev(X[rows]), yd[torch.from_numpy(rows).to(DEV)])
    assert silhouette_score(Xd, yd, sample_size=100, random_state=4) == sub.score


# ------------------------------------------------------------------ (c) the edges of the cluster count
def test_cluster_count_edges():
    from sklearn.metrics import silhouette_samples
    from vit_som_amd import cluster_silhouette
    N = 130
    X = _integers(N, 3, 8)
    D32, M = R.exact_euclidean32(X)
    single = np.arange(N) % 4
    single[single == 3] = 0
    single[77] = 3                                                   # cluster 3: row 77 alone
    for what, y in (("C = 2", np.arange(N) % 2), ("C = N - 1", np.minimum(np.arange(N), N - 2)), ("a singleton", single)):
        C = int(y.max()) + 1
        S, want = R.device_restatement(D32, y, C, M, EUCLIDEAN)
        got = _run(X, y, EUCLIDEAN, C, sums=True)
        assert np.array_equal(got["sums"], S), what
        for k in ("sil", "a", "b"):
            _close(got[k], want[k], 1e-15, f"{what}: {k} against the restatement")
        for k in ("nearest", "counts", "cluster_mean", "score"):
            assert np.array_equal(got[k], want[k], equal_nan=True), (what, k)
        assert got["status"] == want["status"]
        _close(got["sil"], silhouette_samples(X.astype(np.float64), y), 4 * 2.0 ** -24, what)
        rep = cluster_silhouette(_dev(X), _lab(y))
        assert np.array_equal(rep.per_sample.cpu().numpy(), got["sil"]) and rep.score == got["score"] and rep.n_clusters == C
    assert got["sil"][77] == 0.0 and got["a"][77] == 0.0 and got["status"][3] == 1
    assert _run(X, np.minimum(np.arange(N), N - 2), EUCLIDEAN, N - 1)["status"] == [0, 0, N - 1, N - 2]

    # a cluster id in range without a member: skipped for b, NaN in per_cluster, not counted as a label
    y = np.array([0, 2, 5])[np.arange(N) % 3]
    rep = cluster_silhouette(_dev(X), _lab(y), n_clusters=7)
    assert rep.n_clusters == 7 and np.array_equal(rep.counts > 0, [True, False, True, False, False, True, False])
    assert np.array_equal(np.isnan(rep.per_cluster), rep.counts == 0)
    assert set(rep.nearest_cluster.cpu().numpy()) <= {0, 2, 5}
    _close(rep.per_sample.cpu().numpy(), silhouette_samples(X.astype(np.float64), y), 4 * 2.0 ** -24, "empty clusters")
    dense = cluster_silhouette(_dev(X), _lab(y))
    assert torch.equal(dense.per_sample, rep.per_sample) and dense.score == rep.score and dense.n_clusters == 3
    assert np.array_equal(dense.per_cluster, rep.per_cluster[[0, 2, 5]])
    with pytest.raises(ValueError, match=r"Number of labels is 1\. Valid values are 2 to n_samples - 1 \(inclusive\)"):
        cluster_silhouette(_dev(X), _lab(np.full(N, 4)), n_clusters=7)
    with pytest.raises(ValueError, match="Number of labels is 1"):
        cluster_silhouette(_dev(X), _lab(np.full(N, 4)))
    with pytest.raises(ValueError, match=f"Number of labels is {N}"):
        cluster_silhouette(_dev(X), _lab(np.arange(N) * 3))
    with pytest.raises(ValueError, match="outside"):
        cluster_silhouette(_dev(X), _lab(np.arange(N) % 8), n_clusters=7)

    # all rows identical, two clusters: a = b = 0, every s = 0
    for metric in (EUCLIDEAN, COSINE):
        got = _run(np.tile(np.float32([[3.5, -1.25, 7.0]]), (N, 1)), np.arange(N) % 2, metric, 2)
        assert (got["sil"] == 0).all() and (got["a"] == 0).all() and (got["b"] == 0).all() and got["score"] == 0.0
        assert got["status"] == [0, 0, 2, 0]


# ------------------------------------------------------------------ (d) the unit follows the data
@pytest.mark.parametrize("metric", [COSINE, EUCLIDEAN])
@pytest.mark.parametrize("N,D", SHAPES[1:])
def test_power_of_two_scaling_changes_no_bit(N, D, metric):
    """X 2^20 and X 2^-20: every fp32 operation of the contraction scales exactly, the bound's exponent moves by 20, the
    fixed-point values are the same integers: sil is bit for bit that of X."""
    X, y = _blobs(N, D, 5, 9)
    base = _run(X, y, metric, 5, sums=True)
    for scale in (2.0 ** 20, 2.0 ** -20):
        got = _run(X * np.float32(scale), y, metric, 5, sums=True)
        assert np.array_equal(got["sums"], base["sums"])
        assert np.array_equal(got["sil"].view(np.int64), base["sil"].view(np.int64)) and got["score"] == base["score"]
        if metric == EUCLIDEAN:
            assert np.array_equal(got["a"], base["a"] * scale)


# ------------------------------------------------------------------ (e) real-valued data against sklearn
def _fp32_error(X, y, metric):
    """e32: the largest error of the same silhouette computed from torch.cdist in plain fp32 on the CPU (cosine: half the
    squared cdist of the rows normalised in fp32), against fp64 -- the project's rule of tests/numeric_edges.py."""
    s64 = R.silhouette_fp64(R.distances(X, metric), y)[0]
    Xt = torch.from_numpy(X)
    if metric == COSINE:
        Xt = Xt / Xt.norm(dim=1, keepdim=True)
        D32 = 0.5 * torch.cdist(Xt, Xt) ** 2
    else:
        D32 = torch.cdist(Xt, Xt)
    D32 = D32.numpy().astype(np.float64)
    np.fill_diagonal(D32, 0.0)
    return s64, float(np.abs(R.silhouette_fp64(D32, y)[0] - s64).max())


def _against_sklearn(X, y, metric, what):
    from sklearn.metrics import silhouette_samples, silhouette_score
    from vit_som_amd import cluster_silhouette
    s64, e32 = _fp32_error(X, y, metric)
    want = silhouette_samples(X.astype(np.float64), y, metric=NAMES[metric])
    assert np.abs(want - s64).max() <= 1e-9
    tol = 4 * max(e32, 2.0 ** -23)
    rep = cluster_silhouette(_dev(X), _lab(y), metric=NAMES[metric])
    err = float(np.abs(rep.per_sample.cpu().numpy() - want).max())
    print(f"{what} {NAMES[metric]}: e32 {e32:.3e}, tolerance {tol:.3e}, device error {err:.3e}, score {rep.score:.6f}")
    assert err <= tol
    assert abs(rep.score - silhouette_score(X.astype(np.float64), y, metric=NAMES[metric])) <= tol


@pytest.mark.parametrize("metric", [COSINE, EUCLIDEAN])
@pytest.mark.parametrize("N,D", SHAPES)
def test_blobs_against_sklearn(N, D, metric):
    """Tolerance 4 max(e32, 2^-23); e32, the tolerance and the device's error are printed.  The largest shape is the one
    that decides how the entry sums: with one fp32 chain over the 12 288 products of a norm the cosine case is off by
    5e-7 and misses; summed in segments of 128 it passes (Silhouette)."""
    X, y = _blobs(N, D, 6, 11)
    _against_sklearn(X, y, metric, f"blobs ({N}, {D})")


@pytest.mark.parametrize("metric", [COSINE, EUCLIDEAN])
def test_golden_latents_against_sklearn(metric):
    """The latents (D = 256) lie close together -- cosine distances of 1e-4 within a cluster, where 1 - cos cancels -- so
    fp32 itself is far off and the tolerance follows e32; the figures are printed."""
    from test_knn_gpu import _features, _loaders, _model
    m, cfg = _model("ref_cluster_tiny")
    train, _ = _loaders(cfg, 4)
    X, y = _features(m, cfg, train)
    _against_sklearn(X.cpu().numpy(), y.cpu().numpy(), metric, "golden latents")


# ------------------------------------------------------------------ (f) bad input
def test_bad_input():
    from vit_som_amd import cluster_silhouette, ops
    X, y = _blobs(333, 1003, 5, 13)
    for value in (float("nan"), 1e30, float("inf")):
        bad = X.copy()
        bad[200, 17] = value                                         # 1e30: the squared norm overflows
        for metric in (COSINE, EUCLIDEAN):
            with pytest.raises(ValueError, match="not finite"):
                ops.silhouette(_dev(bad), _lab(y), metric, 5)
            with pytest.raises(ValueError, match="not finite"):
                cluster_silhouette(_dev(bad), _lab(y), metric=NAMES[metric])

    # a label outside the range, straight to the entry: NaN for that row, counted, the others as if it were absent --
    # even when it is the row with the largest norm, which would otherwise set the unit
    for label in (5, -1, 2 ** 40):
        for metric in (COSINE, EUCLIDEAN):
            big = X.copy()
            big[200] *= 1000.0
            y_bad = y.copy()
            y_bad[200] = label
            got = _run(big, y_bad, metric, 5)
            assert got["status"][:2] == [1, 0]
            assert np.isnan(got["sil"][200]) and np.isnan(got["a"][200]) and np.isnan(got["b"][200]) and got["nearest"][200] == -1
            keep = np.arange(333) != 200
            _same(got | {"status": [0] + got["status"][1:]}, _run(big[keep], y[keep], metric, 5), np.flatnonzero(keep))

    # norms that underflow to 0: every distance is 0, every s = 0
    tiny = (X * np.float32(1e-30)).astype(np.float32)
    for metric in (COSINE, EUCLIDEAN):
        got = _run(tiny, y, metric, 5)
        assert (got["sil"] == 0).all() and got["score"] == 0.0 and got["status"] == [0, 0, 5, 0]


# ------------------------------------------------------------------ (g) the evaluation path
def _spread_map(m, cfg, loader):
    """The golden states are untrained and put every sample on one unit, where no silhouette exists: place the prototypes
    on K of the loader's own latents, so that the samples spread over the map."""
    from vit_som_amd.evaluation import _som_latents
    som = m.som_layer
    X, _ = _som_latents(m, cfg, loader, "test")
    rows = torch.linspace(0, X.shape[0] - 1, som.n_prototypes, device=DEV).long()
    with torch.no_grad():
        som.prototypes.copy_(X[rows])
    som.invalidate_planes()


@pytest.mark.parametrize("name", ["ref_cluster_tiny", "ref_hexa_euclid_tiny"])
def test_evaluate_silhouette_on_the_tiny_fixtures(name, tmp_path):
    from test_knn_gpu import _loaders, _model
    from vit_som_amd import SilhouetteReport, cluster_silhouette, evaluate_silhouette, visualize_silhouette_map
    from vit_som_amd.evaluation import _som_latents
    from vit_som_amd.kmeans import KMeans
    m, cfg = _model(name)
    som = m.som_layer
    train, _ = _loaders(cfg, 4)                                    # 96 samples in batches of 10
    _spread_map(m, cfg, train)
    metric = som.distance_fcn
    assert metric in ("cosine", "euclidean")
    X, units = _som_latents(m, cfg, train, "test")
    assert X.shape[0] == units.shape[0] == 96 and X.dtype == torch.float32 and units.dtype == torch.int64
    d = cfg["data"]
    bmu = torch.cat([m.predict(x.to(DEV).reshape(-1, d["num_channels"], d["input_size"], d["input_size"]))[0].clone() for x, _ in train])
    assert torch.equal(units, bmu)

    rep = evaluate_silhouette(m, cfg, train)
    want = cluster_silhouette(X, units, metric=metric, n_clusters=som.n_prototypes)
    assert isinstance(rep, SilhouetteReport) and (rep.metric, rep.n_samples, rep.n_clusters) == (metric, 96, som.n_prototypes)
    assert rep.score == want.score and torch.equal(rep.per_sample, want.per_sample) and -1.0 <= rep.score <= 1.0
    assert np.array_equal(rep.per_cluster, want.per_cluster, equal_nan=True)
    assert np.array_equal(rep.counts, torch.bincount(units, minlength=som.n_prototypes).cpu().numpy())
    assert np.array_equal(np.isnan(rep.per_cluster), rep.counts == 0) and 2 <= (rep.counts > 0).sum() < 96

    km = evaluate_silhouette(m, cfg, train, clusters="kmeans", n_clusters=4, metric="euclidean")
    labels = KMeans(n_clusters=4, random_state=0, n_init=10).fit_predict(X).long()
    want = cluster_silhouette(X, labels, metric="euclidean")
    assert km.score == want.score and torch.equal(km.per_sample, want.per_sample) and km.n_clusters == 4 and km.metric == "euclidean"

    sub = evaluate_silhouette(m, cfg, train, sample_size=50)
    rows = torch.from_numpy(np.random.RandomState(0).permutation(96)[:50]).to(DEV)
    assert sub.n_samples == 50 and sub.score == cluster_silhouette(X[rows].contiguous(), units[rows], metric=metric,
                                                                   n_clusters=som.n_prototypes).score
    with pytest.raises(ValueError, match="clusters must be"):
        evaluate_silhouette(m, cfg, train, clusters="labels")

    values = visualize_silhouette_map(m, cfg, train, output_dir=str(tmp_path))
    assert values.shape == tuple(som.map_size) and np.array_equal(values.ravel(), rep.per_cluster, equal_nan=True)
    files = os.listdir(tmp_path)
    assert len(files) == 1 and files[0].endswith("_silhouette_map.png") and os.path.getsize(tmp_path / files[0]) > 0


def _dp_worker(rank, world, port, out):
    import torch.distributed as dist
    from test_knn_gpu import _loaders, _model
    from vit_som_amd import evaluate_silhouette
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    m, cfg = _model("ref_cluster_tiny")
    train, _ = _loaders(cfg, 4)
    _spread_map(m, cfg, train)                                   # as one process: before the model learns of the ranks
    m.world_size, m.rank = world, rank
    rep = evaluate_silhouette(m, cfg, [b for i, b in enumerate(train) if i % world == rank])
    np.savez(f"{out}.{rank}.npz", sil=rep.per_sample.cpu().numpy(), per_cluster=rep.per_cluster, counts=rep.counts,
             scalars=np.array([rep.score, rep.n_samples], dtype=np.float64))
    dist.barrier()
    dist.destroy_process_group()


def test_evaluate_silhouette_two_ranks(tmp_path):
    """Both ranks gather all rows (50 + 46, rank 0's first) and return the same report: that of one process over the rows
    in that order."""
    import torch.multiprocessing as mp
    from test_distributed import _free_port
    from test_knn_gpu import _loaders, _model
    from vit_som_amd import evaluate_silhouette
    out = str(tmp_path / "sil")
    mp.spawn(_dp_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    r0, r1 = np.load(f"{out}.0.npz"), np.load(f"{out}.1.npz")
    for key in ("sil", "per_cluster", "counts", "scalars"):
        assert np.array_equal(r0[key], r1[key], equal_nan=True), key
    m, cfg = _model("ref_cluster_tiny")
    train, _ = _loaders(cfg, 4)
    _spread_map(m, cfg, train)
    single = evaluate_silhouette(m, cfg, train[0::2] + train[1::2])
    assert r0["scalars"].tolist() == [single.score, 96.0]
    assert np.array_equal(r0["sil"], single.per_sample.cpu().numpy()) and np.array_equal(r0["counts"], single.counts)


def _whole_set_entries(m, cfg, loader):
    """What the three entries that collect the whole set on every rank return on `loader`, as host arrays."""
    from vit_som_amd.evaluation import evaluate_kmeans, evaluate_latent_spectrum, evaluate_silhouette
    purity, nmi, _ = evaluate_kmeans(m, cfg, loader)
    sil = evaluate_silhouette(m, cfg, loader)
    spec = evaluate_latent_spectrum(m, cfg, loader)
    return dict(kmeans=np.array([purity, nmi], dtype=np.float64), score=np.array([sil.score], dtype=np.float64),
                per_cluster=sil.per_cluster, counts=sil.counts, explained_variance=spec.explained_variance,
                total_variance=np.array([spec.total_variance], dtype=np.float64))


def _whole_set_worker(rank, world, port, out):
    import torch.distributed as dist
    from test_knn_gpu import _loaders, _model
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    m, cfg = _model("ref_cluster_tiny")
    train, _ = _loaders(cfg, 4)
    _spread_map(m, cfg, train)                                   # as one process: before the model learns of the ranks
    m.world_size, m.rank = world, rank
    np.savez(f"{out}.{rank}.npz", **_whole_set_entries(m, cfg, train[:5] if rank == 0 else train[5:]))
    dist.barrier()
    dist.destroy_process_group()


def test_whole_set_entries_two_ranks(tmp_path):
    """evaluate_kmeans, evaluate_silhouette and evaluate_latent_spectrum share one collector: every rank gathers all rows,
    rank 0's first.  The 96 samples are dealt in contiguous halves (batches 0-4: 50 rows, batches 5-9: 46 rows), so the
    gathered rows are the single-process rows in the single-process order, and both ranks must return bit for bit what
    one process returns on the whole loader."""
    import torch.multiprocessing as mp
    from test_distributed import _free_port
    from test_knn_gpu import _loaders, _model
    out = str(tmp_path / "whole")
    mp.spawn(_whole_set_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    m, cfg = _model("ref_cluster_tiny")
    train, _ = _loaders(cfg, 4)
    assert len(train) == 10
    _spread_map(m, cfg, train)
    single = _whole_set_entries(m, cfg, train)
    assert single["counts"].sum() == 96 and single["explained_variance"].size >= 2
    for rank in (0, 1):
        got = np.load(f"{out}.{rank}.npz")
        assert set(got.files) == set(single)
        for key, want in single.items():
            assert got[key].dtype == want.dtype and got[key].shape == want.shape, (rank, key)
            assert got[key].tobytes() == want.tobytes(), (rank, key)


def test_an_empty_loader_is_a_value_error():
    """Every entry that collects the whole set names itself and the empty loader, whatever it reads from the model."""
    from test_knn_gpu import _model
    from vit_som_amd import evaluation as ev
    m, cfg = _model("ref_cluster_tiny")
    for name in ("evaluate_kmeans", "evaluate_silhouette", "evaluate_latent_spectrum", "evaluate_embedding_quality",
                 "visualize_umap_progression", "visualize_umap_map", "visualize_pca_map", "init_som_from_data", "fit_som_batch"):
        with pytest.raises(ValueError, match=f"^{name}: the loader is empty$"):
            getattr(ev, name)(m, cfg, [])
    m.train()
    with pytest.raises(ValueError, match="empty"):
        ev.fit_som_batch(m, cfg, [])
    assert m.training and torch.is_grad_enabled()                  # both modes are restored on the error path too


def test_driver_reports_silhouette_bmu(tmp_path):
    from vit_som_amd.train import main, synthetic_loaders
    _, cfg = load_golden("ref_cluster_tiny")
    cfg = copy.deepcopy(cfg)
    cfg["hyperparameters"]["batch_size"] = 16
    logs = []
    loaders = lambda c, r, w: synthetic_loaders(c, r, w, n_train=64, n_val=16, n_test=16)      # noqa: E731
    today = {"accuracy", "precision", "recall", "f1", "purity", "nmi", "run_duration", "inference_time"}
    met = main(cfg, n_runs=1, max_epochs=1, make_loaders=loaders, model_states_dir=str(tmp_path / "a"), log=logs.append,
               silhouette=True)
    assert set(met) == today | {"silhouette_bmu"}
    (s,) = met["silhouette_bmu"]
    assert np.isfinite(s) and -1.0 <= s <= 1.0
    print([l for l in logs if "ilhouette" in l])
    assert any("silhouette_bmu" in l for l in logs)
