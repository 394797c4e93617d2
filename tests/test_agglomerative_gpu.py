"""Agglomerative clustering on the MI355X: the distance pass against numpy's direct form, the merge loop against scipy from the
same bits, whole fits, ties, connectivity, and evaluate_map_clusters on the golden models.

Tolerances.  The squared euclidean and the manhattan sums have non-negative terms, so any order of D terms is within
D 2^-52 relative of any other; the cosine distance is within (D + 4) 2^-52 absolute.  Single and complete linkage are min
and max: exact.  An average height is within 3 (N - 1) 2^-53 relative; a Ward height within the larger of that and four
times the error of the restatement's loop (agglomerative_ref.py) against scipy on the same fixture: two fp64 orders of the
same arithmetic, the project's 4 x yardstick rule."""
import copy
import functools

import numpy as np
import pytest
import torch

import agglomerative_ref as R
import memcheck as MC
from helpers import load_golden
from vit_som_amd import AgglomerativeClustering, MapClustersReport, evaluate_map_clusters

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
DIST_SHAPES = ((2, 1), (65, 3), (130, 257), (257, 130), (33, 12288))
MERGE_N = (2, 3, 64, 65, 257, 600, 1025)          # 1025: the pick kernel's 1024 threads take a second slot each
LINK = {"ward": 0, "average": 1, "complete": 2, "single": 3}
METRIC = {"euclidean": 0, "manhattan": 1, "cosine": 2}


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device="cuda", dtype=dtype or t.dtype).contiguous()


@functools.lru_cache(maxsize=None)
def dist_fixture(N, D, metric):
    X = R.gaussian_rows(N, D, 7 * N + D)
    return X, R.distance_matrix(X, metric, squared=True)


def _layouts(X):
    """(name, view, handle): the same rows contiguous, with a padded row stride, and one float off 16-byte alignment."""
    t = _dev(X)
    N, D = t.shape
    yield ("contiguous",) + MC.guarded_copy(t)
    yield ("padded",) + MC.guarded_copy(t, ld=D + 4)
    flat, h = MC.guarded((N * D + 1,), torch.float32, "cuda")
    flat[1:].copy_(t.reshape(-1))
    flat[:1].fill_(float("nan"))
    yield "offset", flat[1:].view(N, D), h


def _distances(x, metric, squared=True):
    from vit_som_amd import ops
    N = x.shape[0]
    out, ho = MC.guarded((N, N), torch.float64, "cuda")
    status, hs = MC.guarded((2,), torch.int32, "cuda")
    ops.agglo_distances(x, METRIC[metric], squared, out, status)
    torch.cuda.synchronize()
    ho.check("out"); ho.all_written("out"); hs.check("status"); hs.all_written("status")
    return out.cpu().numpy(), status.cpu().numpy()


# ------------------------------------------------------------------ the distance pass
@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("shape", DIST_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_distance_pass_against_the_direct_form(shape, metric):
    N, D = shape
    X, want = dist_fixture(N, D, metric)
    first = None
    for name, x, hx in _layouts(X):
        got, status = _distances(x, metric)
        hx.check(f"X ({name})")
        assert not status.any(), (name, status)
        assert np.array_equal(got, got.T), f"{name}: the two halves differ"
        assert not got.diagonal().any(), f"{name}: the diagonal is not zero"
        if metric == "cosine":
            err, bound = np.abs(got - want).max(), (D + 4) * EPS
        else:
            off = ~np.eye(N, dtype=bool)
            err, bound = (np.abs(got - want)[off] / want[off]).max(), D * EPS
        print(f"{N}x{D} {metric} {name}: error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (name, err, bound)
        if first is None:
            first = got
        assert np.array_equal(got, first), f"{name}: the 16-byte and the element path add the columns in one order"
    if metric == "euclidean":                       # the root is the correctly rounded one of the squared sum
        rooted, _ = _distances(_dev(X), metric, squared=False)
        assert np.array_equal(rooted, np.sqrt(first))


@pytest.mark.parametrize("metric", R.METRICS)
def test_duplicated_rows_are_at_exactly_zero(metric):
    X = R.gaussian_rows(130, 257, 3)
    X[129] = X[2]                                   # another tile
    X[70] = X[2]
    X[5] = X[4]                                     # the same tile
    got, status = _distances(_dev(X), metric, squared=False)
    assert not status.any()
    for i, j in ((129, 2), (70, 2), (129, 70), (5, 4)):
        assert got[i, j] == 0.0 and got[j, i] == 0.0, (metric, i, j, got[i, j])
    assert (got[~np.eye(130, dtype=bool)] > 0).sum() == 130 * 129 - 8


def test_bad_values_are_counted_and_refused():
    X = R.gaussian_rows(70, 12, 1)
    X[3, 5] = np.nan
    X[66, 0] = np.nan
    X[69, 11] = np.inf
    _, status = _distances(_dev(X), "euclidean")
    assert status.tolist() == [3, 0]
    with pytest.raises(ValueError, match=r"^Input X contains NaN\."):
        AgglomerativeClustering(linkage="average").fit(_dev(X))
    X = R.gaussian_rows(70, 13, 1)
    X[69, 12] = -np.inf
    with pytest.raises(ValueError, match=r"^Input X contains infinity or a value too large for dtype\('float32'\)\."):
        AgglomerativeClustering(linkage="single", metric="manhattan").fit(_dev(X))
    X = R.gaussian_rows(70, 8, 1)
    X[68] = 0.0
    _, status = _distances(_dev(X), "cosine")
    assert status.tolist() == [0, 1]
    with pytest.raises(ValueError, match="Cosine affinity cannot be used when X contains zero vectors"):
        AgglomerativeClustering(linkage="average", metric="cosine").fit(_dev(X))
    M = torch.zeros(4, 4, dtype=torch.float64, device="cuda")
    M[1, 2] = M[2, 1] = float("inf")
    with pytest.raises(ValueError, match="Input X contains infinity"):
        AgglomerativeClustering(linkage="average", metric="precomputed").fit(M)


# ------------------------------------------------------------------ the merge loop, from numpy's bits
def _merge(M, linkage, adjacency=None):
    """ops.agglo_merge on the host matrix M (squared for Ward) in exact-size guarded buffers -> (children, heights, status)."""
    from vit_som_amd import ops
    N = M.shape[0]
    ws, hw = MC.guarded((ops.agglo_workspace_bytes(N, adjacency is not None),), torch.uint8, "cuda")
    ops.agglo_matrix(ws, N).copy_(_dev(M))
    if adjacency is not None:
        ops.agglo_adjacency(ws, N).copy_(_dev(adjacency.astype(np.uint8)))
    children, hc = MC.guarded((N - 1, 2), torch.int32, "cuda")
    heights, hh = MC.guarded((N - 1,), torch.float64, "cuda")
    status, hs = MC.guarded((4,), torch.int32, "cuda")
    ops.agglo_merge(ws, N, LINK[linkage], adjacency is not None, children, heights, status)
    torch.cuda.synchronize()
    for h, what in ((hw, "workspace"), (hc, "children"), (hh, "distances"), (hs, "status")):
        h.check(what)
    hc.all_written("children"); hh.all_written("distances"); hs.all_written("status")
    return children.cpu().numpy().astype(np.int64), heights.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("N", MERGE_N)
def test_merge_loop_equals_scipy_from_the_same_matrix(N):
    from scipy.cluster.hierarchy import linkage as scipy_linkage
    from scipy.spatial.distance import squareform
    Dm = R.distance_matrix(R.gaussian_rows(N, 4, 11 * N), "euclidean")
    for linkage in R.LINKAGES:
        Z = scipy_linkage(squareform(Dm, checks=False), linkage)
        M = Dm * Dm if linkage == "ward" else Dm
        children, heights, status = _merge(M, linkage)
        assert status[0] == 0 and status[3] == 0 and 0 <= status[2] <= N - 1 and status[1] >= status[2]
        assert np.array_equal(children, Z[:, :2].astype(np.int64)), linkage
        if linkage in ("single", "complete"):
            assert np.array_equal(heights, Z[:, 2]), linkage
            continue
        err = (np.abs(heights - Z[:, 2]) / Z[:, 2]).max()
        bound = 3 * (N - 1) * 2.0 ** -53
        if linkage == "ward":
            ref = R.linkage_tree(M, linkage)[1]
            ref_err = (np.abs(ref - Z[:, 2]) / Z[:, 2]).max()
            print(f"N={N} ward: device error {err:.3e}, restatement error {ref_err:.3e}, 3 (N - 1) 2^-53 = {bound:.3e}")
            assert np.array_equal(heights, ref), "the restatement's arithmetic is the kernel's"
            bound = max(bound, 4 * ref_err)
        else:
            print(f"N={N} average: device error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (linkage, err, bound)


# ------------------------------------------------------------------ whole fits from rows
def _fit(X, **kw):
    ac = AgglomerativeClustering(**kw).fit(_dev(X))
    assert ac.labels_.is_cuda and ac.labels_.dtype == torch.int64 and ac.n_leaves_ == len(X)
    assert ac.children_.shape == (len(X) - 1, 2) and ac.children_.dtype == np.int64 and ac.distances_.dtype == np.float64
    assert (ac.children_[:, 0] < ac.children_[:, 1]).all() and ac.n_connected_components_ == 1
    return ac


@pytest.mark.parametrize("metric", R.METRICS)
def test_fit_from_rows_equals_scipy(metric):
    from test_agglomerative_cpu import scipy_tree
    N, D = 300, 16
    X = R.gaussian_rows(N, D, N)
    for linkage in R.LINKAGES:
        if linkage == "ward" and metric != "euclidean":
            continue
        Z = scipy_tree(N, D, metric, linkage)
        ac = _fit(X, n_clusters=7, metric=metric, linkage=linkage)
        assert np.array_equal(ac.children_, Z[:, :2].astype(np.int64)), (metric, linkage)
        assert (np.abs(ac.distances_ - Z[:, 2]) / Z[:, 2]).max() < 1e-12
        assert np.array_equal(ac.labels_.cpu().numpy(), R.cut(Z[:, :2].astype(np.int64), N, 7)) and ac.n_clusters_ == 7
        again = _fit(X, n_clusters=7, metric=metric, linkage=linkage)
        assert np.array_equal(again.children_, ac.children_) and again.distances_.tobytes() == ac.distances_.tobytes()
        assert torch.equal(again.labels_, ac.labels_)
    # l2 / l1 are the same metrics, a strided X is taken, fit_predict returns labels_
    wide = torch.zeros(N, D + 3, device="cuda")
    wide[:, :D] = _dev(X)
    alias = {"euclidean": "l2", "manhattan": "l1", "cosine": "cosine"}[metric]
    a = AgglomerativeClustering(5, metric=alias, linkage="average")
    b = _fit(X, n_clusters=5, metric=metric, linkage="average")
    assert torch.equal(a.fit_predict(wide[:, :D]), b.labels_) and a.distances_.tobytes() == b.distances_.tobytes()


def test_distance_threshold_and_precomputed():
    from test_agglomerative_cpu import fixture_matrix, scipy_tree
    N, D = 300, 16
    X = R.gaussian_rows(N, D, N)
    Z = scipy_tree(N, D, "euclidean", "complete")
    for threshold in (0.0, float(Z[N // 2, 2]), float(Z[-1, 2]) * 2):
        ac = _fit(X, n_clusters=None, distance_threshold=threshold, linkage="complete")
        assert ac.n_clusters_ == R.clusters_at_threshold(ac.distances_, threshold) == R.clusters_at_threshold(Z[:, 2], threshold)
        assert int(ac.labels_.max()) + 1 == ac.n_clusters_
    Dm = fixture_matrix(N, D, "euclidean")
    for dtype in (torch.float64, torch.float32):
        given = _dev(Dm, dtype)
        ac = AgglomerativeClustering(4, metric="precomputed", linkage="complete").fit(given)
        if dtype == torch.float64:
            assert np.array_equal(ac.children_, Z[:, :2].astype(np.int64)) and np.array_equal(ac.distances_, Z[:, 2])
        assert ac.n_features_in_ == N and int(ac.labels_.max()) == 3
    with pytest.raises(ValueError, match="Cannot extract more clusters than samples: 5 clusters where given for a tree with 4 leaves."):
        AgglomerativeClustering(5, linkage="single").fit(_dev(X[:4]))
    with pytest.raises(ValueError, match=r"Found array with 1 sample\(s\) \(shape=\(1, 16\)\) while a minimum of 2 is required by AgglomerativeClustering."):
        AgglomerativeClustering().fit(_dev(X[:1]))
    with pytest.raises(ValueError, match="16384"):
        AgglomerativeClustering().fit(torch.zeros(16385, 1, device="cuda"))


def _same_as_restatement(X, metric, linkage, adjacency=None, k=4):
    ward = linkage == "ward"
    want = R.linkage_tree(R.distance_matrix(X, metric, squared=ward), linkage, adjacency)
    ac = _fit(X, n_clusters=k, metric=metric, linkage=linkage, connectivity=None if adjacency is None else _dev(adjacency))
    return ac, want


@pytest.mark.parametrize("linkage", R.LINKAGES)
def test_ties_fall_as_in_the_restatement(linkage):
    lattice = np.array([(i, j) for i in range(8) for j in range(8)], dtype=np.float32)
    same = np.full((65, 5), 3.25, dtype=np.float32)
    for X in (lattice, same):
        for metric in R.METRICS:
            if (linkage == "ward" and metric != "euclidean") or (metric == "cosine" and X is lattice):
                continue                            # the lattice holds the zero vector
            ac, (children, heights, missing) = _same_as_restatement(X, metric, linkage)
            assert missing == 0
            assert np.array_equal(ac.children_, children), (linkage, metric)
            assert ac.distances_.tobytes() == heights.tobytes(), (linkage, metric)
            assert np.array_equal(ac.labels_.cpu().numpy(), R.cut(children, len(X), 4))
    assert not _fit(same, linkage=linkage).distances_.any()


# ------------------------------------------------------------------ connectivity
GRIDS = ((8, 8), (9, 7))


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_connectivity_against_the_restatement_and_sklearn(grid):
    from scipy.sparse import csr_matrix
    from sklearn.cluster import AgglomerativeClustering as SK
    from test_agglomerative_cpu import grid_case
    X, adj, _ = grid_case(*grid)
    K = len(X)
    for linkage in R.LINKAGES:
        ac, (children, heights, missing) = _same_as_restatement(X, "euclidean", linkage, adj, k=5)
        assert missing == 0
        assert np.array_equal(ac.children_, children), linkage
        assert (np.abs(ac.distances_ - heights) / heights).max() < 1e-12
        labels = ac.labels_.cpu().numpy()
        assert np.array_equal(labels, R.cut(children, K, 5))
        for c in range(5):                          # every cluster is one region of the grid
            members = np.nonzero(labels == c)[0]
            reach, frontier = {int(members[0])}, [int(members[0])]
            while frontier:
                u = frontier.pop()
                for v in np.nonzero(adj[u] & (labels == c))[0].tolist():
                    if v not in reach:
                        reach.add(v); frontier.append(v)
            assert len(reach) == len(members), (linkage, c)
    for k in (2, 5, 10):
        want = SK(n_clusters=k, linkage="ward", connectivity=csr_matrix(adj)).fit(X.astype(np.float64)).labels_
        for given in (_dev(adj), adj.astype(np.int64), csr_matrix(adj)):
            got = AgglomerativeClustering(k, connectivity=given).fit(_dev(X))
            assert R.same_partition(got.labels_.cpu().numpy(), want) and got.n_connected_components_ == 1


def test_a_split_graph_is_refused_with_its_count():
    X = R.gaussian_rows(70, 3, 4)
    adj = np.zeros((70, 70), dtype=bool)
    adj[:30, :30] = adj[30:66, 30:66] = adj[66:, 66:] = True
    for linkage in ("ward", "single"):
        with pytest.raises(ValueError, match="the connectivity has 3 connected components"):
            AgglomerativeClustering(2, linkage=linkage, connectivity=_dev(adj)).fit(_dev(X))
    children, heights, status = _merge(R.distance_matrix(X, "euclidean"), "average", adj)
    want = R.linkage_tree(R.distance_matrix(X, "euclidean"), "average", adj)
    assert status[0] == 2 == want[2] and np.array_equal(children, want[0]) and (children[-2:] == -1).all()
    assert np.isnan(heights[-2:]).all() and np.array_equal(heights[:-2], want[1][:-2])


# ------------------------------------------------------------------ the map's clusters
def _map_models():
    import vit_som_amd
    from test_kmeans_gpu import _models
    (vm, cfg), (dm, cfgd) = _models()
    cfgr = copy.deepcopy(cfg)
    cfgr["hyperparameters"]["som"]["use_reduced"] = True
    torch.manual_seed(3)
    rm = vit_som_amd.ViTSOM(copy.deepcopy(cfgr), device="cuda:0")
    return (vm, cfg, "ward"), (rm, cfgr, "ward"), (dm, cfgd, "average")


def test_evaluate_map_clusters_on_the_golden_models():
    from test_kmeans_gpu import _separable_images
    from vit_som_amd.evaluation import nmi_from_table, purity_from_table
    for m, cfg, default_linkage in _map_models():
        d, som = cfg["data"], m.som_layer
        K = som.n_prototypes
        batches = _separable_images(5, 12, 4, d["num_channels"], d["input_size"], 8)
        m.train(True)
        rep = evaluate_map_clusters(m, cfg, batches, n_clusters=4)
        assert m.training and isinstance(rep, MapClustersReport)
        assert rep.linkage == default_linkage and rep.metric == som.distance_fcn and rep.connectivity == "grid"
        assert rep.n_clusters == 4 and rep.n_samples == 48 and rep.inference_time > 0
        assert rep.children.shape == (K - 1, 2) and rep.distances.shape == (K - 1,)
        # unit_labels: the class on the prototypes (a cosine map under Ward: on the prototypes at unit length)
        rows = som.prototypes.detach().float().contiguous()
        fit_metric = som.distance_fcn
        if som.distance_fcn == "cosine":
            rows, fit_metric = torch.nn.functional.normalize(rows, p=2, dim=1), "euclidean"
        adj = som.grid_connectivity()
        ac = AgglomerativeClustering(4, metric=fit_metric, linkage=default_linkage, connectivity=adj).fit(rows)
        assert torch.equal(rep.unit_labels, ac.labels_) and np.array_equal(rep.children, ac.children_)
        assert rep.distances.tobytes() == ac.distances_.tobytes()
        # sample labels are unit_labels[bmu]; purity and NMI are the table's
        m.eval()
        bmus = torch.cat([m.predict(x.cuda())[0].reshape(-1).long().clone() for x, _ in batches])
        ys = torch.cat([y for _, y in batches]).numpy()
        labels = rep.unit_labels[bmus]
        assert torch.equal(rep.sample_labels, labels)
        table = np.zeros((4, 256), dtype=np.int64)
        np.add.at(table, (labels.cpu().numpy(), ys), 1)
        assert rep.purity == purity_from_table(table) and rep.nmi == nmi_from_table(table)
        assert np.array_equal(rep.samples_per_cluster, table.sum(axis=1))
        assert np.array_equal(rep.units_per_cluster, np.bincount(rep.unit_labels.cpu().numpy(), minlength=4))
        # every cluster is one connected region of the grid
        unit = rep.unit_labels.cpu().numpy()
        near = adj.cpu().numpy()
        for c in range(4):
            members = np.nonzero(unit == c)[0]
            reach, frontier = {int(members[0])}, [int(members[0])]
            while frontier:
                u = frontier.pop()
                for v in np.nonzero(near[u] & (unit == c))[0].tolist():
                    if v not in reach:
                        reach.add(v); frontier.append(v)
            assert len(reach) == len(members)
        free = evaluate_map_clusters(m, cfg, batches, n_clusters=3, connectivity=None, linkage="complete")
        assert free.connectivity is None and free.linkage == "complete" and int(free.unit_labels.max()) == 2
        if not d.get("num_classes"):                # a clustering config: the distinct labels of the loader
            assert evaluate_map_clusters(m, cfg, batches).n_clusters == 4
        else:
            assert evaluate_map_clusters(m, cfg, batches).n_clusters == d["num_classes"]
    with pytest.raises(ValueError, match="connectivity must be 'grid' or None"):
        evaluate_map_clusters(m, cfg, batches, connectivity="ring")


def test_visualize_map_clusters(tmp_path):
    from test_kmeans_gpu import _models
    from vit_som_amd.evaluation import visualize_map_clusters
    (m, cfg), _ = _models()
    rows, cols = m.som_layer.map_size
    regions = visualize_map_clusters(m, cfg, n_clusters=3, output_dir=str(tmp_path))
    assert regions.shape == (rows, cols) and sorted(np.unique(regions).tolist()) == [0, 1, 2] and regions[0, 0] == 0


def test_driver_reports_the_map_clusters(tmp_path):
    from vit_som_amd.train import main, synthetic_loaders
    _, cfg = load_golden("ref_cluster_tiny")
    cfg = copy.deepcopy(cfg)
    cfg["hyperparameters"]["batch_size"] = 16
    logs = []
    loaders = lambda c, r, w: synthetic_loaders(c, r, w, n_train=64, n_val=16, n_test=16)      # noqa: E731
    today = {"accuracy", "precision", "recall", "f1", "purity", "nmi", "run_duration", "inference_time"}
    met = main(cfg, n_runs=1, max_epochs=1, make_loaders=loaders, model_states_dir=str(tmp_path / "a"), log=logs.append,
               map_clusters=True)
    assert set(met) == today | {"map_cluster_purity", "map_cluster_nmi"}
    (p,), (n,) = met["map_cluster_purity"], met["map_cluster_nmi"]
    assert 0.0 < p <= 1.0 and 0.0 <= n <= 1.0 + 1e-12
    assert any("Map clusters: purity" in l for l in logs)
