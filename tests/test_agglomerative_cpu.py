"""Agglomerative clustering without a GPU: the restatement (agglomerative_ref.py) against scipy and sklearn, the host cut, the
entries' argument checks, SOMLayer.grid_connectivity and the estimator's error sentences."""
import copy
import functools

import numpy as np
import pytest
import torch

import agglomerative_ref as R
from helpers import load_golden
from vit_som_amd.agglomerative import AgglomerativeClustering, cut_tree

FIXTURES = ((300, 16), (257, 130), (600, 8))
GRIDS = ((8, 8), (9, 7))


@functools.lru_cache(maxsize=None)
def fixture_matrix(N, D, metric):
    return R.distance_matrix(R.gaussian_rows(N, D, N), metric)


@functools.lru_cache(maxsize=None)
def scipy_tree(N, D, metric, linkage):
    from scipy.cluster.hierarchy import linkage as scipy_linkage
    from scipy.spatial.distance import squareform
    return scipy_linkage(squareform(fixture_matrix(N, D, metric), checks=False), linkage)


# ------------------------------------------------------------------ the restatement against scipy
@pytest.mark.parametrize("linkage", R.LINKAGES)
@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("shape", FIXTURES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_equals_scipy(shape, metric, linkage):
    Z = scipy_tree(*shape, metric, linkage)
    gaps = np.diff(Z[:, 2]) / Z[1:, 2]
    assert gaps.min() > 1e-10, f"the fixture has merge heights closer than 1e-10 relative ({gaps.min():.3e}): scipy's order is not defined"
    Dm = fixture_matrix(*shape, metric)
    children, heights, missing = R.linkage_tree(Dm * Dm if linkage == "ward" else Dm, linkage)
    assert missing == 0
    assert np.array_equal(children, Z[:, :2].astype(np.int64))
    rel = np.abs(heights - Z[:, 2]) / Z[:, 2]
    assert rel.max() <= 1e-14, rel.max()


def test_direct_form_is_symmetric_and_exact_on_duplicates():
    X = R.gaussian_rows(40, 7, 1)
    X[5] = X[17]
    for metric in R.METRICS:
        Dm = R.distance_matrix(X, metric)
        assert np.array_equal(Dm, Dm.T) and not Dm.diagonal().any() and Dm[5, 17] == 0.0


# ------------------------------------------------------------------ connectivity: Ward against sklearn
@functools.lru_cache(maxsize=None)
def grid_case(rows, cols):
    X = R.gaussian_rows(rows * cols, 6, 100 + rows)
    adj = R.grid_adjacency(rows, cols)
    Dsq = R.distance_matrix(X, "euclidean", squared=True)
    return X, adj, R.linkage_tree(Dsq, "ward", adj)


@pytest.mark.parametrize("k", (2, 5, 10))
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_constrained_ward_gives_sklearns_partition(grid, k):
    from scipy.sparse import csr_matrix
    from sklearn.cluster import AgglomerativeClustering as SK
    X, adj, (children, _, missing) = grid_case(*grid)
    assert missing == 0
    want = SK(n_clusters=k, linkage="ward", connectivity=csr_matrix(adj)).fit(X.astype(np.float64)).labels_
    assert R.same_partition(R.cut(children, len(X), k), want)


def test_restatement_counts_the_components_of_a_split_graph():
    X = R.gaussian_rows(12, 3, 4)
    adj = np.zeros((12, 12), dtype=bool)
    adj[:6, :6] = adj[6:, 6:] = True
    children, heights, missing = R.linkage_tree(R.distance_matrix(X, "euclidean"), "average", adj)
    assert missing == 1 and (children[-1] == -1).all() and np.isnan(heights[-1]) and np.isfinite(heights[:-1]).all()


# ------------------------------------------------------------------ the host cut and the threshold formula
@pytest.mark.parametrize("linkage", R.LINKAGES)
def test_the_cut_and_the_threshold_formula_against_sklearn(linkage):
    from sklearn.cluster import AgglomerativeClustering as SK
    N, D = FIXTURES[0]
    X = R.gaussian_rows(N, D, N).astype(np.float64)
    Z = scipy_tree(N, D, "euclidean", linkage)
    children = Z[:, :2].astype(np.int64)
    for k in (1, 2, 7, 50, N):
        labels = cut_tree(children, N, k)
        assert np.array_equal(labels, R.cut(children, N, k)) and labels.dtype == np.int64
        assert R.same_partition(labels, SK(n_clusters=k, linkage=linkage).fit(X).labels_)
        first = [int(np.nonzero(labels == c)[0][0]) for c in range(k)]
        assert first == sorted(first) and first[0] == 0, "clusters are numbered by their smallest row, ascending"
    with pytest.raises(ValueError, match="Cannot extract more clusters than samples: 301 clusters where given for a tree with 300 leaves."):
        cut_tree(children, N, N + 1)
    for threshold in (0.0, float(Z[N // 2, 2]), float(Z[-3, 2]), float(Z[-1, 2]) * 2):
        sk = SK(n_clusters=None, distance_threshold=threshold, linkage=linkage).fit(X)
        k = R.clusters_at_threshold(Z[:, 2], threshold)
        assert k == sk.n_clusters_
        assert R.same_partition(cut_tree(children, N, k), sk.labels_)


# ------------------------------------------------------------------ the entries' host-side checks
P = 4096                    # stands for a non-null, aligned device pointer: nothing is launched, nothing dereferenced


def _align(n):
    return (n + 255) // 256 * 256


def test_workspace_arithmetic():
    from vit_som_amd import ops
    from vit_som_amd._lib import lib
    for N in (2, 3, 65, 1600, 16384):
        slots = 5 * _align(4 * N) + _align(8 * N) + 256
        assert lib.vsom_agglo_workspace_bytes(N, 0) == _align(8 * N * N) + slots
        assert lib.vsom_agglo_workspace_bytes(N, 1) == _align(8 * N * N) + _align(N * N) + slots
        assert ops.agglo_workspace_bytes(N, True) == lib.vsom_agglo_workspace_bytes(N, 1)
    assert lib.vsom_agglo_workspace_bytes(0, 0) == 0 and lib.vsom_agglo_workspace_bytes(-3, 1) == 0
    assert lib.vsom_agglo_workspace_bytes(16385, 0) == 0
    assert ops.AGGLO_MAX_N == 16384
    # the views ops hands out sit where the entry looks for them
    ws = torch.zeros(lib.vsom_agglo_workspace_bytes(5, 1), dtype=torch.uint8)
    assert ws.numel() == _align(200) + _align(25) + 5 * 256 + 256 + 256


def test_argument_refusals_without_a_launch():
    from vit_som_amd._lib import last_error, lib
    need = lib.vsom_agglo_workspace_bytes(70, 1)
    # distances
    assert lib.vsom_agglo_distances(None, 8, 70, 8, 0, 0, P, 70, P, None) == -1 and "null" in last_error()
    assert lib.vsom_agglo_distances(P, 8, 70, 8, 0, 0, None, 70, P, None) == -1
    assert lib.vsom_agglo_distances(P, 8, 70, 8, 0, 0, P, 70, None, None) == -1
    assert lib.vsom_agglo_distances(P, 8, 0, 8, 0, 0, P, 70, P, None) == -1 and "N=0" in last_error()
    assert lib.vsom_agglo_distances(P, 8, 70, 0, 0, 0, P, 70, P, None) == -1
    assert lib.vsom_agglo_distances(P, 7, 70, 8, 0, 0, P, 70, P, None) == -1          # ldx < D
    assert lib.vsom_agglo_distances(P, 8, 70, 8, 0, 0, P, 69, P, None) == -1          # ldo < N
    assert lib.vsom_agglo_distances(P, 8, 16385, 8, 0, 0, P, 16385, P, None) == -3 and "16384" in last_error()
    assert lib.vsom_agglo_distances(P, 8, 70, 8, 3, 0, P, 70, P, None) == -3 and "metric" in last_error()
    # merge
    assert lib.vsom_agglo_merge(P, need, 70, 0, 1, None, P, P, None) == -1 and "null" in last_error()
    assert lib.vsom_agglo_merge(P, need, 70, 0, 1, P, None, P, None) == -1
    assert lib.vsom_agglo_merge(P, need, 70, 0, 1, P, P, None, None) == -1
    assert lib.vsom_agglo_merge(P, need, 0, 0, 1, P, P, P, None) == -1 and "N=0" in last_error()
    assert lib.vsom_agglo_merge(P, need, 1, 0, 1, P, P, P, None) == -1
    assert lib.vsom_agglo_merge(P, 1 << 40, 16385, 0, 0, P, P, P, None) == -3 and "16384" in last_error()
    assert lib.vsom_agglo_merge(P, need, 70, 4, 1, P, P, P, None) == -3 and "linkage" in last_error()
    assert lib.vsom_agglo_merge(P, need - 1, 70, 0, 1, P, P, P, None) == -4
    assert "too small" in last_error() and str(need) in last_error()
    assert lib.vsom_agglo_merge(None, 1 << 40, 70, 0, 1, P, P, P, None) == -4
    assert lib.vsom_agglo_merge(P, lib.vsom_agglo_workspace_bytes(70, 0) , 70, 0, 1, P, P, P, None) == -4   # sized without the adjacency
    assert lib.vsom_agglo_merge(P + 4, 1 << 40, 70, 0, 1, P, P, P, None) == -2


class _Stub:
    """Stands for the library: a call that got past the wrappers' checks would show here."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append(name)
            return 0
        return entry


def test_the_wrappers_refuse_host_tensors_before_the_library(monkeypatch):
    from vit_som_amd import ops
    stub = _Stub()
    monkeypatch.setattr(ops, "lib", stub)
    N, D = 7, 5
    X, out = torch.zeros(N, D), torch.zeros(N, N, dtype=torch.float64)
    st2, st4 = torch.zeros(2, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    ws = torch.zeros(4096, dtype=torch.uint8)
    ch, di = torch.zeros(N - 1, 2, dtype=torch.int32), torch.zeros(N - 1, dtype=torch.float64)
    for call in (lambda: ops.agglo_distances(X, ops.AGGLO_EUCLIDEAN, True, out, st2),
                 lambda: ops.agglo_merge(ws, N, ops.AGGLO_WARD, False, ch, di, st4),
                 lambda: ops.agglo_matrix(ws, N), lambda: ops.agglo_adjacency(ws, N)):
        with pytest.raises(ValueError, match="expected a HIP device tensor"):
            call()
    with pytest.raises(ValueError, match="expected a tensor"):
        ops.agglo_distances(None, ops.AGGLO_EUCLIDEAN, True, out, st2)
    assert stub.calls == []


# ------------------------------------------------------------------ the grid's adjacency
@pytest.mark.parametrize("topology,degree", (("square", 8), ("hexa", 6)))
def test_grid_connectivity(topology, degree):
    from vit_som_amd.som import SOMLayer
    _, cfg = load_golden("ref_cluster_tiny")
    cfg = copy.deepcopy(cfg)
    rows, cols = 5, 6
    cfg["hyperparameters"]["som"].update(map_size=[rows, cols], topology=topology)
    som = SOMLayer(cfg)
    adj = som.grid_connectivity()
    assert adj.dtype == torch.bool and tuple(adj.shape) == (rows * cols, rows * cols)
    assert torch.equal(adj, adj.t()) and not bool(adj.diagonal().any())
    deg = adj.sum(dim=1).view(rows, cols)
    assert bool((deg[1:-1, 1:-1] == degree).all()) and int(deg.max()) == degree
    assert int(deg[0, 0]) == (3 if topology == "square" else 2)
    if topology == "square":
        assert np.array_equal(adj.numpy(), R.grid_adjacency(rows, cols))
    # one component: the restatement merges it down to one cluster
    assert R.linkage_tree(R.distance_matrix(R.gaussian_rows(rows * cols, 3, 2), "euclidean"), "single", adj.numpy())[2] == 0


# ------------------------------------------------------------------ sklearn's sentences
def _sentence(make, fit):
    with pytest.raises(ValueError) as err:
        fit(make())
    return str(err.value)


def _outside_the_options(message):
    """A parameter sentence without its set of options, whose order sklearn does not fix."""
    head, _, rest = message.partition("{")
    return head, rest.partition("}")[2]


@pytest.mark.parametrize("params,set_valued", (
    (dict(n_clusters=0), False), (dict(n_clusters=2.5), False), (dict(linkage="centroid"), True),
    (dict(n_clusters=None, distance_threshold=-1.0), False), (dict(compute_distances="yes"), False),
    (dict(n_clusters=2, distance_threshold=1.0), False), (dict(n_clusters=None), False),
    (dict(n_clusters=None, distance_threshold=1.0, compute_full_tree=False), False),
    (dict(linkage="ward", metric="manhattan"), False), (dict(linkage="ward", metric="cosine"), False),
    (dict(linkage="ward", metric="precomputed"), False)))
def test_error_sentences_are_sklearns(params, set_valued, monkeypatch):
    from sklearn.cluster import AgglomerativeClustering as SK
    X = R.gaussian_rows(6, 6, 0).astype(np.float64)
    theirs = _sentence(lambda: SK(**params), lambda m: m.fit(X))
    monkeypatch.setattr(AgglomerativeClustering, "_check_x", lambda self, X: X)       # no device here: the rules come first or next
    ours = _sentence(lambda: AgglomerativeClustering(**params), lambda m: m.fit(torch.zeros(6, 6)))
    if set_valued:
        assert _outside_the_options(ours) == _outside_the_options(theirs)
    else:
        assert ours == theirs


def test_own_refusals():
    with pytest.raises(ValueError, match="The 'metric' parameter of AgglomerativeClustering must be a str among .*Got 'chebyshev' instead"):
        AgglomerativeClustering(metric="chebyshev").fit(torch.zeros(4, 4))
    with pytest.raises(ValueError, match="must be a tensor on the GPU"):
        AgglomerativeClustering().fit(torch.zeros(4, 4))
