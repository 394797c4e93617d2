"""HDBSCAN without a GPU: (1) the restatement (hdbscan_ref) agrees with itself -- Kruskal and Prim build the same tree under
(w, lo, hi); (2) the product's host tree code (vit_som_amd.hdbscan.tree_to_labels), fed the spanning tree of sklearn's own
fp64 distances, gives sklearn's noise set, partition and probabilities and the naive restatement's labels exactly; (3) the
surface: sklearn's parameter error sentences, the departures with their reason, host tensors refused before the library is
called, the new entries declared, exported and refusing on the host."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import hdbscan_ref as R
import ops_arguments as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("vsom_hdbscan_init", "vsom_hdbscan_nearest", "vsom_hdbscan_nearest_matrix", "vsom_hdbscan_merge")
_CACHE = {}


def _tree(N, D, offset, min_samples, centers=3):
    """(X, the spanning tree of the fp64 mutual reachability of sklearn's own distances) of a fixture, computed once."""
    key = (N, D, offset, min_samples, centers)
    if key not in _CACHE:
        X = R.blobs(N, D, offset, centers)
        W, _ = R.mutual_reachability(R.distances64(X, R.EUCLIDEAN), min_samples)
        _CACHE[key] = (X, R.prim(W))
    return _CACHE[key]


def _sklearn(X, mcs, ms, **kw):
    from sklearn.cluster import HDBSCAN
    return HDBSCAN(min_cluster_size=mcs, min_samples=ms, algorithm="brute", **kw).fit(X.astype(np.float64))


# ------------------------------------------------------------------ (1) the restatement
@pytest.mark.parametrize("N,D", [(130, 3), (333, 1003)])
def test_kruskal_and_prim_build_the_same_tree(N, D):
    """The order is strict, so the tree is unique: two algorithms, one edge list.  On integer distances ties abound."""
    X = R.blobs(N, D)
    for W in (R.mutual_reachability(R.distances64(X, R.EUCLIDEAN), 5)[0],
              R.mutual_reachability(np.round(R.distances64(X[:, :3], R.EUCLIDEAN)), 3)[0]):
        a, b = R.kruskal(W), R.prim(W)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        assert R.is_spanning_tree(a[0], a[1], N) and (a[0] < a[1]).all()
        assert np.array_equal(np.lexsort((a[1], a[0], a[2])), np.arange(N - 1))
        from scipy.sparse.csgraph import minimum_spanning_tree
        ref = np.sort(minimum_spanning_tree(np.triu(W + 1.0, 1)).data - 1.0)          # + 1: scipy reads a zero as no edge
        assert np.allclose(np.sort(a[2]), ref, rtol=0, atol=1e-12)
    assert not R.is_spanning_tree([0, 1, 0], [1, 2, 2], 4)


def test_core_distances_count_the_row_itself():
    D = np.array([[0.0, 1.0, 4.0], [1.0, 0.0, 2.0], [4.0, 2.0, 0.0]])
    assert R.core_distances(D, 1).tolist() == [0.0, 0.0, 0.0] and R.core_distances(D, 2).tolist() == [1.0, 1.0, 2.0]
    W, core = R.mutual_reachability(D, 2)
    assert W[0, 1] == 1.0 and W[1, 2] == 2.0 and W[0, 2] == 4.0


# ------------------------------------------------------------------ (2) the product's tree code against sklearn
@pytest.mark.parametrize("mcs,ms", R.PARAMS)
@pytest.mark.parametrize("offset", R.OFFSETS)
@pytest.mark.parametrize("N,D", R.SHAPES)
def test_tree_code_gives_sklearns_clusters(N, D, offset, mcs, ms):
    """The same noise set and adjusted Rand index 1.0 against sklearn.cluster.HDBSCAN(algorithm="brute"), probabilities_
    to 1e-9, dbscan_clustering at three cut distances equal up to renumbering; and the naive restatement's labels exactly.
    "leaf" and allow_single_cluster: test_leaf_and_single_cluster."""
    from vit_som_amd import hdbscan as H
    X, (lo, hi, w) = _tree(N, D, offset, ms or mcs)
    out = H.tree_to_labels(lo, hi, w, N, mcs)
    sk = _sklearn(X, mcs, ms)
    labels = out["labels"]
    assert np.array_equal(labels < 0, sk.labels_ < 0) and R.rand_index_is_one(sk.labels_, labels)
    assert np.abs(out["probabilities"] - sk.probabilities_).max() <= 1e-9
    assert labels.max() + 1 == len(out["clusters"]) == len(out["persistence"]) >= 2 and (labels < 0).any()
    first = [int(np.flatnonzero(labels == c)[0]) for c in range(labels.max() + 1)]
    assert first == sorted(first)                                                     # numbered by smallest row
    naive = R.naive_hdbscan(lo, hi, w, N, mcs)
    assert np.array_equal(naive[0], labels) and np.abs(naive[1] - out["probabilities"]).max() <= 1e-12
    assert np.allclose(naive[2], out["persistence"], rtol=1e-12)
    assert np.allclose(np.sort(sk._single_linkage_tree_["value"]), w, rtol=0, atol=1e-12)
    assert np.array_equal(out["single_linkage_tree"][:, 2], w) and out["single_linkage_tree"][-1, 3] == N
    for q in (0.5, 0.9, 0.98):
        cut = float(0.5 * (w[int(q * (N - 2))] + w[int(q * (N - 2)) + 1]))
        mine = H.labels_at_cut(lo, hi, w, N, cut, mcs)
        assert R.same_partition(mine, sk.dbscan_clustering(cut, min_cluster_size=mcs))
        if N <= 333:
            assert np.array_equal(mine, R.naive_cut(lo, hi, w, N, cut, mcs))


def _sk_linkage(sk):
    t = sk._single_linkage_tree_
    return np.stack([t["left_node"], t["right_node"], t["value"], t["cluster_size"]], axis=1).astype(np.float64)


@pytest.mark.parametrize("centers", [1, 3])
@pytest.mark.parametrize("N,D", R.SHAPES)
def test_leaf_and_single_cluster(N, D, centers):
    """cluster_selection_method "eom" / "leaf", with and without allow_single_cluster, on one blob and on three: the
    product's tree of sklearn's fp64 distances (the order (w, lo, hi)) gives sklearn's noise set and adjusted Rand index 1.0,
    and the naive restatement's labels exactly.  The one exception is pinned: at (130, 3) the tree has exactly tied
    weights, which of two tied edges merges first is sklearn's traversal order and not a property of the data, and one point
    of 130 between two neighbouring clusters lands on the other side (one blob, eom; three blobs, leaf): there the noise
    set is equal and at most one label differs.  In addition, given sklearn's OWN single-linkage tree the product's
    condense / select / label code reproduces sklearn's partition and probabilities exactly, on every shape."""
    from vit_som_amd import hdbscan as H
    mcs = 12
    X, (lo, hi, w) = _tree(N, D, 0.0, 4, centers=centers)
    for method in ("eom", "leaf"):
        for single in (False, True):
            sk = _sklearn(X, mcs, 4, cluster_selection_method=method, allow_single_cluster=single)
            out = H.tree_to_labels(lo, hi, w, N, mcs, method, single)
            what = f"({N}, {D}) {centers} blobs {method} single={single}: {out['labels'].max() + 1} clusters, {(out['labels'] < 0).sum()} noise"
            differ = R.labels_that_differ(sk.labels_, out["labels"])
            print(what, f"{differ} labels differ from sklearn's")
            assert np.array_equal(out["labels"] < 0, sk.labels_ < 0), what
            if (N, D) == (130, 3):
                assert differ <= 1, what
            else:
                assert differ == 0 and R.rand_index_is_one(sk.labels_, out["labels"]), what
                assert np.abs(out["probabilities"] - sk.probabilities_).max() <= 1e-9, what
            naive = R.naive_hdbscan(lo, hi, w, N, mcs, method, single)
            assert np.array_equal(naive[0], out["labels"]) and np.abs(naive[1] - out["probabilities"]).max() <= 1e-12, what
            own = H.linkage_to_labels(_sk_linkage(sk), mcs, method, single)
            assert np.array_equal(own["labels"] < 0, sk.labels_ < 0) and R.same_partition(sk.labels_, own["labels"]), what
            assert R.rand_index_is_one(sk.labels_, own["labels"]), what
            assert np.abs(own["probabilities"] - sk.probabilities_).max() <= 1e-9, what
    if centers == 1:
        out = H.tree_to_labels(lo, hi, w, N, mcs, "eom", True)
        assert out["labels"].max() == 0 and (out["labels"] == 0).sum() >= mcs         # one cluster, of at least min_cluster_size rows


@pytest.mark.parametrize("eps", [0.5, 3.0, 40.0])
def test_cluster_selection_epsilon(eps):
    from vit_som_amd import hdbscan as H
    N, D, mcs = 130, 3, 5
    X, (lo, hi, w) = _tree(N, D, 0.0, mcs)
    for method in ("eom", "leaf"):
        for single in (False, True):
            out = H.tree_to_labels(lo, hi, w, N, mcs, method, single, eps)
            sk = _sklearn(X, mcs, None, cluster_selection_method=method, allow_single_cluster=single, cluster_selection_epsilon=eps)
            assert R.same_partition(out["labels"], sk.labels_), (method, single)
            assert np.abs(out["probabilities"] - sk.probabilities_).max() <= 1e-9
            naive = R.naive_hdbscan(lo, hi, w, N, mcs, method, single, eps)
            assert np.array_equal(naive[0], out["labels"])


def test_duplicates_give_infinite_lambda_and_probability_one():
    """Zero distances: lambda is infinite where sklearn's is, and the probabilities are sklearn's."""
    from vit_som_amd import hdbscan as H
    rng = np.random.default_rng(3)
    X = np.repeat(rng.integers(0, 6, (30, 4)), 4, axis=0).astype(np.float32)
    N = X.shape[0]
    W, _ = R.mutual_reachability(R.distances64(X, R.EUCLIDEAN), 3)
    lo, hi, w = R.kruskal(W)
    assert (w == 0).sum() >= 60
    out = H.tree_to_labels(lo, hi, w, N, 3)
    assert np.isinf(out["condensed_tree"]["value"]).any()
    naive = R.naive_hdbscan(lo, hi, w, N, 3)
    assert np.array_equal(naive[0], out["labels"]) and np.array_equal(naive[1], out["probabilities"])
    assert out["labels"].max() >= 1 and (out["probabilities"][out["labels"] >= 0] == 1.0).any()


def test_condensed_tree_and_layout():
    from vit_som_amd import hdbscan as H
    X, (lo, hi, w) = _tree(130, 3, 0.0, 5)
    Z = H.single_linkage(lo, hi, w)
    order, start = H.leaf_layout(Z)
    assert sorted(order.tolist()) == list(range(130))
    for k in (0, 57, 128):                                             # a node's leaves are a slice
        todo, leaves = [130 + k], []
        while todo:
            v = todo.pop()
            if v < 130:
                leaves.append(v)
            else:
                todo += [int(Z[v - 130, 0]), int(Z[v - 130, 1])]
        assert sorted(order[start[130 + k]:start[130 + k] + int(Z[k, 3])].tolist()) == sorted(leaves)
    tree = H.condense_tree(Z, 5)
    assert tree.dtype == H.CONDENSED_DTYPE and tree["parent"].min() == 130
    points = tree[tree["cluster_size"] == 1]
    assert sorted(points["child"].tolist()) == list(range(130))       # every sample leaves the tree exactly once
    assert (tree["child"][tree["cluster_size"] > 1] > tree["parent"][tree["cluster_size"] > 1]).all()
    with pytest.raises(ValueError, match="cycle"):
        H.single_linkage(np.array([0, 0, 1]), np.array([1, 2, 2]), np.array([1.0, 2.0, 3.0]))


# ------------------------------------------------------------------ (3) surface and refusals
def _message(fn):
    with pytest.raises(ValueError) as err:
        fn()
    return str(err.value)


def _sk_message(**kw):
    from sklearn.cluster import HDBSCAN
    with pytest.raises(ValueError) as err:
        HDBSCAN(**kw).fit(np.zeros((8, 2)))
    return str(err.value)


def _set_free(msg):
    """sklearn prints the options of a str parameter as a set, in no fixed order: compare them as a set."""
    m = re.search(r"\{(.*?)\}", msg)
    return (msg[:m.start()], frozenset(m.group(1).split(", ")), msg[m.end():]) if m else (msg, None, "")


@pytest.mark.parametrize("kw", [dict(min_cluster_size=1), dict(min_cluster_size=2.5), dict(min_cluster_size=True), dict(min_samples=0),
                                dict(min_samples=1.5), dict(cluster_selection_epsilon=-1), dict(cluster_selection_epsilon="a"),
                                dict(max_cluster_size=0), dict(max_cluster_size=1.5), dict(metric="nope"), dict(metric=3),
                                dict(metric_params=3), dict(alpha=0), dict(alpha=-1.0), dict(alpha="a"), dict(alpha=float("inf")),
                                dict(algorithm="fast"), dict(algorithm=None), dict(leaf_size=0), dict(n_jobs=1.5),
                                dict(cluster_selection_method="x"), dict(allow_single_cluster=1), dict(allow_single_cluster="a"),
                                dict(store_centers="x"), dict(copy=1), dict(copy="a")], ids=repr)
def test_parameter_error_sentences_are_sklearns(kw):
    from vit_som_amd import HDBSCAN
    ours = _message(lambda: HDBSCAN(**kw).fit(torch.zeros(8, 2)))      # refused before the tensor is looked at
    assert _set_free(ours) == _set_free(_sk_message(**kw))


def test_signature_and_defaults_are_sklearns():
    import sklearn.cluster
    from vit_som_amd import HDBSCAN
    ours, theirs = inspect.signature(HDBSCAN.__init__), inspect.signature(sklearn.cluster.HDBSCAN.__init__)
    assert str(ours) == str(theirs)
    assert list(inspect.signature(HDBSCAN.fit).parameters)[:3] == ["self", "X", "y"]
    assert str(inspect.signature(HDBSCAN.dbscan_clustering)) == str(inspect.signature(sklearn.cluster.HDBSCAN.dbscan_clustering))


def test_the_departures_raise_with_their_reason():
    from vit_som_amd import HDBSCAN
    from vit_som_amd import hdbscan as M
    x = torch.zeros(8, 2)
    for metric in ("manhattan", "l1", "minkowski", "chebyshev"):                  # sklearn's names this class does not compute
        msg = _message(lambda: HDBSCAN(metric=metric).fit(x))
        assert "not supported" in msg and "precomputed" in msg
    msg = _message(lambda: HDBSCAN(metric=lambda a, b: 0.0).fit(x))              # a callable: sklearn takes it
    assert "callable metric is not supported" in msg and "precomputed" in msg
    assert "not supported" in _message(lambda: HDBSCAN(metric_params={"p": 3}).fit(x))
    msg = _message(lambda: HDBSCAN(min_samples=65).fit(x))
    assert "not supported" in msg and "64" in msg and "neighbour" in msg
    msg = _message(lambda: HDBSCAN(alpha=0.5).fit(x))
    assert "alpha" in msg and "not supported" in msg and "1.0" in msg
    msg = _message(lambda: HDBSCAN(max_cluster_size=50).fit(x))
    assert "max_cluster_size" in msg and "not supported" in msg
    for centers in ("centroid", "medoid", "both"):
        msg = _message(lambda: HDBSCAN(store_centers=centers).fit(x))
        assert "store_centers" in msg and "not supported" in msg
    HDBSCAN(algorithm="kd_tree", leaf_size=7, n_jobs=3, copy=True, metric_params={}, min_samples=64)._check_params()   # validated, ignored
    assert "on the GPU" in _message(lambda: HDBSCAN().fit(x))
    assert "on the GPU" in _message(lambda: HDBSCAN().fit(np.zeros((8, 2))))
    assert M.MAX_SAMPLES == 131072 and M.MAX_MIN_SAMPLES == 64
    assert M.default_min_cluster_size(10000, 10) == 50 and M.default_min_cluster_size(300, 10) == 5
    doc = M.HDBSCAN.__doc__ + M.__doc__
    for word in ("fp32", "exact ties", "traversal order", "min_samples <= 64", "alpha", "max_cluster_size", "store_centers", "algorithm",
                 "leaf_size", "n_jobs", "copy", "callable", "131 072", "precomputed", "smallest row", "float32 rounding"):
        assert word in doc, word
    for name in ("INTEGRATION.md", "DESIGN.md"):
        text = " ".join(open(os.path.join(ROOT, name)).read().split())
        for word in ("HDBSCAN", "fp32", "exact ties", "traversal order", "(w, min(i, j), max(i, j))"):
            assert word in text, (name, word)


def _stub_rows():
    z = lambda dtype, *shape: torch.zeros(*shape, dtype=dtype)                   # noqa: E731
    N = 70
    comp, edges, record, best = z(A.I32, N), z(A.I32, N, 3), z(A.I32, 4), z(A.I64, N)
    core = z(A.F32, N)
    return {
        "hdbscan_init": dict(comp=comp, edges=edges, record=record),
        "hdbscan_nearest": dict(X=z(A.F32, N, 5), metric=1, core=core, comp=comp, sq=z(A.F32, N), best=best, record=record),
        "hdbscan_nearest_matrix": dict(M=z(A.F32, N, N), core=core, comp=comp, best=best, record=record),
        "hdbscan_nearest_matrix[f64]": dict(M=z(A.F64, N, N), core=core, comp=comp, best=best, record=record),
        "hdbscan_merge": dict(best=best, comp=comp, edges=edges, work=z(A.I64, 2 * N), record=record),
    }


@pytest.mark.parametrize("name", sorted(_stub_rows()))
def test_host_tensors_are_refused_before_the_library(monkeypatch, name):
    from vit_som_amd import ops
    stub = A.StubLib()
    monkeypatch.setattr(ops, "lib", stub)
    with pytest.raises(ValueError, match="expected a HIP device tensor"):
        getattr(ops, name.split("[")[0])(**_stub_rows()[name])
    assert stub.calls == []
    assert ops.hdbscan_work(70) == 140 and ops.HDBSCAN_MAX_N == ops.DBSCAN_MAX_N == 131072


def test_every_new_entry_is_declared_exported_and_refuses_on_the_host():
    from test_abi import header_functions
    from vit_som_amd._lib import LIB_PATH, SIGNATURES, last_error, lib
    raw = ctypes.CDLL(LIB_PATH)
    for name in ENTRIES:
        assert name in header_functions() and name in SIGNATURES and hasattr(raw, name), name
    P = 4096                                                         # never dereferenced: every call below is refused first
    assert lib.vsom_hdbscan_init(10, None, P, P, None) == -1 and "null" in last_error()
    assert lib.vsom_hdbscan_init(1, P, P, P, None) == -1                                         # N < 2
    assert lib.vsom_hdbscan_init(131073, P, P, P, None) == -3
    assert lib.vsom_hdbscan_nearest(None, 8, 10, 8, 1, P, P, P, P, P, None) == -1 and "null" in last_error()
    assert lib.vsom_hdbscan_nearest(P, 8, 10, 8, 1, P, P, P, None, P, None) == -1
    assert lib.vsom_hdbscan_nearest(P, 8, 1, 8, 1, P, P, P, P, P, None) == -1                    # N < 2
    assert lib.vsom_hdbscan_nearest(P, 4, 10, 8, 1, P, P, P, P, P, None) == -1                   # ldx < D
    assert lib.vsom_hdbscan_nearest(P, 8, 10, 0, 1, P, P, P, P, P, None) == -1                   # D < 1
    assert lib.vsom_hdbscan_nearest(P, 8, 131073, 8, 1, P, P, P, P, P, None) == -3 and "131072" in last_error()
    assert lib.vsom_hdbscan_nearest(P, 8, 10, 8, 7, P, P, P, P, P, None) == -3 and "metric" in last_error()
    assert lib.vsom_hdbscan_nearest_matrix(None, 10, 10, 0, P, P, P, P, None) == -1
    assert lib.vsom_hdbscan_nearest_matrix(P, 9, 10, 0, P, P, P, P, None) == -1                  # ldm < N
    assert lib.vsom_hdbscan_nearest_matrix(P, 131073, 131073, 1, P, P, P, P, None) == -3
    assert lib.vsom_hdbscan_merge(P, 10, P, P, None, P, None) == -1 and "null" in last_error()
    assert lib.vsom_hdbscan_merge(P, 1, P, P, P, P, None) == -1
    assert lib.vsom_hdbscan_merge(P, 131073, P, P, P, P, None) == -3
    header = " ".join(open(os.path.join(ROOT, "include", "vitsom_hip.h")).read().replace("\n *", " ").split())
    for word in ("(w, lo, hi)", "(fp32 bits of w) << 32 | j", "Integer atomics only", "no grid-wide barrier", "ceil(log2 N)",
                 "16 bytes per lane", "natural alignment", "the fp32 rounding of the maximum"):
        assert word in header, word


def test_package_exports_and_driver_flag():
    import vit_som_amd
    from vit_som_amd import evaluation, hdbscan, train
    for name in ("HDBSCAN", "HDBSCANReport", "evaluate_hdbscan", "visualize_hdbscan"):
        assert getattr(vit_som_amd, name) is getattr(hdbscan, name), name
    assert evaluation.evaluate_hdbscan is hdbscan.evaluate_hdbscan and evaluation.visualize_hdbscan is hdbscan.visualize_hdbscan
    assert evaluation.HDBSCANReport is hdbscan.HDBSCANReport
    assert str(inspect.signature(hdbscan.evaluate_hdbscan)) == \
        "(model, config, dataloader, min_cluster_size=None, min_samples=None, metric=None, space='latent')"
    assert [f for f in hdbscan.HDBSCANReport.__dataclass_fields__] == [
        "min_cluster_size", "min_samples", "metric", "space", "n_clusters", "n_noise", "coverage", "cluster_sizes",
        "cluster_persistence", "mean_probability", "purity", "nmi", "noise_per_class", "n_rounds", "labels", "probabilities",
        "n_samples", "fit_time", "inference_time"]
    assert inspect.signature(train.main).parameters["hdbscan_eval"].default is False
    assert train._parser().parse_args(["--config", "c"]).hdbscan_eval is False
    assert train._parser().parse_args(["--config", "c", "--hdbscan-eval"]).hdbscan_eval is True
