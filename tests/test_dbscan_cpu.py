"""DBSCAN without a GPU: (1) the labelling rule of the device (dbscan_ref.labels_from_adjacency) gives sklearn's labels and core
indices, label for label, on every fixture the GPU tests use; (2) the surface: sklearn's parameter error sentences, the
departures with their reason, host tensors refused before the library is called, the new entries exported."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import dbscan_ref as R
import ops_arguments as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(257, 12288), (333, 1003), (130, 3), (700, 64)]
CASES = [(R.EUCLIDEAN, 0.0), (R.EUCLIDEAN, 0.05), (R.COSINE, 0.05), (R.COSINE, 0.10)]
ENTRIES = ("vsom_dbscan_neighbours", "vsom_dbscan_threshold", "vsom_dbscan_init", "vsom_dbscan_round", "vsom_dbscan_finish")


def _sklearn(D64, eps, min_samples):
    from sklearn.cluster import DBSCAN
    sk = DBSCAN(eps=eps, min_samples=min_samples, metric="precomputed").fit(D64)
    return sk.labels_, sk.core_sample_indices_


# ------------------------------------------------------------------ (1) the rule is sklearn's
@pytest.mark.parametrize("metric,offset", CASES)
@pytest.mark.parametrize("N,D", SHAPES)
def test_the_rule_gives_sklearns_labels_on_the_lattice_fixtures(N, D, metric, offset):
    X, _ = R.lattice(N, D, offset, metric)
    D64 = R.distances64(X, metric)
    eps = 0.5295 if metric == R.EUCLIDEAN else R.cosine_eps(D64)
    for min_samples in (5, 1, 12):
        labels, core, record = R.labels_from_adjacency(R.adjacency(D64, eps), min_samples)
        want, want_core = _sklearn(D64, eps, min_samples)
        assert np.array_equal(labels, want) and np.array_equal(np.flatnonzero(core), want_core)
        assert record == [want.max() + 1, want_core.size, int((want >= 0).sum()) - want_core.size, int((want < 0).sum())]
    labels, core, record = R.labels_from_adjacency(R.adjacency(D64, eps), 5)
    print(f"({N}, {D}) metric {metric} offset {offset}: eps {eps:.6g}, clusters / core / border / noise {record}")
    assert record[0] >= 2 and record[2] >= 1 and record[3] >= 1       # a fixture with clusters, border rows and noise


def _hand_built():
    """name -> (points, eps, min_samples): the hand-built cases of test_dbscan_gpu.py, small integer coordinates."""
    rng = np.random.default_rng(3)
    chain = np.zeros((1500, 3))
    chain[:, 0] = np.arange(1500)
    cases = {
        # two clusters of four on a line, three apart from a shared border point in the middle
        "border_between_two": (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [3, 0, 0], [5, 0, 0], [6, 0, 0], [5, 1, 0], [6, 1, 0],
                                         [20, 20, 20]], dtype=np.float64), 2.0, 4),
        "chain_reversed": (chain[::-1].copy(), 1.0, 2),
        "chain_interleaved": (np.concatenate([chain[0::2], chain[1::2]]), 1.0, 2),
        "chain_shuffled": (chain[rng.permutation(1500)], 1.0, 3),
        "duplicates": (np.repeat(rng.integers(0, 6, (40, 8)), 3, axis=0).astype(np.float64), 0.5, 1),
    }
    return cases


@pytest.mark.parametrize("name", sorted(_hand_built()))
def test_the_rule_gives_sklearns_labels_on_the_hand_built_cases(name):
    X, eps, min_samples = _hand_built()[name]
    D64 = R.distances64(X, R.EUCLIDEAN)
    labels, core, _ = R.labels_from_adjacency(R.adjacency(D64, eps), min_samples)
    want, want_core = _sklearn(D64, eps, min_samples)
    assert np.array_equal(labels, want) and np.array_equal(np.flatnonzero(core), want_core)
    if name == "border_between_two":
        assert labels.tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1, -1] and not core[4]      # the border point takes the smaller label
    if name.startswith("chain"):
        assert (labels == 0).all()


def test_the_bit_matrix_of_the_restatement():
    D = np.array([[0.0, 1.0, np.nan], [1.0, 0.0, 2.0], [np.nan, 2.0, 5.0]])
    w = R.bit_matrix(D, 1.0)
    assert w.dtype == np.uint64 and w.shape == (3, 1) and w[:, 0].tolist() == [0b011, 0b011, 0b100]      # the diagonal is set
    assert R.popcounts(w, 3).tolist() == [2, 2, 1]
    D65 = np.zeros((65, 65))
    w = R.bit_matrix(D65, 0.0)
    assert w.shape == (65, 2) and (w[:, 0] == np.uint64(2 ** 64 - 1)).all() and (w[:, 1] == 1).all()
    R.check_structure(w, 65)
    assert R.same_partition([0, 0, 1, -1], [1, 1, 0, -1]) and not R.same_partition([0, 0, 1, -1], [0, 1, 1, -1])


# ------------------------------------------------------------------ (2) surface and refusals
def _message(fn):
    with pytest.raises(ValueError) as err:
        fn()
    return str(err.value)


def _sk_message(**kw):
    from sklearn.cluster import DBSCAN
    with pytest.raises(ValueError) as err:
        DBSCAN(**kw).fit(np.zeros((4, 2)))
    return str(err.value)


def _set_free(msg):
    """sklearn prints the options of a str parameter as a set, in no fixed order: compare them as a set."""
    m = re.search(r"\{(.*?)\}", msg)
    return (msg[:m.start()], frozenset(m.group(1).split(", ")), msg[m.end():]) if m else (msg, None, "")


@pytest.mark.parametrize("kw", [dict(eps=0), dict(eps=-1.0), dict(eps="a"), dict(eps=float("nan")), dict(eps=float("inf")),
                                dict(min_samples=0), dict(min_samples=1.5), dict(min_samples="3"), dict(metric="nope"),
                                dict(metric=3), dict(algorithm="fast"), dict(algorithm=None), dict(leaf_size=0), dict(p=-1),
                                dict(n_jobs="x"), dict(metric_params=3)], ids=repr)
def test_parameter_error_sentences_are_sklearns(kw):
    from vit_som_amd import DBSCAN
    ours = _message(lambda: DBSCAN(**kw).fit(torch.zeros(4, 2)))     # refused before the tensor is looked at
    assert _set_free(ours) == _set_free(_sk_message(**kw))


def test_signature_and_defaults_are_sklearns():
    import sklearn.cluster
    from vit_som_amd import DBSCAN
    ours, theirs = inspect.signature(DBSCAN.__init__), inspect.signature(sklearn.cluster.DBSCAN.__init__)
    assert str(ours) == str(theirs)
    assert list(inspect.signature(DBSCAN.fit).parameters)[:4] == ["self", "X", "y", "sample_weight"]


def test_the_departures_raise_with_their_reason():
    from vit_som_amd import DBSCAN, k_distances
    from vit_som_amd import dbscan as M
    x = torch.zeros(4, 2)
    assert "popcount" in _message(lambda: DBSCAN().fit(x, sample_weight=np.ones(4)))
    assert "popcount" in _message(lambda: DBSCAN().fit_predict(x, sample_weight=np.ones(4)))
    for metric in ("manhattan", "l1", "minkowski", "chebyshev"):                  # sklearn's names this class does not compute
        msg = _message(lambda: DBSCAN(metric=metric).fit(x))
        assert "not supported" in msg and "precomputed" in msg
    msg = _message(lambda: DBSCAN(metric=lambda a, b: 0.0).fit(x))               # a callable: sklearn takes it
    assert "callable metric is not supported" in msg and "precomputed" in msg
    assert "not supported" in _message(lambda: DBSCAN(metric_params={"p": 3}).fit(x))
    DBSCAN(algorithm="kd_tree", leaf_size=7, p=1.5, n_jobs=3, metric_params={})._check_params()      # validated, then ignored
    assert "on the GPU" in _message(lambda: DBSCAN().fit(x))
    assert "on the GPU" in _message(lambda: DBSCAN().fit(np.zeros((4, 2))))
    assert "on the GPU" in _message(lambda: k_distances(x, 1))
    assert M.MAX_SAMPLES == 131072 and M.MAX_K == 63 and M.ROUNDS_PER_CALL >= 1
    doc = M.DBSCAN.__doc__ + M.__doc__
    for word in ("sample_weight", "algorithm", "leaf_size", "n_jobs", "callable", "131 072", "fp32", "precomputed", "agglo_distances"):
        assert word in doc, word
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for word in ("DBSCAN", "sample_weight", "leaf_size", "131 072", "agglo_distances"):
        assert word in integration, word


def test_eps_from_the_k_distance_curve():
    from vit_som_amd.dbscan import eps_from_k_distances
    curve = torch.arange(10, dtype=torch.float32)
    assert eps_from_k_distances(curve, 0.5) == 5.0 and eps_from_k_distances(curve, 0.0) == 0.0 and eps_from_k_distances(curve, 1.0) == 9.0
    with pytest.raises(ValueError, match="eps_quantile"):
        eps_from_k_distances(curve, 1.5)


def _stub_rows():
    z = lambda dtype, *shape: torch.zeros(*shape, dtype=dtype)                   # noqa: E731
    N, W = 70, 2
    adj, count, status = z(A.I64, N, W), z(A.I32, N), z(A.I64, 2)
    core, root = z(A.U8, N), z(A.I32, N)
    return {
        "dbscan_neighbours": dict(X=z(A.F32, N, 5), metric=1, eps=0.5, sq=z(A.F32, N), adj=adj, count=count, status=status),
        "dbscan_threshold": dict(M=z(A.F32, N, N), eps=0.5, adj=adj, count=count, status=status),
        "dbscan_threshold[f64]": dict(M=z(A.F64, N, N), eps=0.5, adj=adj, count=count, status=status),
        "dbscan_init": dict(count=count, min_samples=5, core=core, root=root),
        "dbscan_round": dict(adj=adj, core=core, root=root, rounds=2, changed=z(A.I32, 1)),
        "dbscan_finish": dict(adj=adj, core=core, root=root, labels=z(A.I64, N), record=z(A.I32, 4)),
    }


@pytest.mark.parametrize("name", sorted(_stub_rows()))
def test_host_tensors_are_refused_before_the_library(monkeypatch, name):
    from vit_som_amd import ops
    stub = A.StubLib()
    monkeypatch.setattr(ops, "lib", stub)
    with pytest.raises(ValueError, match="expected a HIP device tensor"):
        getattr(ops, name.split("[")[0])(**_stub_rows()[name])
    assert stub.calls == []


def test_every_new_entry_is_declared_exported_and_refuses_on_the_host():
    from test_abi import header_functions
    from vit_som_amd._lib import LIB_PATH, SIGNATURES, last_error, lib
    raw = ctypes.CDLL(LIB_PATH)
    for name in ENTRIES:
        assert name in header_functions() and name in SIGNATURES and hasattr(raw, name), name
    P = 4096                                                         # never dereferenced: every call below is refused first
    assert lib.vsom_dbscan_neighbours(None, 8, 10, 8, 1, 0.5, P, P, P, P, None) == -1 and "null" in last_error()
    assert lib.vsom_dbscan_neighbours(P, 8, 1, 8, 1, 0.5, P, P, P, P, None) == -1               # N < 2
    assert lib.vsom_dbscan_neighbours(P, 4, 10, 8, 1, 0.5, P, P, P, P, None) == -1              # ldx < D
    assert lib.vsom_dbscan_neighbours(P, 8, 10, 8, 1, -0.5, P, P, P, P, None) == -1 and "eps" in last_error()
    assert lib.vsom_dbscan_neighbours(P, 8, 10, 8, 1, float("nan"), P, P, P, P, None) == -1
    assert lib.vsom_dbscan_neighbours(P, 8, 131073, 8, 1, 0.5, P, P, P, P, None) == -3 and "2 GiB" in last_error()
    assert lib.vsom_dbscan_neighbours(P, 8, 10, 8, 7, 0.5, P, P, P, P, None) == -3 and "metric" in last_error()
    assert lib.vsom_dbscan_threshold(P, 9, 10, 0, 0.5, P, P, P, None) == -1                     # ldm < N
    assert lib.vsom_dbscan_threshold(P, 131073, 131073, 1, 0.5, P, P, P, None) == -3
    assert lib.vsom_dbscan_init(P, 10, 0, P, P, None) == -1                                     # min_samples < 1
    assert lib.vsom_dbscan_round(P, 10, P, P, 0, P, None) == -1 and lib.vsom_dbscan_round(P, 10, P, None, 1, P, None) == -1
    assert lib.vsom_dbscan_finish(P, 0, P, P, P, P, None) == -1
    header = open(os.path.join(ROOT, "include", "vitsom_hip.h")).read().replace("\n *", " ")      # comment lines joined
    for word in ("bit (j & 63) of adj[i][j >> 6]", "the diagonal is set", "bits of columns >= N are clear", "symmetric bit for bit",
                 "16 bytes per lane", "natural alignment"):
        assert word in " ".join(header.split()), word


def test_package_exports_and_driver_flag():
    import vit_som_amd
    from vit_som_amd import dbscan, evaluation, train
    for name in ("DBSCAN", "DBSCANReport", "evaluate_dbscan", "k_distances"):
        assert getattr(vit_som_amd, name) is getattr(dbscan, name), name
    assert evaluation.evaluate_dbscan is dbscan.evaluate_dbscan and evaluation.visualize_dbscan is dbscan.visualize_dbscan
    assert str(inspect.signature(dbscan.evaluate_dbscan)) == "(model, config, dataloader, eps=None, min_samples=5, metric=None, eps_quantile=0.5)"
    assert [f for f in dbscan.DBSCANReport.__dataclass_fields__] == [
        "eps", "min_samples", "metric", "n_clusters", "n_core", "n_border", "n_noise", "coverage", "cluster_sizes", "purity", "nmi",
        "noise_per_class", "k_distances", "labels", "n_samples", "inference_time"]
    assert inspect.signature(train.main).parameters["dbscan_eval"].default is False
    assert train._parser().parse_args(["--config", "c"]).dbscan_eval is False
    assert train._parser().parse_args(["--config", "c", "--dbscan-eval"]).dbscan_eval is True
