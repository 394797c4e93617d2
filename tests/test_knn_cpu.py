"""The kNN probe without GPU compute: the restatement (knn_ref.py) on hand-checkable cases, the host arithmetic and the
argument refusals of vsom_knn_query / vsom_knn_vote, KNNClassifier's ValueErrors and the driver flag."""
import numpy as np
import pytest
import torch

import knn_ref as R


# ------------------------------------------------------------------ the restatement
def test_ties_go_to_the_lower_index():
    Q = np.array([[0.0, 0.0]])
    X = np.array([[1.0, 0.0], [0.0, 2.0], [0.0, 1.0], [-1.0, 0.0], [3.0, 0.0]])
    idx, dist = R.topk(R.distances(Q, X, R.EUCLIDEAN), 4)
    assert idx.tolist() == [[0, 2, 3, 1]] and dist.tolist() == [[1.0, 1.0, 1.0, 2.0]]
    idx, _ = R.topk(R.distances(Q, X, R.EUCLIDEAN), 2, index_base=100)
    assert idx.tolist() == [[100, 102]]


def test_cosine_conventions():
    Q = np.array([[0.0, 0.0], [1.0, 1.0], [2.0, 0.0]])
    X = np.array([[0.0, 0.0], [1.0, 1.0], [0.0, 3.0], [-1.0, -1.0], [1.0, 0.0]])
    D = R.distances(Q, X, R.COSINE)
    assert D[0].tolist() == [0.0, 1.0, 1.0, 1.0, 1.0]              # zero query: 0 from the zero row, 1 from every other
    assert D[1, 0] == 1.0 and D[1, 1] == 0.0                       # a zero bank row; an identical row exactly 0
    assert abs(D[1, 2] - (1.0 - 1.0 / np.sqrt(2.0))) < 1e-15 and abs(D[1, 3] - 2.0) < 1e-15
    assert D[2, 4] == 0.0 or D[2, 4] < 1e-15                       # parallel rows: clamped at 0, never negative
    assert (D >= 0).all()


def test_exclude_and_tail():
    Q = X = np.array([[0.0], [1.0], [3.0]])
    D = R.distances(Q, X, R.EUCLIDEAN)
    idx, dist = R.topk(D, 2, exclude=np.arange(3))
    assert idx.tolist() == [[1, 2], [0, 2], [1, 0]] and dist.tolist() == [[1.0, 3.0], [1.0, 2.0], [2.0, 3.0]]
    idx, dist = R.topk(D, 4, exclude=np.arange(3))                 # two candidates for four slots
    assert idx[:, 2:].tolist() == [[-1, -1]] * 3 and np.isinf(dist[:, 2:]).all()
    # exclude names GLOBAL ordinals: with a base of 10 nothing is excluded
    idx, _ = R.topk(D, 1, index_base=10, exclude=np.arange(3))
    assert idx.tolist() == [[10], [11], [12]]


def test_streaming_equals_one_piece_in_the_restatement():
    rng = np.random.default_rng(0)
    Q, X = rng.integers(-2, 3, (7, 3)).astype(float), rng.integers(-2, 3, (23, 3)).astype(float)
    D = R.distances(Q, X, R.EUCLIDEAN)
    whole = R.topk(D, 5)
    idx, dist = R.empty_lists(7, 5)
    for a, b in ((15, 23), (0, 4), (4, 15)):
        idx, dist = R.fold(idx, dist, D[:, a:b], index_base=a)
    assert np.array_equal(idx, whole[0]) and np.array_equal(dist, whole[1])


def test_vote_rules():
    labels = np.array([0, 1, 1, 2, 5])
    idx = np.array([[0, 1, 2], [3, 0, -1], [-1, -1, -1], [0, 4, 9]])
    dist = np.array([[0.5, 1.0, 2.0], [0.0, 0.0, np.inf], [np.inf] * 3, [1.0, 1.0, 1.0]], dtype=np.float32)
    pred, scores, status = R.vote(idx, dist, labels, 3, R.UNIFORM)
    assert pred.tolist() == [1, 0, -1, 0]                          # row 1: classes 2 and 0 tie at 1 vote -> the lowest class
    assert scores[0].tolist() == [1.0, 2.0, 0.0] and status == [2, 1]        # label 5 and index 9 refused; one empty query
    pred, scores, _ = R.vote(idx, dist, labels, 3, R.DISTANCE)
    assert scores[0].tolist() == [2.0, 1.5, 0.0] and pred[0] == 0            # 1/0.5 against 1/1 + 1/2
    assert scores[1].tolist() == [1.0, 0.0, 1.0] and pred[1] == 0            # both at distance 0: weight 1 each
    d0 = np.array([[0.0, 0.25, 0.25]], dtype=np.float32)
    pred, scores, _ = R.vote(np.array([[0, 1, 2]]), d0, labels, 3, R.DISTANCE)
    assert scores[0].tolist() == [1.0, 0.0, 0.0] and pred[0] == 0            # a neighbour at 0 takes the whole vote
    pred, scores, _ = R.vote(idx[:1], dist[:1], labels, 3, R.SOFTMAX, temperature=0.5)
    T = np.float64(np.float32(0.5))
    # shifted by the query's smallest valid distance (0.5): the nearest neighbour weighs exactly 1
    assert scores[0, 0] == 1.0 and scores[0, 1] == np.exp(-0.5 / T) + np.exp(-1.5 / T) and pred[0] == 0
    far = np.array([[100.0, 100.5, 101.0]], dtype=np.float32)                # exp(-100 / 0.07) underflows; the shift does not
    pred, scores, _ = R.vote(np.array([[3, 1, 2]]), far, labels, 3, R.SOFTMAX, temperature=0.07)
    assert scores[0, 2] == 1.0 and 0.0 < scores[0, 1] < 1e-3 and pred[0] == 2


# ------------------------------------------------------------------ the C-ABI, host side
def test_workspace_bytes_is_host_arithmetic():
    from vit_som_amd._lib import lib
    f = lib.vsom_knn_query_workspace_bytes
    assert f(0, 10, 5) == 0 and f(10, 0, 5) == 0 and f(10, 10, 0) == 0 and f(-3, 10, 5) == 0
    assert f(1, 1, 1) > 0
    for Nb in (1, 64, 4096, 100000):
        sizes = [f(Nq, Nb, 20) for Nq in (1, 127, 128, 129, 255, 256, 257, 384, 385, 1000, 10000, 262144, 262145, 1000000)]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])), (Nb, sizes)
        sizes = [f(1000, Nb, k) for k in range(1, 65)]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])), (Nb, sizes)
    # the two norm vectors and candidate slabs for every query
    assert f(10000, 4096, 20) >= 4 * (10000 + 4096) + 2 * 4 * 10000 * 20


def test_argument_refusals_without_a_launch():
    """Bad calls are refused on the host before any launch (negative VSOM_E* codes); 16 stands for a non-null pointer."""
    from vit_som_amd._lib import last_error, lib
    big = 1 << 30

    def query(Q=16, ldq=4, Nq=4, X=16, ldx=4, Nb=4, D=4, k=2, metric=0, base=0, idx=16, dist=16, ws=16, ws_bytes=big):
        return lib.vsom_knn_query(Q, ldq, Nq, X, ldx, Nb, D, k, metric, base, 0, None, idx, dist, ws, ws_bytes, None)

    for null in ("Q", "X", "idx", "dist"):
        assert query(**{null: None}) == -1 and "null" in last_error()
    assert query(k=65) == -3 and "k=65" in last_error()
    assert query(metric=7) == -3 and "metric 7" in last_error()
    assert query(metric=2) == -3                                   # manhattan: not a kNN metric
    assert query(ws_bytes=lib.vsom_knn_query_workspace_bytes(4, 4, 2) - 1) == -4 and "workspace" in last_error()
    assert query(ws=None) == -4
    assert query(ws=24) == -4                                      # not 16-byte aligned
    assert query(ldq=3) == -1 and query(ldx=3) == -1 and query(D=0) == -1 and query(k=0) == -1
    assert query(Nq=0) == -1 and query(Nb=0) == -1 and query(base=-1) == -1
    assert query(Nq=2 ** 31) == -1 and query(Nb=2 ** 31) == -1

    def vote(idx=16, dist=16, Nq=4, k=2, labels=16, n_bank=4, n_classes=10, weights=0, T=0.07, pred=16, status=16):
        return lib.vsom_knn_vote(idx, dist, Nq, k, labels, n_bank, n_classes, weights, T, pred, None, status, None)

    for null in ("idx", "dist", "labels", "pred", "status"):
        assert vote(**{null: None}) == -1 and "null" in last_error()
    assert vote(k=65) == -3
    assert vote(n_classes=1025) == -3 and "1025" in last_error()
    assert vote(weights=2, T=0.0) == -1 and "temperature" in last_error()
    assert vote(weights=2, T=-1.0) == -1
    assert vote(weights=3) == -3
    assert vote(Nq=0) == -1 and vote(n_classes=0) == -1 and vote(n_bank=0) == -1


# ------------------------------------------------------------------ KNNClassifier
def test_classifier_value_errors():
    from vit_som_amd import KNNClassifier
    X, y = torch.zeros(8, 4), torch.zeros(8, dtype=torch.int64)
    with pytest.raises(ValueError, match="exceeds the kernel's limit of 64"):
        KNNClassifier(n_neighbors=65).fit(X, y)
    with pytest.raises(ValueError, match="n_neighbors"):
        KNNClassifier(n_neighbors=0).fit(X, y)
    with pytest.raises(ValueError, match="weights"):
        KNNClassifier(weights="gaussian").fit(X, y)
    with pytest.raises(ValueError, match="metric"):
        KNNClassifier(metric="manhattan").fit(X, y)
    with pytest.raises(ValueError, match="temperature"):
        KNNClassifier(weights="softmax", temperature=0.0).fit(X, y)
    with pytest.raises(ValueError, match="1024"):
        KNNClassifier(n_classes=1025).fit(X, y)
    with pytest.raises(ValueError, match="float32"):
        KNNClassifier().fit(X.double(), y)
    with pytest.raises(ValueError, match="on the GPU"):
        KNNClassifier().fit(X, y)
    with pytest.raises(ValueError, match="float32"):
        KNNClassifier().partial_fit_query(X.half())
    with pytest.raises(ValueError, match="fit"):
        KNNClassifier().predict(X)
    with pytest.raises(ValueError, match="partial_fit_query"):
        KNNClassifier().update(X, y)
    with pytest.raises(ValueError, match="no queries"):
        KNNClassifier().predict()


def test_driver_flag_parses_and_defaults_to_off():
    import inspect
    from vit_som_amd import train
    assert train._parser().parse_args(["--config", "c.yaml"]).knn_eval is False
    assert train._parser().parse_args(["--config", "c.yaml", "--knn-eval"]).knn_eval is True
    assert inspect.signature(train.main).parameters["knn_eval"].default is False
