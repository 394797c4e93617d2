"""The kNN probe on the MI355X: vsom_knn_query against fp64 and against the restatement (knn_ref.py), its conventions,
streaming invariance, leave-one-out against vsom_umap_knn, reproducibility; vsom_knn_vote against the restatement;
KNNClassifier; evaluate_knn on the tiny fixtures, through the driver and over two ranks."""
import copy

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import knn_ref as R
from helpers import golden_params, load_golden
from knn_checks import lists_against_fp64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
METRIC = {"cosine": R.COSINE, "euclidean": R.EUCLIDEAN}


def _randn(Nq, Nb, D, seed=1):
    g = torch.Generator().manual_seed(seed)
    Q = torch.randn(Nq, D, generator=g)
    X = torch.randn(Nb, D, generator=g)
    return Q, X


def _query(Q, X, k, metric, poison=-7, **kw):
    """One vsom_knn_query call into poisoned outputs (device tensors in, device tensors out)."""
    from vit_som_amd import ops
    idx = torch.full((Q.shape[0], k), poison, dtype=torch.int64, device=DEV)
    dist = torch.full((Q.shape[0], k), float(poison), dtype=torch.float32, device=DEV)
    ops.knn_query(Q, X, k, METRIC[metric], idx, dist, **kw)
    return idx, dist


def _stream(Q, X, k, metric, pieces):
    """The bank folded piece by piece: pieces = [(a, b), ...] row ranges, index_base = a."""
    from vit_som_amd import ops
    idx = torch.full((Q.shape[0], k), -9, dtype=torch.int64, device=DEV)
    dist = torch.full((Q.shape[0], k), -9.0, dtype=torch.float32, device=DEV)
    for n, (a, b) in enumerate(pieces):
        ops.knn_query(Q, X[a:b], k, METRIC[metric], idx, dist, index_base=a, accumulate=n > 0)
    return idx, dist


# ------------------------------------------------------------------ 1. against fp64
FP64_CASES = [(130, 257, 3, 2), (130, 257, 1003, 64), (333, 1000, 64, 20), (65, 3000, 3136, 15), (257, 700, 12288, 20),
              (1, 64, 8, 64)]


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("Nq,Nb,D,k", FP64_CASES)
def test_query_against_fp64(Nq, Nb, D, k, metric):
    """test_umap_gpu.py::test_knn_against_fp64's checks and tolerances (the project's own for this contraction): the fp64
    distance of every chosen index agrees with the returned one (cosine 1e-5; euclidean squared, 1e-5 (|q|^2 + |x|^2)), the
    lists ascend, indices are valid, and on every row whose k + 1 smallest fp64 distances are pairwise further apart than
    that tolerance the indices are the fp64 top-k exactly."""
    Q, X = (t.to(DEV) for t in _randn(Nq, Nb, D))
    idx, dist = _query(Q, X, k, metric)
    idx2, dist2 = _query(Q, X, k, metric, poison=-3)
    torch.cuda.synchronize()
    assert torch.equal(idx, idx2) and torch.equal(dist, dist2)
    share, _ = lists_against_fp64(idx, dist, Q, X, k, metric)         # knn_checks.py: shared with the edge suite
    print(f"({Nq}, {Nb}, {D}, {k}) {metric}: rows compared index by index {share:.3f}")
    assert share >= (0.25 if (Nq, Nb, D, k) == (130, 257, 1003, 64) else 0.5), share


# ------------------------------------------------------------------ 2. exact on integer data
@pytest.fixture(scope="module")
def integer_data():
    g = torch.Generator().manual_seed(2)
    Q = torch.randint(-3, 4, (200, 40), generator=g).float()
    X = torch.randint(-3, 4, (500, 40), generator=g).float()
    return Q, X


def test_integer_data_euclidean_is_exact(integer_data):
    """Every dot product and norm is an integer below 2^24: exact in fp32, so the neighbours are decided exactly (ties
    are plentiful) and the distances are float32(sqrt(integer)) bit for bit -- on every row."""
    Q, X = integer_data
    k = 64
    idx, dist = _query(Q.to(DEV), X.to(DEV), k, "euclidean")
    D2 = ((Q.double()[:, None, :] - X.double()[None, :, :]) ** 2).sum(-1).numpy()
    assert len(np.unique(D2[0])) < 200                               # ties are plentiful
    ri, rd = R.topk(R.distances(Q.numpy(), X.numpy(), R.EUCLIDEAN), k)
    assert np.array_equal(idx.cpu().numpy(), ri)
    want = np.sqrt(np.take_along_axis(D2, ri, axis=1)).astype(np.float32)
    assert np.array_equal(dist.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(want, rd.astype(np.float32))


def test_integer_data_cosine(integer_data):
    """The same data under cosine: dot products and squared norms are exact, the two square roots, the product, the
    quotient and the difference round (below 4e-7 in all), so rows whose k + 1 smallest distances are 1e-6 apart must
    match the restatement index for index."""
    Q, X = integer_data
    k = 64
    idx, dist = _query(Q.to(DEV), X.to(DEV), k, "cosine")
    Dc = R.distances(Q.numpy(), X.numpy(), R.COSINE)
    ri, rd = R.topk(Dc, k)
    srt = np.sort(Dc, axis=1)[:, :k + 1]
    clear = (np.diff(srt, axis=1) > 1e-6).all(axis=1)
    got = idx.cpu().numpy()
    assert np.array_equal(got[clear], ri[clear])
    assert np.abs(dist.cpu().numpy().astype(np.float64) - np.take_along_axis(Dc, got, axis=1)).max() <= 1e-6
    print(f"integer cosine: rows compared index by index {clear.mean():.3f}")


# ------------------------------------------------------------------ 3. conventions
def test_cosine_conventions():
    g = torch.Generator().manual_seed(3)
    X = torch.randn(64, 16, generator=g)
    X[10] = X[4]
    X[20] = 0.0
    Q = torch.randn(3, 16, generator=g)
    Q[0] = X[4]
    Q[1] = 0.0
    idx, dist = _query(Q.to(DEV), X.to(DEV), 5, "cosine")
    idx, dist = idx.cpu(), dist.cpu()
    assert idx[0, :2].tolist() == [4, 10] and dist[0, :2].tolist() == [0.0, 0.0] and dist[0, 2] > 0
    assert idx[1].tolist() == [20, 0, 1, 2, 3] and dist[1].tolist() == [0.0, 1.0, 1.0, 1.0, 1.0]
    assert 20 not in idx[2].tolist() or dist[2][idx[2].tolist().index(20)] == 1.0
    # euclidean: the duplicate pair at exactly 0 as well
    idx, dist = _query(Q.to(DEV), X.to(DEV), 5, "euclidean")
    assert idx[0, :2].tolist() == [4, 10] and dist[0, :2].tolist() == [0.0, 0.0]


# ------------------------------------------------------------------ 4. streaming invariance
@pytest.fixture(scope="module")
def lists_333():
    """Case (333, 1000, 64, 20), cosine, in one call: shared by the streaming, reproducibility and vote tests (read only)."""
    Q, X = (t.to(DEV) for t in _randn(333, 1000, 64))
    idx, dist = _query(Q, X, 20, "cosine")
    torch.cuda.synchronize()
    return Q, X, idx, dist


def test_streaming_is_bitwise_invariant(lists_333):
    Q, X, idx, dist = lists_333
    for metric in ("cosine", "euclidean"):
        one = (idx, dist) if metric == "cosine" else _query(Q, X, 20, metric)
        a = _stream(Q, X, 20, metric, [(s, min(s + 257, 1000)) for s in range(0, 1000, 257)])
        b = _stream(Q, X, 20, metric, [(700, 1000), (0, 300), (300, 700)])
        for got in (a, b):
            assert torch.equal(got[0], one[0]) and torch.equal(got[1], one[1]), metric


def test_streaming_is_bitwise_invariant_at_the_latent_width():
    Q, X = (t.to(DEV) for t in _randn(257, 700, 12288))
    one = _query(Q, X, 20, "cosine")
    got = _stream(Q, X, 20, "cosine", [(s, min(s + 64, 700)) for s in range(0, 700, 64)])
    assert torch.equal(got[0], one[0]) and torch.equal(got[1], one[1])


def test_short_bank_leaves_an_empty_tail_that_a_second_chunk_fills(lists_333):
    Q, X, _, _ = lists_333
    idx, dist = _query(Q, X[:10], 20, "cosine")
    assert (idx[:, 10:] == -1).all() and torch.isinf(dist[:, 10:]).all() and (dist[:, 10:] > 0).all()
    assert (idx[:, :10] >= 0).all() and torch.isfinite(dist[:, :10]).all()
    assert (idx[:, :10].sort(dim=1).values == torch.arange(10, device=DEV)).all()
    got = _stream(Q, X, 20, "cosine", [(0, 10), (10, 40)])
    one = _query(Q, X[:40], 20, "cosine")
    assert torch.equal(got[0], one[0]) and torch.equal(got[1], one[1]) and (got[0] >= 0).all()


def test_element_wise_loads_give_the_same_bits(lists_333):
    """The same rows from a base pointer 4 bytes off 16-byte alignment take the generic load path: identical lists."""
    Q, X, idx, dist = lists_333
    buf = torch.zeros(X.numel() + 4, device=DEV)
    Xo = buf[1:1 + X.numel()].view_as(X)
    Xo.copy_(X)
    assert Xo.data_ptr() % 16 != 0
    got = _query(Q, Xo, 20, "cosine")
    assert torch.equal(got[0], idx) and torch.equal(got[1], dist)


# ------------------------------------------------------------------ 5. leave-one-out against vsom_umap_knn
@pytest.mark.parametrize("N", [500, 461])                              # 461: the last 64-column tile holds 13 columns, fewer than a wave's 32 rows
@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_leave_one_out_equals_umap_knn(metric, N):
    """Queries = bank with exclude = arange(N): no row returns itself, and the lists are columns 1 .. k of vsom_umap_knn
    with k + 1 on the same data (no duplicate rows), distances bit for bit: the query and the self mode of the one search,
    held together."""
    from vit_som_amd import ops
    D, k = 32, 15
    X = _randn(1, N, D, seed=5)[1].to(DEV)
    ar = torch.arange(N, device=DEV)
    idx, dist = _query(X, X, k, metric, exclude=ar)
    assert (idx != ar[:, None]).all()
    ui = torch.empty(N, k + 1, dtype=torch.int64, device=DEV)
    ud = torch.empty(N, k + 1, dtype=torch.float32, device=DEV)
    ops.umap_knn(X, k + 1, METRIC[metric], ui, ud)
    assert torch.equal(ui[:, 0], ar)
    assert torch.equal(idx, ui[:, 1:]) and torch.equal(dist, ud[:, 1:])
    # without exclude every row finds itself first, at exactly 0
    idx0, dist0 = _query(X, X, k, metric)
    assert torch.equal(idx0[:, 0], ar) and (dist0[:, 0] == 0).all() and torch.equal(idx0[:, 1:], idx[:, :-1])


@pytest.mark.parametrize("N,D", [(461, 32), (130, 3)])                 # 130 x 3: two row blocks, element-wise loads, D below one 8-group
@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_self_mode_equals_query_mode_with_duplicates(metric, N, D):
    """Rows 3, 5 and N // 2 identical, row 7 zero.  vsom_knn_query(X, X) holds row i in its own list at exactly 0, among its
    duplicates by index; moved to the front, the list is vsom_umap_knn's bit for bit.  A row without a duplicate is first
    already."""
    from vit_som_amd import ops
    k = 15
    X = _randn(1, N, D, seed=6)[1]
    X[5] = X[3]
    X[N // 2] = X[3]
    X[7] = 0.0
    X = X.to(DEV)
    ar = torch.arange(N, device=DEV)
    idx, dist = _query(X, X, k, metric)
    own = idx == ar[:, None]
    assert (own.sum(1) == 1).all() and (dist[own] == 0).all()
    slot = torch.arange(k, device=DEV).expand(N, k)
    order = torch.where(own, -1, slot).argsort(dim=1, stable=True)     # the row's own entry first, the rest as they were
    qi, qd = idx.gather(1, order), dist.gather(1, order)
    ui = torch.full((N, k), -7, dtype=torch.int64, device=DEV)
    ud = torch.full((N, k), -7.0, dtype=torch.float32, device=DEV)
    ops.umap_knn(X, k, METRIC[metric], ui, ud)
    assert torch.equal(ui, qi) and torch.equal(ud, qd)
    single = torch.ones(N, dtype=torch.bool, device=DEV)
    single[[3, 5, N // 2]] = False
    assert torch.equal(ui[single], idx[single]) and torch.equal(ud[single], dist[single])
    assert ui[5, :3].tolist() == [5, 3, N // 2] and ud[5, :3].tolist() == [0.0, 0.0, 0.0]


# ------------------------------------------------------------------ 6. reproducibility
def test_two_calls_are_bitwise_equal(lists_333):
    Q, X, idx, dist = lists_333
    again = _query(Q, X, 20, "cosine", poison=-1)
    assert torch.equal(again[0], idx) and torch.equal(again[1], dist)


# ------------------------------------------------------------------ 7. the vote
def _vote(idx, dist, labels, n_classes, weights, T=0.07):
    from vit_som_amd import ops
    Nq = idx.shape[0]
    pred = torch.full((Nq,), -5, dtype=torch.int64, device=DEV)
    scores = torch.full((Nq, n_classes), -5.0, dtype=torch.float64, device=DEV)
    status = torch.zeros(2, dtype=torch.int32, device=DEV)
    ops.knn_vote(idx, dist, labels, n_classes, weights, T, pred, status, scores)
    pred2 = torch.full((Nq,), -6, dtype=torch.int64, device=DEV)
    ops.knn_vote(idx, dist, labels, n_classes, weights, T, pred2, torch.zeros_like(status), None)     # scores are optional
    assert torch.equal(pred, pred2)
    return pred.cpu().numpy(), scores.cpu().numpy(), status.cpu().tolist()


@pytest.fixture(scope="module")
def vote_inputs(lists_333):
    _, _, idx, dist = lists_333
    labels = torch.randint(0, 10, (1000,), generator=torch.Generator().manual_seed(7))
    return idx, dist, labels.to(DEV), idx.cpu().numpy(), dist.cpu().numpy(), labels.numpy()


@pytest.mark.parametrize("weights", [R.UNIFORM, R.DISTANCE])
def test_vote_uniform_and_distance_are_exact(vote_inputs, weights):
    """fp64 sums in neighbour order on both sides (1 / d is one correctly rounded division): bit for bit, ties included."""
    idx, dist, labels, idx_h, dist_h, labels_h = vote_inputs
    pred, scores, status = _vote(idx, dist, labels, 10, weights)
    rp, rs, rstat = R.vote(idx_h, dist_h, labels_h, 10, weights)
    assert status == rstat == [0, 0]
    assert np.array_equal(scores.view(np.uint64), rs.view(np.uint64))
    assert np.array_equal(pred, rp)
    if weights == R.UNIFORM:
        top = np.sort(rs, axis=1)
        assert (top[:, -1] == top[:, -2]).any()                       # vote ties occur and went to the lowest class


def test_vote_softmax(vote_inputs):
    idx, dist, labels, idx_h, dist_h, labels_h = vote_inputs
    pred, scores, status = _vote(idx, dist, labels, 10, R.SOFTMAX, 0.07)
    rp, rs, rstat = R.vote(idx_h, dist_h, labels_h, 10, R.SOFTMAX, 0.07)
    assert status == rstat == [0, 0]
    assert (np.abs(scores - rs) <= 1e-12 * rs).all() and np.array_equal(scores == 0, rs == 0)      # device exp against numpy's
    top = np.sort(rs, axis=1)
    clear = (top[:, -1] - top[:, -2]) > 1e-9 * top[:, -1]
    assert np.array_equal(pred[clear], rp[clear])
    assert clear.mean() >= 0.99, clear.mean()


@pytest.mark.parametrize("weights", [R.UNIFORM, R.DISTANCE, R.SOFTMAX])
def test_vote_counts_what_it_skips(vote_inputs, weights):
    idx, dist, labels, _, _, _ = vote_inputs
    idx, dist, labels = idx[:40].clone(), dist[:40].clone(), labels.clone()
    idx[0, 0] = 1000                                                  # an index >= n_bank
    idx[1, 3] = 2 ** 40
    labels[idx[2, 0]] = 10                                            # labels outside [0, n_classes)
    labels[idx[3, 1]] = -1
    idx[4, :] = -1                                                    # a query whose list is empty
    dist[4, :] = float("inf")
    idx[5, 5:] = -1                                                   # a short list
    dist[5, 5:] = float("inf")
    dist[6, 0] = 0.0                                                  # a neighbour at distance 0
    pred, scores, status = _vote(idx, dist, labels, 10, weights)
    rp, rs, rstat = R.vote(idx.cpu().numpy(), dist.cpu().numpy(), labels.cpu().numpy(), 10, weights)
    assert status == rstat and status[0] >= 4 and status[1] == 1
    assert pred[4] == -1 and (scores[4] == 0).all()
    if weights == R.SOFTMAX:
        assert (np.abs(scores - rs) <= 1e-12 * rs).all()
        top = np.sort(rs, axis=1)
        clear = (top[:, -1] - top[:, -2]) > 1e-9 * top[:, -1]
        assert np.array_equal(pred[clear | (rp < 0)], rp[clear | (rp < 0)])
    else:
        assert np.array_equal(scores, rs) and np.array_equal(pred, rp)


# ------------------------------------------------------------------ 8. KNNClassifier
def _blobs(n_train=400, n_test=100, ncls=4, D=16, seed=11):
    """Two well-separated Gaussian blobs per class."""
    g = torch.Generator().manual_seed(seed)
    centers = 20.0 * torch.randn(2 * ncls, D, generator=g)

    def make(n):
        b = torch.randint(0, 2 * ncls, (n,), generator=g)
        return (centers[b] + torch.randn(n, D, generator=g)).to(DEV), (b % ncls).to(DEV)
    return make(n_train), make(n_test)


@pytest.mark.parametrize("weights", ["uniform", "distance", "softmax"])
@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_classifier_on_blobs(weights, metric):
    from vit_som_amd import KNNClassifier
    (X, y), (Q, yq) = _blobs()
    clf = KNNClassifier(n_neighbors=10, weights=weights, metric=metric, temperature=0.5).fit(X, y)
    pred = clf.predict(Q)
    assert pred.dtype == torch.int64 and pred.is_cuda and torch.equal(pred, yq)
    assert clf.score(Q, yq) == 1.0 and clf.refused() == 0
    scores = clf.predict_scores(Q)
    assert scores.shape == (100, 4) and scores.dtype == torch.float64 and torch.equal(scores.argmax(1), yq)
    assert KNNClassifier(n_neighbors=10, weights=weights, metric=metric, temperature=0.5, n_classes=6).fit(X, y).score(Q, yq) == 1.0


def test_classifier_leave_one_out_and_streaming():
    from vit_som_amd import KNNClassifier, ops
    (X, y), (Q, yq) = _blobs()
    clf = KNNClassifier(n_neighbors=10, metric="euclidean").fit(X, y)
    dist, idx = clf.kneighbors()                                       # leave-one-out on the bank
    ui = torch.empty(400, 11, dtype=torch.int64, device=DEV)
    ud = torch.empty(400, 11, dtype=torch.float32, device=DEV)
    ops.umap_knn(X, 11, R.EUCLIDEAN, ui, ud)
    assert torch.equal(idx, ui[:, 1:]) and torch.equal(dist, ud[:, 1:])
    assert torch.equal(clf.kneighbors(return_distance=False), idx)
    # streaming update equals fit
    dq, iq = clf.kneighbors(Q)
    s = KNNClassifier(n_neighbors=10, metric="euclidean").partial_fit_query(Q)
    for a in range(0, 400, 150):
        s.update(X[a:a + 150], y[a:a + 150])
    ds, is_ = s.kneighbors()
    assert torch.equal(is_, iq) and torch.equal(ds, dq)
    assert torch.equal(s.predict(), clf.predict(Q)) and torch.equal(s.predict_scores(), clf.predict_scores(Q))
    with pytest.raises(ValueError, match="exceeds the bank"):
        KNNClassifier(n_neighbors=10).fit(X[:5].contiguous(), y[:5]).predict(Q)
    with pytest.raises(ValueError, match="contiguous"):
        KNNClassifier().fit(X[:, ::2], y)
    with pytest.raises(ValueError, match="columns"):
        clf.kneighbors(Q[:, :8].contiguous())


# ------------------------------------------------------------------ 9. evaluate_knn
def _model(name):
    import vit_som_amd
    z, cfg = load_golden(name)
    cls = vit_som_amd.DESOM if cfg["hyperparameters"]["model_arch"] == "desom" else vit_som_amd.ViTSOM
    m = cls(copy.deepcopy(cfg), device=DEV)
    m.load_state_dict(golden_params(z))
    return m, cfg


def _split(cfg, seed, ncls, n_per, n_train, nb_train, nb_test):
    """One class-structured set (test_kmeans_gpu._separable_images: a prototype per class plus noise, shuffled), its first
    n_train samples in batches of nb_train as the bank and the rest in batches of nb_test as the queries."""
    from test_kmeans_gpu import _separable_images
    d = cfg["data"]
    batches = _separable_images(seed, n_per, ncls, d["num_channels"], d["input_size"], 10)
    x, y = torch.cat([b[0] for b in batches]), torch.cat([b[1] for b in batches])
    cut = lambda a, b, nb: [(x[i:min(i + nb, b)], y[i:min(i + nb, b)]) for i in range(a, b, nb)]      # noqa: E731
    return cut(0, n_train, nb_train), cut(n_train, len(y), nb_test)


def _loaders(cfg, ncls, seed=21):
    """train: ncls x 24 samples in batches of 10; test: ncls x 8 in batches of 7 (a short last batch each)."""
    return _split(cfg, seed, ncls, 32, 24 * ncls, 10, 7)


def _features(m, cfg, loader):
    d = cfg["data"]
    f, ys = [], []
    for x, y in loader:
        z = m.get_latent_representation(x.to(DEV).reshape(-1, d["num_channels"], d["input_size"], d["input_size"]))
        f.append(z.reshape(z.shape[0], -1).clone())
        ys.append(y.to(DEV))
    return torch.cat(f).contiguous(), torch.cat(ys)


def _same_report(a, b):
    assert a.accuracy == b.accuracy and a.n_train == b.n_train and a.n_test == b.n_test and a.k == b.k
    assert np.array_equal(a.confusion, b.confusion) and np.array_equal(a.per_class_accuracy, b.per_class_accuracy, equal_nan=True)


def test_evaluate_knn_on_the_tiny_fixture():
    from vit_som_amd import KNNClassifier, KNNReport
    from vit_som_amd.evaluation import evaluate_knn
    m, cfg = _model("ref_cls_tiny")
    d = cfg["data"]
    m.set_schedule(120, 100)
    (opt,), _ = m.configure_optimizers()
    g = torch.Generator().manual_seed(0)

    def step():
        x = torch.rand(5, d["num_channels"], d["input_size"], d["input_size"], generator=g).to(DEV)
        loss = m.train_step_fused(x, torch.randint(0, 5, (5,), generator=g).to(DEV))
        opt.step()
        return loss
    m.train()
    for _ in range(3):                                                 # the third step records the launch tape
        step()
    train, test = _loaders(cfg, 5)
    rep = evaluate_knn(m, cfg, train, test, k=10)
    assert isinstance(rep, KNNReport) and (rep.n_train, rep.n_test, rep.k) == (120, 40, 10) and rep.inference_time > 0
    assert rep.confusion.shape == (5, 5) and rep.confusion.dtype == np.int64 and rep.confusion.sum() == 40
    assert rep.per_class_accuracy.shape == (5,)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(rep.per_class_accuracy, np.diag(rep.confusion) / rep.confusion.sum(axis=1), equal_nan=True)
    assert rep.accuracy == np.diag(rep.confusion).sum() / 40
    X, y = _features(m, cfg, train)
    Q, yq = _features(m, cfg, test)
    clf = KNNClassifier(n_neighbors=10, weights="softmax", metric="cosine", temperature=0.07, n_classes=5).fit(X, y)
    assert rep.accuracy == clf.score(Q, yq)
    pred = clf.predict(Q).cpu().numpy()
    cm = np.zeros((5, 5), dtype=np.int64)
    np.add.at(cm, (yq.cpu().numpy(), pred), 1)
    assert np.array_equal(rep.confusion, cm)
    _same_report(evaluate_knn(m, cfg, train, test, k=10, bank_rows=7), rep)       # many folds and a partial last buffer
    _same_report(evaluate_knn(m, cfg, train, test, k=10, bank_rows=120), rep)     # the bank exactly fills the buffer once
    with pytest.raises(ValueError, match="exceeds the 10 training"):
        evaluate_knn(m, cfg, train[:1], test, k=20)                    # one batch of ten as the whole bank
    with pytest.raises(ValueError, match="num_labels"):
        evaluate_knn(m, cfg, train, test, k=10, num_labels=3)
    # the model's training buffers and launch tape are left usable
    m.train()
    loss = step()
    torch.cuda.synchronize()
    assert np.isfinite(float(loss))


def test_evaluate_knn_desom_and_unsupported_models():
    from test_classifier_gpu import _model as _vit_classifier
    from vit_som_amd.evaluation import evaluate_knn
    m, cfg = _model("ref_desom_tiny")
    train, test = _loaders(cfg, 4)
    rep = evaluate_knn(m, cfg, train, test, k=5, num_labels=4)
    assert (rep.n_train, rep.n_test) == (96, 32) and rep.confusion.shape == (4, 4) and rep.confusion.sum() == 32
    assert 0.0 <= rep.accuracy <= 1.0
    _same_report(evaluate_knn(m, cfg, train, test, k=5, num_labels=4, bank_rows=7, metric="cosine"), rep)
    assert evaluate_knn(m, cfg, train, test, k=5, num_labels=4, weights="distance", metric="euclidean").n_test == 32
    _, vcfg, vm = _vit_classifier("ref_vitcls_hd8")
    with pytest.raises(ValueError, match="ViTClassifier"):
        evaluate_knn(vm, vcfg, train, test)
    with pytest.raises(ValueError, match="model_arch"):
        evaluate_knn(m, {**cfg, "hyperparameters": {**cfg["hyperparameters"], "model_arch": "vit"}}, train, test)


def test_driver_reports_knn_accuracy(tmp_path):
    from vit_som_amd.train import main, synthetic_loaders
    _, cfg = load_golden("ref_cluster_tiny")
    cfg = copy.deepcopy(cfg)
    cfg["hyperparameters"]["batch_size"] = 16
    logs = []
    loaders = lambda c, r, w: synthetic_loaders(c, r, w, n_train=64, n_val=16, n_test=16)      # noqa: E731
    today = {"accuracy", "precision", "recall", "f1", "purity", "nmi", "run_duration", "inference_time"}
    met = main(cfg, n_runs=1, max_epochs=1, make_loaders=loaders, model_states_dir=str(tmp_path / "a"), log=logs.append)
    assert set(met) == today
    met = main(cfg, n_runs=1, max_epochs=1, make_loaders=loaders, model_states_dir=str(tmp_path / "b"), log=logs.append, knn_eval=True)
    assert set(met) == today | {"knn_accuracy"}
    (acc,) = met["knn_accuracy"]
    assert np.isfinite(acc) and 0.0 <= acc <= 1.0
    assert len(met["purity"]) == 1 and any("kNN probe: accuracy" in l for l in logs)


# ------------------------------------------------------------------ 10. two ranks
def _dp_loaders(cfg):
    """train: 12 batches of 10, test: 6 batches of 6 -- an even number of equal batches each, so both ranks fold alike."""
    return _split(cfg, 31, 4, 39, 120, 10, 6)


def _dp_worker(rank, world, port, out):
    import torch.distributed as dist
    from vit_som_amd.evaluation import evaluate_knn
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    m, cfg = _model("ref_cluster_tiny")
    m.world_size, m.rank = world, rank
    train, test = _dp_loaders(cfg)
    mine = lambda batches: [b for i, b in enumerate(batches) if i % world == rank]       # noqa: E731
    rep = evaluate_knn(m, cfg, mine(train), mine(test), k=10, num_labels=4, bank_rows=32)
    np.savez(f"{out}.{rank}.npz", confusion=rep.confusion, per_class=rep.per_class_accuracy,
             scalars=np.array([rep.accuracy, rep.n_train, rep.n_test, rep.k], dtype=np.float64))
    dist.barrier()
    dist.destroy_process_group()


def test_evaluate_knn_two_ranks(tmp_path):
    """Both ranks return the same report, and its confusion matrix is the single-process one on the same data (the
    features are random floats: no exact distance ties, so the ranks' different bank ordinals change nothing)."""
    from test_distributed import _free_port
    from vit_som_amd.evaluation import evaluate_knn
    out = str(tmp_path / "knn")
    mp.spawn(_dp_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    r0, r1 = np.load(f"{out}.0.npz"), np.load(f"{out}.1.npz")
    for key in ("confusion", "per_class", "scalars"):
        assert np.array_equal(r0[key], r1[key], equal_nan=True), key
    m, cfg = _model("ref_cluster_tiny")
    train, test = _dp_loaders(cfg)
    single = evaluate_knn(m, cfg, train, test, k=10, num_labels=4)
    assert np.array_equal(r0["confusion"], single.confusion) and r0["confusion"].sum() == 36
    assert r0["scalars"].tolist() == [single.accuracy, 120.0, 36.0, 10.0]
