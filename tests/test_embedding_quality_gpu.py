"""Trustworthiness / continuity on the MI355X: vsom_knn_ranks and embedding_quality.py against sklearn and the restatement
(embedding_quality_ref.py) on integer data where fp32 decides exactly, the bitwise threshold on real-valued data, massive
ties, fp64 where ties are not exact, the entry's conventions; evaluate_embedding_quality, map_neighbourhood and the driver
on the tiny fixtures."""
import copy

import numpy as np
import pytest
import torch

import embedding_quality_ref as R
from helpers import load_golden
from test_embedding_quality_cpu import fixture_a, rows_distinct

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COSINE, EUCLIDEAN = 0, 1                       # VSOM_DIST_*


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _ranks(A, nbr, metric, poison=-7):
    """One vsom_knn_ranks call into poisoned outputs (device tensors in, host int64 arrays out)."""
    from vit_som_amd import ops
    nbr = torch.as_tensor(nbr, dtype=torch.int64).to(DEV).contiguous()
    less = torch.full(nbr.shape, poison, dtype=torch.int32, device=DEV)
    tied = torch.full(nbr.shape, poison - 1, dtype=torch.int32, device=DEV)
    ops.knn_ranks(A, nbr, metric, less, tied)
    return less.cpu().numpy().astype(np.int64), tied.cpu().numpy().astype(np.int64)


def _own_neighbours(A, k, metric):
    """(idx [N, k + 1], dist [N, k + 1]) of vsom_umap_knn with the self column dropped: a row's k + 1 nearest other rows."""
    from vit_som_amd import ops
    N = A.shape[0]
    idx = torch.empty(N, k + 2, dtype=torch.int64, device=DEV)
    dist = torch.empty(N, k + 2, dtype=torch.float32, device=DEV)
    ops.umap_knn(A, k + 2, metric, idx, dist)
    assert torch.equal(idx[:, 0], torch.arange(N, device=DEV))
    return idx[:, 1:].cpu().numpy(), dist[:, 1:].cpu().numpy()


# ------------------------------------------------------------------ (a) exact against sklearn
def test_exact_against_sklearn_on_integer_data():
    """Dot products and norms are integers below 2^24, exact in fp32, and no two distances of a row coincide (asserted,
    also after the float32 square root): device and fp64 order every row identically, so the integer penalties are the
    restatement's and the two values sklearn's."""
    import sklearn.manifold as sk
    from vit_som_amd import EmbeddingQuality, continuity, embedding_quality, rank_penalties, trustworthiness
    X, E, k = fixture_a()
    N = X.shape[0]
    DX, DE = R.sq_distances(X), R.sq_distances(E)
    for D2 in (DX, DE):
        assert D2.max() < 2 ** 24 and rows_distinct(D2) and rows_distinct(np.sqrt(D2.astype(np.float64)).astype(np.float32))
    Xd, Ed = _dev(X), _dev(E)
    for A, B, DA, DB in ((Xd, Ed, DX, DE), (Ed, Xd, DE, DX)):
        pen = rank_penalties(A, B, k)
        nbr = R.neighbours(DB, k)
        less, tied = R.counts(DA, nbr)
        assert np.array_equal(pen.neighbours, nbr)
        assert np.array_equal(pen.less, less) and np.array_equal(pen.tied, tied) and not tied.any()
        want = R.penalties(less, tied, k)
        assert isinstance(pen.total, int) and pen.total == int(want.sum()) and np.array_equal(pen.per_row, want.astype(np.int64))
    t_sk = sk.trustworthiness(X.astype(np.float64), E.astype(np.float64), n_neighbors=k)
    c_sk = sk.trustworthiness(E.astype(np.float64), X.astype(np.float64), n_neighbors=k)
    assert t_sk == 0.6860484064222382 and c_sk == 0.7324610591900311
    t, c = trustworthiness(Xd, Ed, n_neighbors=k), continuity(Xd, Ed, n_neighbors=k)
    print(f"trustworthiness {t!r} (sklearn {t_sk!r}), continuity {c!r} (sklearn {c_sk!r})")
    assert abs(t - t_sk) <= 1e-12 and abs(c - c_sk) <= 1e-12
    for ties in ("max", "average"):
        assert trustworthiness(Xd, Ed, n_neighbors=k, ties=ties) == t
    q = embedding_quality(Xd, Ed, n_neighbors=k, metric="euclidean")
    assert isinstance(q, EmbeddingQuality) and (q.trustworthiness, q.continuity, q.n_neighbors, q.n_samples) == (t, c, k, N)
    assert q.trust_penalty == int(q.trust_per_row.sum()) and q.cont_penalty == int(q.cont_per_row.sum())
    with pytest.raises(ValueError, match=r"n_neighbors \(65\) should be less than n_samples / 2 \(65.0\)"):
        trustworthiness(Xd, Ed, n_neighbors=65)
    with pytest.raises(ValueError, match="limit of 63"):
        trustworthiness(Xd, Ed, n_neighbors=64)


# ------------------------------------------------------------------ (b) the bitwise threshold
@pytest.mark.parametrize("metric", [COSINE, EUCLIDEAN])
@pytest.mark.parametrize("N,D", [(257, 12288), (333, 1003), (130, 3)])
def test_own_neighbours_rank_themselves(N, D, metric):
    """A row's own k nearest rows (vsom_umap_knn), ranked in the same space: neighbour j has exactly j rows before it, less
    those of the list that lie at its own distance -- only if the threshold of a slot is bit for bit the distance the tile
    pass computes for that pair; and less + tied is what the list's runs of equal distances say.  No tolerance.
    (333, 1003) and (130, 3) take the element-wise loads (D % 4 != 0), (257, 12288) the 16-byte buffer loads."""
    k = 20
    A = _dev(np.random.default_rng(1).standard_normal((N, D)))
    idx, dist = _own_neighbours(A, k, metric)                     # k + 1 columns: one more than ranked
    less, tied = _ranks(A, idx[:, :k], metric)
    for j in range(k):
        before_equal = (dist[:, :j] == dist[:, j:j + 1]).sum(1)
        assert np.array_equal(less[:, j], j - before_equal), j
        run = (dist[:, :k] == dist[:, j:j + 1]).sum(1)            # the listed rows at this distance, itself included
        open_end = dist[:, k] == dist[:, j]                       # the run goes on past the list: only a lower bound
        assert (tied[:, j] >= run - 1).all() and np.array_equal(tied[~open_end, j], run[~open_end] - 1), j
    print(f"({N}, {D}) metric {metric}: slots with a tie {(tied > 0).mean():.4f}")


# ------------------------------------------------------------------ (c) ties
def test_massive_ties_equal_the_restatement():
    """E: the integer coordinates of a 25 x 28 grid (every distance many times over); X: small integer rows, some of them
    duplicated.  Neighbour lists, less and tied equal the restatement exactly in both directions, under all three policies."""
    from vit_som_amd import continuity, rank_penalties, trustworthiness
    rng = np.random.default_rng(7)
    E = np.stack(np.divmod(np.arange(700), 28), axis=1)
    X = rng.integers(0, 12, (700, 5))
    X[rng.choice(700, 60, replace=False)] = X[rng.choice(700, 60)]                   # duplicates
    DX, DE = R.sq_distances(X), R.sq_distances(E)
    assert (DX[~np.eye(700, dtype=bool)] == 0).any() and len(np.unique(DE)) < 1500
    k = 12
    Xd, Ed = _dev(X), _dev(E)
    for A, B, DA, DB in ((Xd, Ed, DX, DE), (Ed, Xd, DE, DX)):
        nbr = R.neighbours(DB, k)
        less, tied = R.counts(DA, nbr)
        assert tied.max() > 3
        for ties in R.TIES:
            pen = rank_penalties(A, B, k, ties=ties)
            assert np.array_equal(pen.neighbours, nbr) and np.array_equal(pen.less, less) and np.array_equal(pen.tied, tied)
            want = R.penalties(less, tied, k, ties)
            assert np.array_equal(np.asarray(pen.per_row, dtype=np.float64), want) and pen.total == want.sum(), ties
    lo, hi = trustworthiness(Xd, Ed, n_neighbors=k, ties="max"), trustworthiness(Xd, Ed, n_neighbors=k, ties="min")
    assert lo < trustworthiness(Xd, Ed, n_neighbors=k, ties="average") < hi
    assert continuity(Xd, Ed, n_neighbors=k, ties="min") == R.trustworthiness(DE, DX, k, "min")


# ------------------------------------------------------------------ (d) against fp64
def _compare_with_fp64(less, D64, tol, nbr, max_left_out):
    """less equals the fp64 count on every slot whose fp64 distance is further than the tolerance from every other of its
    row; elsewhere it is off by no more than the number of rows inside that window."""
    want, unsure = R.counts_with_window(D64, nbr, tol)
    valid = want >= 0
    clear = valid & (unsure == 0)
    assert np.array_equal(less[clear], want[clear])
    assert (np.abs(less - want)[valid] <= unsure[valid]).all()
    assert np.array_equal(less[~valid], want[~valid])
    left_out = 1.0 - clear.sum() / valid.sum()
    print(f"slots left out {left_out:.4f}, device != fp64 on {(less != want)[valid].mean():.4f}")
    assert left_out <= max_left_out, left_out


@pytest.mark.parametrize("metric", [COSINE, EUCLIDEAN])
def test_ranks_against_fp64(metric):
    """N(0,1) rows at (257, 12288), neighbour lists from a random 2-D embedding.  The tolerances are the project's for this
    contraction (test_knn_gpu.py::test_query_against_fp64): 1e-5 (|a|^2 + |b|^2) on the squared euclidean distance, 1e-5
    on the cosine distance.  No more than 30 % of the slots may need the window."""
    rng = np.random.default_rng(1)
    X = rng.standard_normal((257, 12288)).astype(np.float32)
    E = rng.standard_normal((257, 2))
    k = 15
    nbr = R.neighbours(np.sqrt(((E[:, None] - E[None]) ** 2).sum(-1)), k)
    Xd = X.astype(np.float64)
    sq = (Xd * Xd).sum(1)
    G = Xd @ Xd.T
    if metric == EUCLIDEAN:
        D64 = np.maximum(sq[:, None] + sq[None, :] - 2.0 * G, 0.0)           # squared: the same order
        tol = 1e-5 * (sq[:, None] + sq[None, :])
    else:
        D64 = 1.0 - G / np.sqrt(sq[:, None] * sq[None, :])
        tol = np.full_like(D64, 1e-5)
    less, _ = _ranks(torch.from_numpy(X).to(DEV), nbr, metric)
    _compare_with_fp64(less, D64, tol, nbr, 0.30)


# ------------------------------------------------------------------ (e) conventions
def _integer_case(N, D, k, hi, seed):
    """Integer rows and an arbitrary neighbour table with empty and self slots."""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, hi, (N, D))
    nbr = rng.integers(0, N, (N, k))
    nbr[rng.random((N, k)) < 0.05] = -1
    own = rng.random((N, k)) < 0.05
    nbr[own] = np.broadcast_to(np.arange(N)[:, None], (N, k))[own]
    return X, nbr


def test_conventions():
    from vit_som_amd import ops
    X, nbr = _integer_case(300, 6, 9, 16, 3)
    nbr[0, :3] = [-1, 0, 5]
    A = _dev(X)
    want = R.counts(R.sq_distances(X), nbr)
    less, tied = _ranks(A, nbr, EUCLIDEAN)
    assert less[0, 0] == tied[0, 0] == -1 and less[0, 1] == tied[0, 1] == -1 and less[0, 2] >= 0       # empty, self, a row
    assert ((nbr < 0) | (nbr == np.arange(300)[:, None])).sum() > 20
    assert np.array_equal(less, want[0]) and np.array_equal(tied, want[1])          # poisoned outputs fully overwritten
    again = _ranks(A, nbr, EUCLIDEAN, poison=-3)
    assert np.array_equal(again[0], less) and np.array_equal(again[1], tied)        # two calls are bit-identical
    wide = torch.full((300, 11), 1e30, device=DEV)                                   # lda = 11 > D = 6: the padding is never read
    wide[:, :6] = A
    strided = _ranks(wide[:, :6], nbr, EUCLIDEAN)
    assert np.array_equal(strided[0], less) and np.array_equal(strided[1], tied)
    for bad in (300, -2, 2 ** 40):
        table = torch.as_tensor(nbr).to(DEV)
        table[7, 4] = bad
        out = torch.zeros(300, 9, dtype=torch.int32, device=DEV)
        with pytest.raises(ValueError, match="outside"):
            ops.knn_ranks(A, table, EUCLIDEAN, out, out.clone())


@pytest.mark.parametrize("N,k", [(3000, 15), (4300, 6)])
def test_many_column_chunks_equal_the_restatement(N, k):
    """Several column chunks, combined by integer atomics: N = 3000 runs 47 chunks of one tile, N = 4300 is the first size
    range at which a chunk holds more than one tile (68 tiles in 61 chunks).  D = 8 takes the 16-byte loads."""
    X, nbr = _integer_case(N, 8, k, 32, N)
    want = R.counts(R.sq_distances(X), nbr)
    less, tied = _ranks(_dev(X), nbr, EUCLIDEAN)
    assert np.array_equal(less, want[0]) and np.array_equal(tied, want[1])
    assert want[1].max() > 10


# ------------------------------------------------------------------ (f) the evaluation path
@pytest.mark.parametrize("name", ["ref_cluster_tiny", "ref_cls_tiny"])
def test_evaluate_embedding_quality_on_the_tiny_fixtures(name):
    from test_knn_gpu import _features, _loaders, _model
    from vit_som_amd import EmbeddingQuality, EmbeddingQualityReport, continuity, trustworthiness
    from vit_som_amd.evaluation import evaluate_embedding_quality
    m, cfg = _model(name)
    train, _ = _loaders(cfg, 4)                                    # 96 samples in batches of 10
    rep = evaluate_embedding_quality(m, cfg, train)
    assert isinstance(rep, EmbeddingQualityReport) and isinstance(rep, EmbeddingQuality)
    assert (rep.n_samples, rep.n_neighbors) == (96, 15) and rep.fitted_rows is None and rep.fitted is None
    assert rep.embedding.shape == (96, 2) and rep.embedding.dtype == np.float32 and np.isfinite(rep.embedding).all()
    assert 0.0 <= rep.trustworthiness <= 1.0 and 0.0 <= rep.continuity <= 1.0
    X, _ = _features(m, cfg, train)
    E = torch.from_numpy(rep.embedding).to(DEV)
    assert rep.trustworthiness == trustworthiness(X, E, n_neighbors=15, metric="cosine")
    assert rep.continuity == continuity(X, E, n_neighbors=15, metric="cosine")
    assert rep.trust_per_row.shape == (96,) and rep.trust_penalty == int(rep.trust_per_row.sum())
    if name == "ref_cluster_tiny":
        sub = evaluate_embedding_quality(m, cfg, train, n_neighbors=10, fit_rows=64)
        assert sub.fitted_rows.dtype == bool and sub.fitted_rows.sum() == 64 and sub.n_neighbors == 10
        E = torch.from_numpy(sub.embedding).to(DEV)
        assert sub.trustworthiness == trustworthiness(X, E, n_neighbors=10, metric="cosine")
        # the two parts are the whole: penalties add up, each part normalised by its own row count
        for whole, part_f, part_t in ((sub.trustworthiness, sub.fitted[0], sub.transformed[0]),
                                      (sub.continuity, sub.fitted[1], sub.transformed[1])):
            assert abs(96 * (1 - whole) - 64 * (1 - part_f) - 32 * (1 - part_t)) <= 1e-9
    with pytest.raises(ValueError, match="model_arch"):
        evaluate_embedding_quality(m, {**cfg, "hyperparameters": {**cfg["hyperparameters"], "model_arch": "vit"}}, train)


def _dp_worker(rank, world, port, out):
    import torch.distributed as dist
    from test_knn_gpu import _loaders, _model
    from vit_som_amd.evaluation import evaluate_embedding_quality
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    m, cfg = _model("ref_cluster_tiny")
    m.world_size, m.rank = world, rank
    train, _ = _loaders(cfg, 4)
    rep = evaluate_embedding_quality(m, cfg, [b for i, b in enumerate(train) if i % world == rank])
    np.savez(f"{out}.{rank}.npz", embedding=rep.embedding, trust=rep.trust_per_row, cont=rep.cont_per_row,
             scalars=np.array([rep.trustworthiness, rep.continuity, rep.n_samples], dtype=np.float64))
    dist.barrier()
    dist.destroy_process_group()


def test_evaluate_embedding_quality_two_ranks(tmp_path):
    """Both ranks gather all rows (50 + 46, rank 0's first) and return the same report: that of one process over the rows
    in that order."""
    import torch.multiprocessing as mp
    from test_distributed import _free_port
    from test_knn_gpu import _loaders, _model
    from vit_som_amd.evaluation import evaluate_embedding_quality
    out = str(tmp_path / "eq")
    mp.spawn(_dp_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    r0, r1 = np.load(f"{out}.0.npz"), np.load(f"{out}.1.npz")
    for key in ("embedding", "trust", "cont", "scalars"):
        assert np.array_equal(r0[key], r1[key]), key
    m, cfg = _model("ref_cluster_tiny")
    train, _ = _loaders(cfg, 4)
    single = evaluate_embedding_quality(m, cfg, train[0::2] + train[1::2])
    assert r0["scalars"].tolist() == [single.trustworthiness, single.continuity, 96.0]
    assert np.array_equal(r0["trust"], single.trust_per_row) and np.array_equal(r0["embedding"], single.embedding)


@pytest.mark.parametrize("name", ["ref_hexa_euclid_tiny", "ref_cluster_tiny"])
def test_map_neighbourhood_equals_the_restatement(name):
    """The hexagonal (euclidean) and a square (cosine) map: ranks of the grid neighbours among the prototypes against fp64
    on the prototypes copied to the host, with the window rule of test_ranks_against_fp64 should two distances nearly
    coincide."""
    import knn_ref
    from test_knn_gpu import _model
    from vit_som_amd import MapNeighbourhood
    from vit_som_amd.evaluation import map_neighbourhood, umatrix
    m, cfg = _model(name)
    som = m.som_layer
    assert som.topology == ("hexa" if "hexa" in name else som.topology)
    got = map_neighbourhood(m)
    assert isinstance(got, MapNeighbourhood)
    nbr = umatrix(m)[1]
    assert np.array_equal(got.neighbours, nbr) and got.ranks.shape == nbr.shape
    W = som.prototypes.detach().float().cpu().numpy().astype(np.float64)
    sq = (W * W).sum(1)
    if som._dist_mode == EUCLIDEAN:
        D64 = np.maximum(sq[:, None] + sq[None, :] - 2.0 * (W @ W.T), 0.0)
        tol = 1e-5 * (sq[:, None] + sq[None, :])
    else:
        assert som._dist_mode == COSINE
        D64 = knn_ref.distances(W, W, knn_ref.COSINE)
        tol = np.full_like(D64, 1e-5)
    valid = nbr >= 0
    assert np.array_equal(got.ranks >= 1, valid) and (got.ranks[~valid] == -1).all()
    _compare_with_fp64(np.where(valid, got.ranks - 1, -1), D64, tol, nbr.astype(np.int64), 0.30)
    deg = valid.sum(1, keepdims=True)
    assert got.mean_rank == got.ranks[valid].sum() / valid.sum()
    assert got.within_degree == (valid & (got.ranks <= deg)).sum() / valid.sum()
    assert 1.0 <= got.mean_rank <= som.n_prototypes - 1 and 0.0 <= got.within_degree <= 1.0


def test_driver_reports_trustworthiness_and_continuity(tmp_path):
    from vit_som_amd.train import main, synthetic_loaders
    _, cfg = load_golden("ref_cluster_tiny")
    cfg = copy.deepcopy(cfg)
    cfg["hyperparameters"]["batch_size"] = 16
    logs = []
    loaders = lambda c, r, w: synthetic_loaders(c, r, w, n_train=64, n_val=16, n_test=16)      # noqa: E731
    today = {"accuracy", "precision", "recall", "f1", "purity", "nmi", "run_duration", "inference_time"}
    met = main(cfg, n_runs=1, max_epochs=1, make_loaders=loaders, model_states_dir=str(tmp_path / "a"), log=logs.append,
               embedding_quality=True)
    assert set(met) == today | {"trustworthiness", "continuity"}
    (t,), (c,) = met["trustworthiness"], met["continuity"]
    assert 0.0 <= t <= 1.0 and 0.0 <= c <= 1.0
    assert any("Embedding quality: trustworthiness" in l for l in logs)
