"""UMAP on the MI355X: the kNN kernel against an fp64 brute force, one layout epoch against the numpy restatement of
step 8 (vit_som_amd/umap.py), whole fits (reproducibility, both inits, quality on blobs) and
visualize_umap_progression on a tiny ViTSOM (one process and two ranks)."""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from test_umap_cpu import knn_table, neg_sample

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ kNN
def _knn_data(N, D, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(N, 6, generator=g) @ torch.randn(6, D, generator=g) + 0.05 * torch.randn(N, D, generator=g)
    X[5] = X[3]                                  # duplicates of row 3
    X[N // 2] = X[3]
    X[7] = 0.0                                   # a zero row
    return X


def _ref_dist(Xd, sq, rows, cols, metric):
    """fp64 distance (euclidean: squared) between rows[i] and every cols[i, :] (device tensors)."""
    diff = Xd[rows][:, None, :] - Xd[cols]
    if metric == "euclidean":
        return (diff * diff).sum(-1)
    nrm = sq.sqrt()
    dot = (Xd[rows][:, None, :] * Xd[cols]).sum(-1)
    ni, nj = nrm[rows][:, None], nrm[cols]
    d = 1.0 - dot / (ni * nj)
    d = torch.where((ni == 0) & (nj == 0), torch.zeros_like(d), d)
    return torch.where((ni == 0) ^ (nj == 0), torch.ones_like(d), d)


def _ref_sorted(Xd, sq, r0, r1, k, metric):
    """fp64 distances of rows r0..r1 to all rows, the k + 1 smallest in order (euclidean: squared), self first."""
    G = Xd[r0:r1] @ Xd.T
    if metric == "euclidean":
        dist = (sq[r0:r1, None] + sq[None, :] - 2.0 * G).clamp_min(0.0)
    else:
        nrm = sq.sqrt()
        ni, nj = nrm[r0:r1, None], nrm[None, :]
        dist = 1.0 - G / (ni * nj)
        dist = torch.where((ni == 0) & (nj == 0), torch.zeros_like(dist), dist)
        dist = torch.where((ni == 0) ^ (nj == 0), torch.ones_like(dist), dist)
    ar = torch.arange(r0, r1, device=Xd.device)
    dist[ar - r0, ar] = -1.0
    return torch.topk(dist, k + 1, largest=False, sorted=True)


KNN_CASES = [(257, 3, 2), (257, 1003, 64), (257, 3136, 15), (3000, 64, 15), (3000, 3136, 64), (3000, 3, 64),
             (20011, 64, 2), (20011, 3136, 15), (20011, 1003, 64)]


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("N,D,k", KNN_CASES)
def test_knn_against_fp64(N, D, k, metric):
    from vit_som_amd import ops
    from vit_som_amd.umap import METRICS
    X = _knn_data(N, D, N + D + k).cuda()
    idx = torch.empty(N, k, dtype=torch.int64, device="cuda")
    dist = torch.empty(N, k, dtype=torch.float32, device="cuda")
    ops.umap_knn(X, k, METRICS[metric], idx, dist)
    idx2, dist2 = torch.full_like(idx, -1), torch.full_like(dist, -1.0)
    ops.umap_knn(X, k, METRICS[metric], idx2, dist2)
    torch.cuda.synchronize()
    assert torch.equal(idx, idx2) and torch.equal(dist, dist2)               # bitwise reproducible
    ar = torch.arange(N, device="cuda")
    assert torch.equal(idx[:, 0], ar) and (dist[:, 0] == 0).all()           # the row itself first, at 0
    assert ((idx >= 0) & (idx < N)).all()
    assert (dist[:, 1:] >= dist[:, :-1]).all()
    # duplicates follow the row at distance exactly 0, lower index first
    assert idx[3, :3].tolist() == [3, 5, N // 2][:k] and (dist[3, :3] == 0).all()
    assert idx[5, :3].tolist() == [5, 3, N // 2][:k]
    if metric == "cosine":                                                   # zero row: every other row at 1
        assert (dist[7, 1:] == 1).all() and idx[7, 1:].tolist() == [j for j in range(k) if j != 7][:k - 1]

    Xd = X.double()
    sq = (Xd * Xd).sum(1)
    checked = 0
    for r0 in range(0, N, 512):
        r1 = min(N, r0 + 512)
        rows = torch.arange(r0, r1, device="cuda")
        mine = _ref_dist(Xd, sq, rows, idx[r0:r1], metric)                   # exact distance of what the kernel chose
        got = dist[r0:r1].double()
        if metric == "euclidean":
            tol = 1e-5 * (sq[rows][:, None] + sq[idx[r0:r1]])
            assert ((got * got - mine).abs() <= tol).all()
        else:
            assert ((got - mine).abs() <= 1e-5).all()
        rv, ri = _ref_sorted(Xd, sq, r0, r1, k, metric)
        rv[:, 0] = 0.0
        if metric == "euclidean":
            sqj = sq[ri]
            gap_tol = 1e-5 * (sq[rows][:, None] + torch.maximum(sqj[:, 1:], sqj[:, :-1]))
        else:
            gap_tol = torch.full_like(rv[:, 1:], 1e-5)
        clear = ((rv[:, 1:] - rv[:, :-1]) > gap_tol).all(dim=1)
        clear &= (rows != 3) & (rows != 5) & (rows != N // 2) & (rows != 7)
        assert torch.equal(idx[r0:r1][clear], ri[clear, :k])
        checked += int(clear.sum())
    assert checked >= N // 4, checked


def test_knn_rejects_what_it_does_not_cover():
    from vit_som_amd import UMAP
    X = torch.randn(100, 8, device="cuda")
    with pytest.raises(ValueError, match="contiguous"):
        UMAP().fit(X[:, ::2])
    with pytest.raises(ValueError, match="exceed"):
        UMAP(n_neighbors=15).fit(X[:15])
    with pytest.raises(ValueError, match="init"):
        UMAP(init=np.zeros((99, 2))).fit(X)


# ------------------------------------------------------------------ one epoch
def ref_epoch(indptr, indices, eps, nxt, eps_neg, nxt_neg, Y, a, b, gamma, alpha, n, seed):
    """Step 8 for epoch n (float64): every term reads Y, the attraction counts twice; returns (Y', next, next_neg)."""
    N, dim = Y.shape
    out, nxt, nxt_neg = Y.copy(), nxt.copy(), nxt_neg.copy()
    for v in range(N):
        acc = np.zeros(dim)
        for e in range(indptr[v], indptr[v + 1]):
            if nxt[e] > n:
                continue
            diff = Y[v] - Y[indices[e]]
            d2 = (diff * diff).sum()
            c = (-2.0 * a * b * d2 ** (b - 1.0)) / (a * d2 ** b + 1.0) if d2 > 0.0 else 0.0
            g = np.clip(c * diff, -4.0, 4.0)
            acc += g
            acc += g
            nxt[e] = nxt[e] + eps[e]
            n_neg = int(np.floor((n - nxt_neg[e]) / eps_neg[e]))
            for p in range(n_neg):
                diff = Y[v] - Y[neg_sample(seed, n, e, p, N)]
                d2 = (diff * diff).sum()
                if not d2 > 0.0:
                    continue
                c = 2.0 * gamma * b / ((0.001 + d2) * (a * d2 ** b + 1.0))
                acc += np.clip(c * diff, -4.0, 4.0)
            nxt_neg[e] = nxt_neg[e] + n_neg * eps_neg[e]
        out[v] = Y[v] + alpha * acc
    return out, nxt, nxt_neg


@pytest.mark.parametrize("dim", [2, 3])
def test_epoch_against_restatement(dim):
    from vit_som_amd import ops
    from vit_som_amd.umap import find_ab_params, fuzzy_simplicial_set, make_schedule
    rng = np.random.default_rng(dim)
    pts = rng.normal(size=(80, 4))
    idx, dist = knn_table(pts, 8)
    G = fuzzy_simplicial_set(idx, dist, 1.0, 1.0)[0].astype(np.float32)
    n_epochs = 30
    P, eps, eps_neg = make_schedule(G, n_epochs, 5)
    a, b = find_ab_params(1.0, 0.1)
    gamma, seed = 1.0, 0x1234_5678_9ABC_DEF1
    Y = rng.uniform(0.0, 10.0, size=(80, dim)).astype(np.float32)
    indptr, indices = P.indptr.astype(np.int64), P.indices.astype(np.int64)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()      # noqa: E731
    dptr, dind, deps, deps_neg = t(indptr), t(indices), t(eps), t(eps_neg)
    dnxt, dnxt_neg = deps.clone(), deps_neg.clone()
    nxt, nxt_neg = eps.copy(), eps_neg.copy()
    Yin, Yout = t(Y), torch.empty(80, dim, dtype=torch.float32, device="cuda")
    sampled = repelled = 0
    for n in range(6):
        alpha = 1.0 if n == 0 else 1.0 * (1.0 - (n - 1) / n_epochs)
        ops.umap_epoch(dptr, dind, deps, dnxt, deps_neg, dnxt_neg, Yin, Yout, a, b, gamma, alpha, n, seed)
        yin = Yin.cpu().numpy().astype(np.float64)
        ref, nxt_new, nxt_neg_new = ref_epoch(indptr, indices, eps, nxt, eps_neg, nxt_neg, yin, a, b, gamma, alpha, n, seed)
        sampled += int((nxt_new != nxt).sum())
        repelled += int((nxt_neg_new != nxt_neg).sum())
        nxt, nxt_neg = nxt_new, nxt_neg_new
        got = Yout.cpu().numpy()
        assert np.array_equal(dnxt.cpu().numpy(), nxt) and np.array_equal(dnxt_neg.cpu().numpy(), nxt_neg)
        assert np.allclose(got, ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max()), np.abs(got - ref).max()
        if n == 0:
            assert np.array_equal(got, Y)                                    # epoch 0 samples nothing
        Yin, Yout = Yout, Yin
    assert sampled > 0 and repelled > 0


# ------------------------------------------------------------------ whole fits
def _blobs(n=2000, d=64, k=8, seed=0):
    from sklearn.datasets import make_blobs
    X, y = make_blobs(n_samples=n, n_features=d, centers=k, cluster_std=1.0, center_box=(-20.0, 20.0), random_state=seed)
    return X.astype(np.float32), y


def _loo_knn_agreement(Y, y, k=5):
    from sklearn.neighbors import NearestNeighbors
    ind = NearestNeighbors(n_neighbors=k + 1).fit(Y).kneighbors(Y, return_distance=False)[:, 1:]
    votes = y[ind]
    pred = np.array([np.bincount(v).argmax() for v in votes])
    return float((pred == y).mean())


@pytest.fixture(scope="module")
def blob_fit():
    from vit_som_amd import UMAP
    X, y = _blobs()
    Xd = torch.from_numpy(X).cuda()
    m = UMAP(random_state=7)
    return X, y, Xd, m, m.fit_transform(Xd)


def test_fit_is_reproducible(blob_fit):
    from vit_som_amd import UMAP
    X, y, Xd, m, Y = blob_fit
    assert Y.shape == (2000, 2) and Y.dtype == torch.float32 and Y.is_cuda and torch.isfinite(Y).all()
    assert torch.equal(UMAP(random_state=7).fit_transform(Xd), Y)
    assert not torch.equal(UMAP(random_state=8).fit_transform(Xd), Y)
    import scipy.sparse
    assert isinstance(m.graph_, scipy.sparse.csr_matrix) and m.graph_.dtype == np.float32 and m.graph_.shape == (2000, 2000)
    assert abs(m._a - 1.57694346) < 1e-6 and abs(m._b - 0.89506088) < 1e-6


def test_blobs_layout_quality(blob_fit):
    from sklearn.manifold import trustworthiness
    X, y, Xd, m, Y = blob_fit
    Yh = Y.cpu().numpy()
    tw, agree = trustworthiness(X, Yh, n_neighbors=5), _loo_knn_agreement(Yh, y)
    print(f"blobs: trustworthiness {tw:.4f}, 5-NN agreement {agree:.4f}")
    assert tw >= 0.93 and agree >= 0.99, (tw, agree)            # first run on an MI355X: 0.9498, 1.0


@pytest.mark.parametrize("init", ["spectral", "random"])
@pytest.mark.parametrize("dim,metric", [(2, "cosine"), (3, "euclidean")])
def test_inits_dims_metrics(init, dim, metric):
    """8 separated blobs of 60 points, n_neighbors=10: 8 > 2 dim components (PCA meta-positions)."""
    from sklearn.manifold import trustworthiness
    from vit_som_amd import UMAP
    X, y = _blobs(n=480, d=32, seed=3)
    m = UMAP(n_neighbors=10, n_components=dim, metric=metric, init=init, random_state=1)
    Y = m.fit_transform(torch.from_numpy(X).cuda())
    import scipy.sparse.csgraph
    assert scipy.sparse.csgraph.connected_components(m.graph_)[0] > 2 * dim
    Yh = Y.cpu().numpy()
    assert Yh.shape == (480, dim) and np.isfinite(Yh).all()
    tw, agree = trustworthiness(X, Yh, n_neighbors=5), _loo_knn_agreement(Yh, y)
    print(f"{init} dim={dim} {metric}: trustworthiness {tw:.4f}, 5-NN agreement {agree:.4f}")
    assert tw >= 0.94 and agree >= 0.99, (tw, agree)            # first run: 0.968 - 0.976, 1.0


def test_init_array_is_used():
    from vit_som_amd import UMAP
    X, _ = _blobs(n=300, d=16, seed=5)
    Xd = torch.from_numpy(X).cuda()
    init = np.random.default_rng(0).normal(size=(300, 2))
    a = UMAP(init=init, random_state=0, n_epochs=1).fit_transform(Xd).cpu().numpy()     # epoch 0 moves nothing
    ref = 10.0 * (init - init.min(0)) / (init.max(0) - init.min(0))
    assert np.allclose(a, ref.astype(np.float32), rtol=0, atol=1e-5)


# ------------------------------------------------------------------ visualize_umap_progression
def _vitsom():
    import copy
    import vit_som_amd
    from helpers import golden_params, load_golden
    z, cfg = load_golden("ref_cluster_tiny")
    m = vit_som_amd.ViTSOM(copy.deepcopy(cfg), device="cuda:0")
    m.load_state_dict(golden_params(z))
    return m, cfg


def _batches(cfg):
    from test_kmeans_gpu import _separable_images
    d = cfg["data"]
    return _separable_images(9, 12, 4, d["num_channels"], d["input_size"], 8)


def test_visualize_umap_progression(tmp_path):
    from vit_som_amd.evaluation import visualize_umap_progression
    m, cfg = _vitsom()
    batches = _batches(cfg)
    emb, labels = visualize_umap_progression(m, cfg, batches, epoch=3, output_dir=str(tmp_path))
    n = sum(len(y) for _, y in batches)
    assert emb.shape == (n, 2) and emb.dtype == np.float32 and np.isfinite(emb).all()
    assert np.array_equal(labels, np.concatenate([y.numpy() for _, y in batches]))
    try:
        import matplotlib  # noqa: F401
        assert os.path.getsize(tmp_path / "som_umap_epoch_3.png") > 0
    except ImportError:
        pass
    emb2, _ = visualize_umap_progression(m, cfg, batches, epoch=4, output_dir=str(tmp_path))
    assert np.array_equal(emb, emb2)


def _dp_worker(rank, world, port, out):
    import torch.distributed as dist
    from vit_som_amd.evaluation import visualize_umap_progression
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    m, cfg = _vitsom()
    m.world_size, m.rank = world, rank
    mine = [b for i, b in enumerate(_batches(cfg)) if i % world == rank]
    emb, labels = visualize_umap_progression(m, cfg, mine, output_dir=f"{out}_plots")
    np.savez(f"{out}.{rank}.npz", emb=emb, labels=labels)
    dist.barrier()
    dist.destroy_process_group()


def test_visualize_umap_progression_two_ranks(tmp_path):
    from test_distributed import _free_port
    from vit_som_amd.evaluation import visualize_umap_progression
    out = str(tmp_path / "um")
    mp.spawn(_dp_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    r0, r1 = np.load(f"{out}.0.npz"), np.load(f"{out}.1.npz")
    assert np.array_equal(r0["emb"], r1["emb"]) and np.array_equal(r0["labels"], r1["labels"])
    m, cfg = _vitsom()
    batches = _batches(cfg)
    order = [b for i, b in enumerate(batches) if i % 2 == 0] + [b for i, b in enumerate(batches) if i % 2 == 1]
    emb, labels = visualize_umap_progression(m, cfg, order, output_dir=str(tmp_path / "single"))
    assert np.array_equal(r0["emb"], emb) and np.array_equal(r0["labels"], labels)
    assert emb.shape[0] == sum(len(y) for _, y in batches)
