"""UMAP.transform on the MI355X: the one-launch layout kernel (vsom_umap_transform_layout) against the numpy restatement
(umap_transform_ref.py) in slices, over a whole run under the edge rule of numeric_edges.py and on degenerate inputs;
UMAP.transform end to end on held-out blobs; visualize_umap_map and the fit_rows= subset fit on a tiny ViTSOM (one process
and two ranks)."""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import umap_transform_ref as R
from numeric_edges import E32_MAX, accepts, bound
from test_umap_gpu import _batches, _vitsom

pytestmark = pytest.mark.gpu

SEED = 0x1234_5678_9ABC_DEF1
ALPHA, GAMMA, RATE = 0.25, 1.0, 5


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _ab():
    from vit_som_amd.umap import find_ab_params
    return find_ab_params(1.0, 0.1)


def _kernel(idx, w, eps, Yt, n_epochs, e0, e1, Y=None, ws=None, seed=SEED):
    """One call of the entry -> (Y, ws, status[0]); Y and ws are created when not carried over from an earlier slice."""
    from vit_som_amd import ops
    a, b = _ab()
    M, k = idx.shape
    Y = torch.full((M, Yt.shape[1]), float("nan"), device="cuda") if Y is None else Y
    ws = ops.umap_transform_workspace(M, k, "cuda") if ws is None else ws
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.umap_transform_layout(_t(idx), _t(w), _t(eps), _t(Yt), Y, a, b, GAMMA, ALPHA, n_epochs, e0, e1, RATE, seed, status, ws)
    torch.cuda.synchronize()
    return Y, ws, int(status.item())


def _state(ws, M, k):
    from vit_som_amd import ops
    nxt, nxt_neg = ops.umap_transform_state(ws, M, k)
    return nxt.T.cpu().numpy(), nxt_neg.T.cpu().numpy()


def _ref(idx, w, eps, Yt, n_epochs, e0, e1, dtype=np.float64, seed=SEED, **kw):
    a, b = _ab()
    return R.layout(idx, w, eps, Yt, a, b, GAMMA, ALPHA, n_epochs, e0, e1, RATE, seed, dtype, **kw)


def _small(dim, k=8, N=80, M=70, n_epochs=30, seed=0):
    """M new points among N training points in 4-D, their exact kNN table and transform graph, a random training
    embedding in [0, 10]^dim."""
    from vit_som_amd.umap import transform_graph
    rng = np.random.default_rng(100 * dim + seed)
    train, new = rng.normal(size=(N, 4)), rng.normal(size=(M, 4))
    D = np.sqrt(((new[:, None, :] - train[None, :, :]) ** 2).sum(-1))
    idx = np.stack([np.lexsort((np.arange(N), D[i]))[:k] for i in range(M)]).astype(np.int64)
    dist = np.take_along_axis(D, idx, axis=1)
    w, eps = transform_graph(idx, dist, 1.0, n_epochs)
    Yt = rng.uniform(0.0, 10.0, size=(N, dim)).astype(np.float32)
    return idx, w, eps, Yt


# ------------------------------------------------------------------ the kernel in slices
@pytest.mark.parametrize("dim", [1, 2, 3, 4])
def test_layout_against_restatement_sliced(dim):
    """Two workgroups of 64, the second ragged; epochs [0, 6) of a 30-epoch schedule."""
    idx, w, eps, Yt = _small(dim)
    Y, ws, refused = _kernel(idx, w, eps, Yt, 30, 0, 6)
    ref, nxt, nxt_neg, attractions, repulsions = _ref(idx, w, eps, Yt, 30, 0, 6)
    assert refused == 0 and attractions > 0 and repulsions > 0
    got_nxt, got_neg = _state(ws, 70, 8)
    assert np.array_equal(got_nxt, nxt) and np.array_equal(got_neg, nxt_neg)
    assert (nxt != eps).any() and (nxt_neg != eps / RATE).any()
    got = Y.cpu().numpy()
    print(f"dim {dim}: max |kernel - fp64| {np.abs(got - ref).max():.3e} at scale {np.abs(ref).max():.3f}")
    assert np.allclose(got, ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max()), np.abs(got - ref).max()
    init, _, _ = _kernel(idx, w, eps, Yt, 30, 0, 0)                      # no epoch: the init alone, rounded once
    assert np.array_equal(init.cpu().numpy(), R.init(idx, w, eps, Yt, np.float32))


@pytest.mark.parametrize("dim", [2, 3])
def test_layout_chains_and_repeats(dim):
    from vit_som_amd import ops
    idx, w, eps, Yt = _small(dim)

    def same_state(ws_a, ws_b):                                          # the buffer's padding is not state
        return all(torch.equal(x, y) for x, y in zip(ops.umap_transform_state(ws_a, 70, 8), ops.umap_transform_state(ws_b, 70, 8)))
    Y, ws, _ = _kernel(idx, w, eps, Yt, 30, 0, 6)
    Y2, ws2, _ = _kernel(idx, w, eps, Yt, 30, 0, 6)
    assert torch.equal(Y, Y2) and same_state(ws, ws2)                    # two identical calls: the same bits
    Yc, wsc, _ = _kernel(idx, w, eps, Yt, 30, 0, 3)
    assert not torch.equal(Yc, Y) and not same_state(wsc, ws)
    Yc, wsc, _ = _kernel(idx, w, eps, Yt, 30, 3, 6, Y=Yc, ws=wsc)
    assert torch.equal(Yc, Y) and same_state(wsc, ws)                    # [0, 3) then [3, 6) is [0, 6)
    assert not torch.equal(_kernel(idx, w, eps, Yt, 30, 0, 6, seed=SEED + 1)[0], Y)


# ------------------------------------------------------------------ blobs: 2000 train the map, 200 are new
@pytest.fixture(scope="module")
def blobs():
    from sklearn.datasets import make_blobs
    from vit_som_amd import UMAP
    X, y = make_blobs(n_samples=2200, n_features=64, centers=8, cluster_std=1.0, center_box=(-20.0, 20.0), random_state=0)
    X = X.astype(np.float32)
    Xtr, Xnew = torch.from_numpy(X[:2000]).cuda(), torch.from_numpy(X[2000:]).cuda()
    m = UMAP(random_state=7)
    m.fit(Xtr)
    return dict(Xtr=Xtr, Xnew=Xnew, ytr=y[:2000], ynew=y[2000:], model=m, Yt=m.embedding_.cpu().numpy())


def _new_rows_graph(blobs, n_epochs):
    """The 200 held-out rows' kNN table (the device search) and transform graph."""
    from vit_som_amd import ops
    from vit_som_amd.umap import METRICS, transform_graph
    idx = torch.empty(200, 15, dtype=torch.int64, device="cuda")
    dist = torch.empty(200, 15, dtype=torch.float32, device="cuda")
    ops.knn_query(blobs["Xnew"], blobs["Xtr"], 15, METRICS["euclidean"], idx, dist)
    idx = idx.cpu().numpy()
    return (idx,) + transform_graph(idx, dist.cpu().numpy(), 1.0, n_epochs)


def test_whole_run_under_the_edge_rule(blobs):
    """All 30 epochs of 200 points: the kernel may be FACTOR times as far from the fp64 restatement as the float32
    restatement is, or within the sliced test's tolerance."""
    idx, w, eps = _new_rows_graph(blobs, 30)
    Yt = blobs["Yt"]
    ref, nxt, nxt_neg, attractions, repulsions = _ref(idx, w, eps, Yt, 30, 0, 30)
    y32 = _ref(idx, w, eps, Yt, 30, 0, 30, np.float32)[0]
    Y, ws, refused = _kernel(idx, w, eps, Yt, 30, 0, 30)
    got_nxt, got_neg = _state(ws, 200, 15)
    assert refused == 0 and np.array_equal(got_nxt, nxt) and np.array_equal(got_neg, nxt_neg)
    assert attractions > 200 and repulsions > 1000
    e32 = float(np.abs(y32.astype(np.float64) - ref).max())
    e_k = float(np.abs(Y.cpu().numpy().astype(np.float64) - ref).max())
    floor = 1e-5 * float(np.abs(ref).max())
    print(f"whole run: e_k {e_k:.3e}, e32 {e32:.3e}, floor {floor:.3e}, bound {bound(floor, e32):.3e}, scale {np.abs(ref).max():.3f}")
    assert e32 <= E32_MAX, e32                                           # otherwise the bound would be vacuous
    assert accepts(e_k, floor, e32), (e_k, e32, floor)


# ------------------------------------------------------------------ degenerate inputs
def test_single_point_and_extreme_k():
    for M, k, N in [(1, 8, 80), (70, 2, 80), (70, 64, 80)]:
        idx, w, eps, Yt = _small(2, k=k, N=N, M=M)
        Y, ws, refused = _kernel(idx, w, eps, Yt, 30, 0, 30)
        ref, nxt, nxt_neg, _, _ = _ref(idx, w, eps, Yt, 30, 0, 30)
        got_nxt, got_neg = _state(ws, M, k)
        assert refused == 0 and np.array_equal(got_nxt, nxt) and np.array_equal(got_neg, nxt_neg)
        e32 = float(np.abs(_ref(idx, w, eps, Yt, 30, 0, 30, np.float32)[0].astype(np.float64) - ref).max())
        e_k = float(np.abs(Y.cpu().numpy() - ref).max())
        assert e32 <= E32_MAX and accepts(e_k, 1e-5 * float(np.abs(ref).max()), e32), (M, k, e_k, e32)


def test_three_training_points_and_a_coincident_one():
    """N = 3: every negative sample is one of the point's own neighbours.  Row 0's only live edge has weight 1, so its
    init IS that training row (d2 = 0: the attraction adds nothing) until a repulsion from another row moves it."""
    from vit_som_amd.umap import transform_graph
    rng = np.random.default_rng(5)
    M, k, N = 70, 3, 3
    dist = np.sort(rng.uniform(0.5, 2.0, size=(M, k)), axis=1)
    idx = np.stack([rng.permutation(N) for _ in range(M)]).astype(np.int64)
    w, eps = transform_graph(idx, dist, 1.0, 30)
    w[0], eps[0] = [1.0, 0.0, 0.0], [1.0, np.inf, np.inf]
    Yt = rng.uniform(0.0, 10.0, size=(N, 2)).astype(np.float32)
    start, _, _ = _kernel(idx, w, eps, Yt, 30, 0, 0)
    assert torch.equal(start[0].cpu(), torch.from_numpy(Yt[idx[0, 0]]))  # the point coincides with a training row
    Y, ws, refused = _kernel(idx, w, eps, Yt, 30, 0, 30)
    ref, nxt, nxt_neg, _, repulsions = _ref(idx, w, eps, Yt, 30, 0, 30)
    got = Y.cpu().numpy()
    assert refused == 0 and np.isfinite(got).all() and repulsions > 0
    assert np.array_equal(_state(ws, M, k)[0], nxt) and np.array_equal(_state(ws, M, k)[1], nxt_neg)
    e32 = float(np.abs(_ref(idx, w, eps, Yt, 30, 0, 30, np.float32)[0].astype(np.float64) - ref).max())
    assert e32 <= E32_MAX and accepts(float(np.abs(got - ref).max()), 1e-5 * float(np.abs(ref).max()), e32)
    # one epoch moves a point by at most alpha * 4 per term and component: the clip's reach
    one, _, _ = _kernel(idx, w, eps, Yt, 30, 0, 2)
    terms = 1 + int(np.floor((1 - eps[0, 0] / RATE) / (eps[0, 0] / RATE)))
    assert np.abs(one[0].cpu().numpy() - Yt[idx[0, 0]]).max() <= ALPHA * 4.0 * terms


def test_all_but_one_edge_pruned():
    idx, w, eps, Yt = _small(2)
    eps[:, 1:] = np.inf
    eps[:, 0] = 1.0
    Y, ws, refused = _kernel(idx, w, eps, Yt, 30, 0, 6)
    ref, nxt, nxt_neg, attractions, _ = _ref(idx, w, eps, Yt, 30, 0, 6)
    got_nxt, got_neg = _state(ws, 70, 8)
    assert refused == 0 and attractions == 70 * 5                        # epochs 1 .. 5, one edge each
    assert np.array_equal(got_nxt, nxt) and np.array_equal(got_neg, nxt_neg)
    assert np.isinf(got_nxt[:, 1:]).all() and (got_nxt[:, 0] == 6.0).all()
    assert np.allclose(Y.cpu().numpy(), ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())


def test_refused_edges_are_counted_and_skipped():
    """Ordinals -1 and N, a NaN and a negative weight, a zero and a NaN eps: never followed, counted, and the other rows
    keep a clean run's bits."""
    idx, w, eps, Yt = _small(2)
    clean, ws_clean, refused = _kernel(idx, w, eps, Yt, 30, 0, 6)
    assert refused == 0
    bad_idx, bad_w, bad_eps = idx.copy(), w.copy(), eps.copy()
    bad_idx[3, 0], bad_idx[66, 7] = -1, 80
    Y, ws, refused = _kernel(bad_idx, bad_w, bad_eps, Yt, 30, 0, 6)
    assert refused == 2
    others = np.setdiff1d(np.arange(70), [3, 66])
    assert torch.equal(Y[others], clean[others]) and torch.isfinite(Y).all()
    ref, nxt, nxt_neg, _, _ = _ref(bad_idx, bad_w, bad_eps, Yt, 30, 0, 6)
    assert np.array_equal(_state(ws, 70, 8)[0], nxt) and np.isinf(nxt[3, 0]) and np.isinf(nxt[66, 7])
    assert np.allclose(Y.cpu().numpy(), ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())
    bad_w[10, 2], bad_w[11, 0], bad_eps[12, 1], bad_eps[13, 3] = np.nan, -0.5, 0.0, np.nan
    Y, ws, refused = _kernel(bad_idx, bad_w, bad_eps, Yt, 30, 0, 6)
    assert refused == 6 and torch.isfinite(Y).all()
    others = np.setdiff1d(others, [10, 11, 12, 13])
    assert torch.equal(Y[others], clean[others])


# ------------------------------------------------------------------ UMAP.transform end to end
def _vote_agreement(Y, Ytr, ytr, y, k=5):
    from sklearn.neighbors import NearestNeighbors
    ind = NearestNeighbors(n_neighbors=k).fit(Ytr).kneighbors(Y, return_distance=False)
    return float((np.array([np.bincount(v).argmax() for v in ytr[ind]]) == y).mean())


def test_transform_end_to_end(blobs):
    from vit_som_amd import UMAP
    m, Xtr, Xnew = blobs["model"], blobs["Xtr"], blobs["Xnew"]
    assert m._raw_data is Xtr and m.transform(Xtr) is m.embedding_
    Y = m.transform(Xnew)
    assert Y.shape == (200, 2) and Y.dtype == torch.float32 and Y.is_cuda and torch.isfinite(Y).all()
    assert torch.equal(m.transform(Xnew), Y)                             # does not depend on earlier calls
    m2 = UMAP(random_state=7)
    m2.fit(Xtr)
    assert torch.equal(m2.embedding_, m.embedding_) and torch.equal(m2.transform(Xnew), Y)
    one = m.transform(Xnew[:1].contiguous())                             # M = 1 (its graph has its own max(w))
    assert one.shape == (1, 2) and torch.isfinite(one).all()
    # the restatement at transform's own settings: 100 epochs, learning_rate / 4, the model's seed
    idx, w, eps = _new_rows_graph(blobs, 100)
    seed = int(np.frombuffer(np.random.RandomState(7).bytes(8), dtype="<u8")[0])
    ref = R.layout(idx, w, eps, blobs["Yt"], m._a, m._b, 1.0, 0.25, 100, 0, 100, 5, seed, np.float64)[0]
    got = Y.cpu().numpy()
    agree_ref = _vote_agreement(ref, blobs["Yt"], blobs["ytr"], blobs["ynew"])
    agree = _vote_agreement(got, blobs["Yt"], blobs["ytr"], blobs["ynew"])
    print(f"transform: 5-NN vote agreement {agree:.4f} (fp64 restatement {agree_ref:.4f}), max |diff| {np.abs(got - ref).max():.3e}")
    assert agree >= agree_ref, (agree, agree_ref)


# ------------------------------------------------------------------ evaluation
def _latents(m, cfg, batches):
    d = cfg["data"]
    lat = [m.get_latent_representation(x.cuda().reshape(-1, d["num_channels"], d["input_size"], d["input_size"]))
           .reshape(len(y), -1).float().clone() for x, y in batches]
    return torch.cat(lat).contiguous()


def test_visualize_umap_map(tmp_path):
    from vit_som_amd import visualize_umap_map
    m, cfg = _vitsom()
    batches = _batches(cfg)
    emb, labels, protos = visualize_umap_map(m, cfg, batches, epoch=3, output_dir=str(tmp_path))
    n, K = sum(len(y) for _, y in batches), m.som_layer.n_prototypes
    assert emb.shape == (n, 2) and labels.shape == (n,) and protos.shape == (K, 2)
    assert emb.dtype == np.float32 and protos.dtype == np.float32 and np.isfinite(emb).all() and np.isfinite(protos).all()
    assert np.array_equal(labels, np.concatenate([y.numpy() for _, y in batches]))
    try:
        import matplotlib  # noqa: F401
        assert os.path.getsize(tmp_path / "som_umap_map_epoch_3.png") > 0
    except ImportError:
        pass
    emb2, _, protos2 = visualize_umap_map(m, cfg, batches, epoch=4, output_dir=str(tmp_path))
    assert np.array_equal(emb, emb2) and np.array_equal(protos, protos2)

    class NoLatents:
        pass
    with pytest.raises(ValueError, match="visualize_umap_map: needs"):
        visualize_umap_map(NoLatents(), cfg, batches)


def test_fit_rows(tmp_path):
    from vit_som_amd import UMAP
    from vit_som_amd.evaluation import visualize_umap_progression
    m, cfg = _vitsom()
    batches = _batches(cfg)
    X = _latents(m, cfg, batches)
    N = X.shape[0]
    new = lambda: UMAP(n_neighbors=15, min_dist=0.1, metric="cosine", random_state=42)      # noqa: E731
    emb, _ = visualize_umap_progression(m, cfg, batches, output_dir=str(tmp_path), fit_rows=None)
    assert np.array_equal(emb, new().fit_transform(X).cpu().numpy())     # what it returned before the keyword existed
    assert np.array_equal(visualize_umap_progression(m, cfg, batches, output_dir=str(tmp_path), fit_rows=N)[0], emb)
    rows = 30
    assert 15 < rows < N
    emb, _ = visualize_umap_progression(m, cfg, batches, output_dir=str(tmp_path), fit_rows=rows)
    sub = np.sort(np.random.RandomState(42).permutation(N)[:rows])
    rest = np.setdiff1d(np.arange(N), sub)
    r = new()
    fitted = r.fit_transform(X[torch.from_numpy(sub).cuda()].contiguous())
    assert emb.shape == (N, 2) and np.array_equal(emb[sub], fitted.cpu().numpy())
    assert np.array_equal(emb[rest], r.transform(X[torch.from_numpy(rest).cuda()].contiguous()).cpu().numpy())


def _dp_worker(rank, world, port, out):
    import torch.distributed as dist
    from vit_som_amd import visualize_umap_map
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    m, cfg = _vitsom()
    m.world_size, m.rank = world, rank
    mine = [b for i, b in enumerate(_batches(cfg)) if i % world == rank]
    emb, labels, protos = visualize_umap_map(m, cfg, mine, output_dir=f"{out}_plots", fit_rows=30)
    np.savez(f"{out}.{rank}.npz", emb=emb, labels=labels, protos=protos)
    dist.barrier()
    dist.destroy_process_group()


def test_visualize_umap_map_two_ranks(tmp_path):
    from test_distributed import _free_port
    from vit_som_amd import visualize_umap_map
    out = str(tmp_path / "um")
    mp.spawn(_dp_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    r0, r1 = np.load(f"{out}.0.npz"), np.load(f"{out}.1.npz")
    assert all(np.array_equal(r0[key], r1[key]) for key in ("emb", "labels", "protos"))
    m, cfg = _vitsom()
    batches = _batches(cfg)
    order = [b for i, b in enumerate(batches) if i % 2 == 0] + [b for i, b in enumerate(batches) if i % 2 == 1]
    emb, labels, protos = visualize_umap_map(m, cfg, order, output_dir=str(tmp_path / "single"), fit_rows=30)
    assert all(np.array_equal(r0[key], val) for key, val in (("emb", emb), ("labels", labels), ("protos", protos)))
    assert emb.shape[0] == sum(len(y) for _, y in batches)
