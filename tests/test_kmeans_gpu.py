"""k-means for evaluate_kmeans on the MI355X: the assign / update kernels against the float64 oracle of
test_kmeans_cpu.py, the Lloyd loop, k-means++ and the full fit against sklearn, and evaluate_kmeans on ViTSOM / DESOM
(one process and two ranks)."""
import copy

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from helpers import golden_params, load_golden
from test_kmeans_cpu import assign_oracle, average_centers, donor_case, lloyd_oracle, sums_counts

pytestmark = pytest.mark.gpu


def _data(seed, N, D, k, dup=False):
    g = torch.Generator().manual_seed(seed)
    means = torch.randn(k, D, generator=g) * 2.0
    X = means[torch.randint(0, k, (N,), generator=g)] + torch.randn(N, D, generator=g)
    if dup:
        X[N // 2:N // 2 + 50] = X[:50]
    C = X[torch.randperm(N, generator=g)[:k]].clone()
    return X, C


def _one_iteration(X, C, prev, alias=False):
    """assign + update on the device -> (labels, mind, centres_new, counts, status).  alias: one buffer is both
    prev_labels and labels (the header allows it)."""
    from vit_som_amd import ops
    N, D = X.shape
    k = C.shape[0]
    ws = torch.empty(ops.kmeans_workspace_bytes(N, D, k), dtype=torch.uint8, device="cuda")
    labels = prev.clone() if alias else torch.empty(N, dtype=torch.int64, device="cuda")
    mind = torch.empty(N, dtype=torch.float32, device="cuda")
    cnew = torch.empty(k, D, dtype=torch.float32, device="cuda")
    counts = torch.empty(k, dtype=torch.int64, device="cuda")
    status = torch.empty(4, dtype=torch.float64, device="cuda")
    ops.kmeans_assign(X, C, labels, labels if alias else prev, mind, ws)
    ops.kmeans_update(C, cnew, N, mind, counts, status, ws)
    torch.cuda.synchronize()
    return labels.cpu().numpy(), mind.cpu().numpy(), cnew.cpu().numpy(), counts.cpu().numpy(), status.cpu().numpy()


def _check_iteration(Xh, Ch, prev_h, out, min_clear=0.0):
    labels, mind, cnew, counts, status = out
    k = Ch.shape[0]
    ref_l, ref_m, gap = assign_oracle(Xh, Ch)
    clear = gap > 1e-4 * np.maximum(ref_m, 1e-30)
    assert clear.mean() >= min_clear, clear.mean()                          # a few rows: the label check must not be empty
    assert np.array_equal(labels[clear], ref_l[clear]), int((labels[clear] != ref_l[clear]).sum())
    # mind: the distance to the centre the kernel chose
    own = ((Xh.astype(np.float64) - Ch.astype(np.float64)[labels]) ** 2).sum(axis=1)
    assert np.allclose(mind, own, rtol=1e-5, atol=1e-5 * own.max())
    sums, cnt = sums_counts(Xh, labels, k)
    assert np.array_equal(counts, cnt)
    ref_c = average_centers(sums, cnt)
    assert np.allclose(cnew, ref_c, rtol=1e-5, atol=1e-5 * np.abs(ref_c).max())
    assert int(status[0]) == int((labels != prev_h).sum())                  # changed count: exact
    assert int(status[2]) == int((cnt == 0).sum())
    assert abs(status[3] - own.sum()) <= 1e-5 * own.sum() + 1e-30
    shift = ((cnew.astype(np.float64) - Ch.astype(np.float64)) ** 2).sum()
    assert abs(status[1] - shift) <= 1e-9 * max(shift, 1.0)


# small shapes on the tiled pass's other paths: fewer rows than one step (one workgroup, 4 centres to a chunk, 16-byte
# loads); element loads with 12 centres to a chunk; element loads with 16 to a chunk, two D-tiles and ragged 17 / 16-row
# workgroups; 16-byte loads with two D-tiles
_SMALL = [(5, 8, 3), (70, 7, 11), (33, 2310, 13), (40, 2400, 16)]


@pytest.mark.parametrize("N,D,k,alias", [(50000, 3072, 10, False), (2000, 784, 10, False), (1000, 12288, 200, False),
                                         (777, 10, 7, False), (1001, 37, 1, False), (2000, 784, 10, True), (777, 10, 7, True)]
                         + [s + (False,) for s in _SMALL])
def test_assign_update_against_oracle(N, D, k, alias):
    X, C = _data(N + D + k, N, D, k)
    prev = torch.randint(-1, k, (N,), generator=torch.Generator().manual_seed(1))
    out = _one_iteration(X.cuda(), C.cuda(), prev.cuda(), alias=alias)
    _check_iteration(X.numpy(), C.numpy(), prev.numpy(), out, min_clear=0.9 if (N, D, k) in _SMALL else 0.0)


def test_assign_strided_ties_and_duplicates():
    N, D, k = 3000, 96, 6
    X, C = _data(7, N, D, k, dup=True)
    big = torch.zeros(N, D + 5)
    big[:, :D] = X
    big[:, D:] = float("nan")                               # padding columns must never be read
    Xs = big.cuda()[:, :D]
    assert Xs.stride(0) == D + 5
    prev = torch.full((N,), -1, dtype=torch.int64)
    out = _one_iteration(Xs, C.cuda(), prev.cuda())
    _check_iteration(X.numpy(), C.numpy(), prev.numpy(), out)
    # exact ties: two equal centres -> the lower index wins for every row
    C2 = torch.cat([C[:1], C[:1], C[1:]])
    labels = _one_iteration(X.cuda(), C2.cuda(), prev.cuda())[0]
    ref = assign_oracle(X.numpy(), C2.numpy())[0]
    assert not (labels == 1).any() and np.array_equal(labels[ref != 0], ref[ref != 0])
    # odd D and unaligned rows (scalar path): same checks
    Xo = torch.zeros(N, 33)
    Xo[:, :31] = X[:, :31]
    Xu = Xo.cuda()[:, 1:32]
    out = _one_iteration(Xu, Xu[:k].clone(), prev.cuda())
    _check_iteration(Xo[:, 1:32].numpy(), Xo[:k, 1:32].numpy(), prev.numpy(), out)


def test_fit_is_deterministic():
    from vit_som_amd import KMeans
    X, _ = _data(11, 20000, 256, 10)
    X = X.cuda()
    a = KMeans(10, n_init=3, random_state=0).fit(X)
    b = KMeans(10, n_init=3, random_state=0).fit(X)
    assert torch.equal(a.cluster_centers_, b.cluster_centers_) and torch.equal(a.labels_, b.labels_)
    assert a.inertia_ == b.inertia_ and a.n_iter_ == b.n_iter_


def _blobs_f32(seed, n, d, k, std=1.0):
    from sklearn.datasets import make_blobs
    X, y = make_blobs(n_samples=n, n_features=d, centers=k, cluster_std=std, random_state=seed)
    return X.astype(np.float32), y


@pytest.mark.parametrize("seed,n,d,k,std", [(0, 3000, 20, 5, 4.0), (1, 5000, 64, 10, 6.0)])
def test_lloyd_from_init_matches_sklearn(seed, n, d, k, std):
    from sklearn.cluster import KMeans as SK
    from vit_som_amd import KMeans
    X, _ = _blobs_f32(seed, n, d, k, std)
    C0 = X[np.random.default_rng(seed).choice(n, k, replace=False)]
    ref = SK(n_clusters=k, init=C0, n_init=1, algorithm="lloyd").fit(X)
    km = KMeans(k, init=C0).fit(torch.from_numpy(X).cuda())
    assert np.array_equal(km.labels_.cpu().numpy(), ref.labels_)
    assert km.n_iter_ == ref.n_iter_
    assert abs(km.inertia_ - ref.inertia_) <= 1e-5 * ref.inertia_
    # and the float64 oracle agrees on the same init
    ol, oi, _, on = lloyd_oracle(X, C0)
    assert np.array_equal(ol, ref.labels_) and on == ref.n_iter_


def test_empty_cluster_relocation_matches_sklearn():
    from sklearn.cluster import KMeans as SK
    from vit_som_amd import KMeans
    X, _ = _blobs_f32(3, 2000, 12, 3, 1.0)
    C0 = np.concatenate([X[[0, 1, 2]], np.full((1, 12), 1e3, np.float32)])
    ref = SK(n_clusters=4, init=C0, n_init=1, algorithm="lloyd").fit(X)
    km = KMeans(4, init=C0).fit(torch.from_numpy(X).cuda())
    assert np.array_equal(km.labels_.cpu().numpy(), ref.labels_)
    assert km.n_iter_ == ref.n_iter_
    assert np.allclose(km.cluster_centers_.cpu().numpy(), ref.cluster_centers_, rtol=1e-5, atol=1e-4)
    assert abs(km.inertia_ - ref.inertia_) <= 1e-5 * ref.inertia_


def test_emptied_donor_placed_like_sklearn():
    """The relocation empties a one-member donor; _average_centers puts it on the heaviest cluster."""
    from sklearn.cluster import KMeans as SK
    from vit_som_amd import KMeans
    X, C0 = donor_case(np.float32)
    Xd = torch.from_numpy(X).cuda()
    for max_iter in (1, 300):
        ref = SK(n_clusters=3, init=C0, n_init=1, algorithm="lloyd", max_iter=max_iter).fit(X)
        km = KMeans(3, init=C0, max_iter=max_iter).fit(Xd)
        assert np.array_equal(km.labels_.cpu().numpy(), ref.labels_) and km.n_iter_ == ref.n_iter_
        assert np.allclose(km.cluster_centers_.cpu().numpy(), ref.cluster_centers_, rtol=1e-5, atol=1e-4)
        assert abs(km.inertia_ - ref.inertia_) <= 1e-5 * ref.inertia_


def test_kmeans_plusplus_picks_sklearn_rows():
    from sklearn.cluster import kmeans_plusplus as sk_pp
    from vit_som_amd import kmeans_plusplus
    for seed, k in [(0, 10), (1, 4), (2, 1)]:
        X, _ = _blobs_f32(seed, 4000, 32, max(k, 2), 1.0)
        _, ref_idx = sk_pp(X, k, random_state=seed)
        centers, idx = kmeans_plusplus(torch.from_numpy(X).cuda(), k, random_state=seed)
        assert np.array_equal(idx, ref_idx)
        assert torch.equal(centers.cpu(), torch.from_numpy(X[idx]))


def _same_up_to_permutation(a, b):
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


def test_full_fit_matches_sklearn():
    from sklearn.cluster import KMeans as SK
    from vit_som_amd import KMeans
    X, _ = _blobs_f32(5, 6000, 48, 8, 2.0)
    ref = SK(n_clusters=8, random_state=0, n_init=10).fit(X)
    km = KMeans(8, random_state=0, n_init=10)
    labels = km.fit_predict(torch.from_numpy(X).cuda())
    assert labels.dtype == torch.int64 and labels.is_cuda
    assert _same_up_to_permutation(labels.cpu().numpy(), ref.labels_)
    assert abs(km.inertia_ - ref.inertia_) <= 1e-5 * ref.inertia_


class _Loader(list):
    pass


def _separable_images(seed, n_per, ncls, C, S, nb):
    g = torch.Generator().manual_seed(seed)
    protos = torch.rand(ncls, C, S, S, generator=g)
    y = torch.arange(ncls).repeat_interleave(n_per)
    x = (protos[y] + 0.05 * torch.randn(len(y), C, S, S, generator=g)).clamp(0, 1)
    perm = torch.randperm(len(y), generator=g)
    x, y = x[perm], y[perm]
    return _Loader((x[i:i + nb], y[i:i + nb]) for i in range(0, len(y), nb))


def _sklearn_metrics(feats, ys):
    from sklearn.cluster import KMeans as SK
    from sklearn.metrics import normalized_mutual_info_score
    from test_evaluation import purity_reference_loop
    pred = SK(n_clusters=len(np.unique(ys)), random_state=0, n_init=10).fit_predict(feats)
    return purity_reference_loop(ys, pred)[0], normalized_mutual_info_score(ys, pred)


def _models():
    import vit_som_amd
    z, cfg = load_golden("ref_cluster_tiny")
    vm = vit_som_amd.ViTSOM(copy.deepcopy(cfg), device="cuda:0")
    vm.load_state_dict(golden_params(z))
    zd, cfgd = load_golden("ref_desom_cls_tiny")
    dm = vit_som_amd.DESOM(copy.deepcopy(cfgd), device="cuda:0")
    dm.load_state_dict(golden_params(zd))
    return (vm, cfg), (dm, cfgd)


def test_evaluate_kmeans_vitsom_and_desom():
    from vit_som_amd.evaluation import evaluate_kmeans
    for m, cfg in _models():
        d = cfg["data"]
        batches = _separable_images(5, 12, 4, d["num_channels"], d["input_size"], 8)
        feats, ys = [], []
        for x, y in batches:
            out = m(x.cuda())
            f = out[1]                                   # vit_som: recon_img, desom: x_encoded
            feats.append(f.reshape(f.shape[0], -1).cpu().numpy()); ys.append(y.numpy())
        feats, ys = np.concatenate(feats), np.concatenate(ys)
        assert feats.shape[1] == (d["num_channels"] * d["input_size"] ** 2 if cfg["hyperparameters"]["model_arch"] == "vit_som"
                                  else m.autoencoder.encoder_dims[-1])
        purity, nmi, _ = evaluate_kmeans(m, cfg, batches)
        p_ref, n_ref = _sklearn_metrics(feats, ys)
        assert abs(purity - p_ref) < 1e-12 and abs(nmi - n_ref) < 1e-10, (purity, p_ref, nmi, n_ref)


def _dp_worker(rank, world, port, out):
    import torch.distributed as dist
    from vit_som_amd.evaluation import evaluate_kmeans
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    (m, cfg), _ = _models()
    m.world_size, m.rank = world, rank
    d = cfg["data"]
    batches = _separable_images(6, 10, 4, d["num_channels"], d["input_size"], 8)
    mine = _Loader(b for i, b in enumerate(batches) if i % world == rank)
    res = evaluate_kmeans(m, cfg, mine)
    torch.save(res[:2], f"{out}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


def test_evaluate_kmeans_two_ranks(tmp_path):
    from test_distributed import _free_port
    out = str(tmp_path / "km")
    mp.spawn(_dp_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    r0, r1 = torch.load(f"{out}.0"), torch.load(f"{out}.1")
    (m, cfg), _ = _models()
    d = cfg["data"]
    batches = _separable_images(6, 10, 4, d["num_channels"], d["input_size"], 8)
    order = [b for i, b in enumerate(batches) if i % 2 == 0] + [b for i, b in enumerate(batches) if i % 2 == 1]
    feats = np.concatenate([m(x.cuda())[1].reshape(x.shape[0], -1).cpu().numpy() for x, _ in order])
    ys = np.concatenate([y.numpy() for _, y in order])
    p_ref, n_ref = _sklearn_metrics(feats, ys)
    assert r0 == r1
    assert abs(r0[0] - p_ref) < 1e-12 and abs(r0[1] - n_ref) < 1e-10
