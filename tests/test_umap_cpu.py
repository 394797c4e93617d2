"""Host pieces of the HIP UMAP (vit_som_amd/umap.py) against a float64 numpy restatement of umap-learn 0.5's steps 2-6
(stated in umap.py's docstring), the negative-sample hash, and argument validation.  No GPU."""
import numpy as np
import pytest
import scipy.sparse
import torch

SMOOTH_K_TOLERANCE = 1e-5
_M64 = (1 << 64) - 1


# ------------------------------------------------------------------ restatement
def splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def neg_sample(seed, epoch, edge, p, N):
    """The negative sample p of edge `edge` in epoch `epoch` (include/vitsom_hip.h, vsom_umap_neg_sample)."""
    return splitmix64(splitmix64(seed ^ edge) ^ ((epoch << 32) | p)) % N


def ref_smooth_knn_dist(d, lc=1.0, n_iter=64):
    """Step 2, one row at a time (umap-learn's smooth_knn_dist in float64)."""
    N, k = d.shape
    target = np.log2(k)
    sigma, rho = np.zeros(N), np.zeros(N)
    mean_all = d.mean()
    for i in range(N):
        row = d[i]
        nz = row[row > 0.0]
        if nz.shape[0] >= lc:
            idx = int(np.floor(lc))
            t = lc - idx
            if idx > 0:
                rho[i] = nz[idx - 1]
                if t > SMOOTH_K_TOLERANCE:
                    rho[i] += t * (nz[idx] - nz[idx - 1])
            else:
                rho[i] = t * nz[0]
        elif nz.shape[0] > 0:
            rho[i] = np.max(nz)
        lo, hi, mid = 0.0, np.inf, 1.0
        for _ in range(n_iter):
            psum = 0.0
            for j in range(1, k):
                x = row[j] - rho[i]
                psum += np.exp(-(x / mid)) if x > 0 else 1.0
            if abs(psum - target) < SMOOTH_K_TOLERANCE:
                break
            if psum > target:
                hi = mid
                mid = (lo + hi) / 2.0
            else:
                lo = mid
                mid = mid * 2 if hi == np.inf else (lo + hi) / 2.0
        floor = 1e-3 * (np.mean(row) if rho[i] > 0.0 else mean_all)
        sigma[i] = floor if mid < floor else mid
    return sigma, rho


def ref_graph(knn_idx, knn_dist, sigma, rho, mix):
    """Steps 3-4 as a dense float64 matrix."""
    N, k = knn_idx.shape
    A = np.zeros((N, N))
    for i in range(N):
        for j in range(k):
            c = knn_idx[i, j]
            x = knn_dist[i, j] - rho[i]
            A[i, c] = 0.0 if c == i else (1.0 if x <= 0.0 or sigma[i] == 0.0 else np.exp(-(x / sigma[i])))
    P = A * A.T
    return mix * (A + A.T - P) + (1.0 - mix) * P


def knn_table(X, k):
    """Exact kNN in float64: ascending (distance, index), the row itself first."""
    D = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1))
    np.fill_diagonal(D, -1.0)
    N = X.shape[0]
    idx = np.stack([np.lexsort((np.arange(N), D[i]))[:k] for i in range(N)])
    dist = np.take_along_axis(D, idx, axis=1)
    dist[:, 0] = 0.0
    return idx, dist


def _points(seed, N=120, dim=5):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(N, dim))
    X[10] = X[3]                       # duplicates: zero distances past the row itself
    X[11] = X[3]
    X[40:60] = X[40]                   # 20 copies: rows whose k distances are all zero
    return X


# ------------------------------------------------------------------ steps 2-4
@pytest.mark.parametrize("lc", [1.0, 1.5, 0.5])
@pytest.mark.parametrize("k", [15, 5])
def test_sigma_rho_match_restatement(lc, k):
    from vit_som_amd.umap import smooth_knn_dist
    idx, dist = knn_table(_points(1), k)
    sigma, rho = smooth_knn_dist(dist, lc)
    rs, rr = ref_smooth_knn_dist(dist, lc)
    assert np.allclose(rho, rr, rtol=1e-5, atol=0)
    assert np.allclose(sigma, rs, rtol=1e-5, atol=0)
    assert (rho[40:60] == 0).all()                     # all-zero rows: rho = 0, sigma floored at 1e-3 mean(all)
    assert np.allclose(sigma[40:60], 1e-3 * dist.mean(), rtol=1e-12)


@pytest.mark.parametrize("lc", [1.0, 1.5, 0.5])
@pytest.mark.parametrize("mix", [1.0, 0.5])
def test_graph_matches_restatement_and_is_symmetric(lc, mix):
    from vit_som_amd.umap import fuzzy_simplicial_set
    idx, dist = knn_table(_points(2), 15)
    G, sigma, rho = fuzzy_simplicial_set(idx, dist, mix, lc)
    rs, rr = ref_smooth_knn_dist(dist, lc)
    R = ref_graph(idx, dist, rs, rr, mix)
    Gd = G.toarray()
    assert np.array_equal(Gd != 0, R != 0)                      # sparsity exact
    assert np.abs(Gd - R).max() <= 1e-6
    assert G.has_sorted_indices and G.nnz == int((Gd != 0).sum())
    assert np.array_equal(Gd, Gd.T)                             # symmetric bit for bit
    G32 = G.astype(np.float32).toarray()
    assert np.array_equal(G32, G32.T)


def test_ab_params_at_defaults():
    from vit_som_amd.umap import find_ab_params
    a, b = find_ab_params(1.0, 0.1)
    assert abs(a - 1.57694346) < 1e-7 and abs(b - 0.89506088) < 1e-7


def test_pruning_and_epochs_per_sample():
    from vit_som_amd.umap import default_n_epochs, fuzzy_simplicial_set, make_schedule
    assert default_n_epochs(10000) == 500 and default_n_epochs(10001) == 200
    idx, dist = knn_table(_points(3), 15)
    G = fuzzy_simplicial_set(idx, dist, 1.0, 1.0)[0].astype(np.float32)
    for n_epochs, rate in [(200, 5), (20, 3)]:
        P, eps, eps_neg = make_schedule(G, n_epochs, rate)
        Gd = G.toarray().astype(np.float64)
        keep = (Gd > 0) & (Gd >= Gd.max() / n_epochs)
        assert np.array_equal(P.toarray() != 0, keep)
        assert np.array_equal(P.toarray(), np.where(keep, G.toarray(), 0))
        w = Gd[keep]                                            # row-major = CSR order with sorted indices
        assert np.array_equal(eps, Gd.max() / w)
        assert np.array_equal(eps_neg, (Gd.max() / w) / rate)
        assert eps.min() == 1.0
        Pd = P.toarray()
        assert np.array_equal(Pd, Pd.T)
    assert (G.toarray() < G.toarray().max() / 20).any()        # the second case prunes something


# ------------------------------------------------------------------ negative samples
def test_negative_sample_hash():
    from vit_som_amd import ops
    assert splitmix64(0) == 0xE220A8397B1DCDAF                  # SplitMix64's first output from state 0
    known = {(0, 0, 0, 0, 1000): 55, (42, 1, 0, 0, 70000): 61557, (42, 199, 123456, 3, 70000): 21270,
             ((1 << 64) - 1, 499, 1 << 40, 7, 60000): 32782, (12345, 7, 99, 4, 257): 182}
    for args, want in known.items():
        assert neg_sample(*args) == want
        assert ops.umap_neg_sample(*args) == want
    rng = np.random.default_rng(0)
    for _ in range(200):
        args = (int(rng.integers(0, 1 << 63)) * 2 + 1, int(rng.integers(0, 500)), int(rng.integers(0, 1 << 40)),
                int(rng.integers(0, 64)), int(rng.integers(1, 1 << 31)))
        assert ops.umap_neg_sample(*args) == neg_sample(*args)
    assert ops.umap_neg_sample(1, 0, 0, 0, 0) == -1


# ------------------------------------------------------------------ validation
@pytest.mark.parametrize("kw,msg", [({"n_neighbors": 1}, "n_neighbors"), ({"n_neighbors": 65}, "n_neighbors"),
                                    ({"n_components": 5}, "n_components"), ({"n_components": 0}, "n_components"),
                                    ({"metric": "manhattan"}, "metric"), ({"init": "pca"}, "init"),
                                    ({"n_epochs": 0}, "n_epochs"), ({"min_dist": 2.0}, "min_dist"),
                                    ({"set_op_mix_ratio": 1.5}, "set_op_mix_ratio"),
                                    ({"negative_sample_rate": 0}, "negative_sample_rate"),
                                    ({"learning_rate": 0.0}, "learning_rate")])
def test_parameter_validation(kw, msg):
    from vit_som_amd import UMAP
    with pytest.raises(ValueError, match=msg):
        UMAP(**kw).fit(torch.zeros(100, 4))


def test_input_validation():
    from vit_som_amd import UMAP
    with pytest.raises(ValueError, match="GPU"):
        UMAP().fit(torch.zeros(100, 4))
    with pytest.raises(ValueError, match="exceed"):
        UMAP(n_neighbors=15).fit(torch.zeros(15, 4))
    with pytest.raises(ValueError, match="float32"):
        UMAP().fit(torch.zeros(100, 4, dtype=torch.float64))
    with pytest.raises(ValueError):
        UMAP().fit(np.zeros((100, 4), np.float32))


def test_c_abi_rejects_bad_calls():
    from vit_som_amd._lib import last_error, lib
    assert lib.vsom_umap_knn(None, 8, 100, 8, 5, 1, 16, 16, 16, 1 << 20, None) == -1
    assert lib.vsom_umap_knn(16, 8, 100, 8, 65, 1, 16, 16, 16, 1 << 20, None) == -3 and "k=65" in last_error()
    assert lib.vsom_umap_knn(16, 8, 100, 8, 5, 2, 16, 16, 16, 1 << 20, None) == -3               # manhattan
    assert lib.vsom_umap_knn(16, 8, 100, 8, 100, 1, 16, 16, 16, 1 << 20, None) == -1             # k >= N
    assert lib.vsom_umap_knn(16, 8, 100, 8, 5, 1, 16, 16, 16, 64, None) == -4                    # workspace
    assert lib.vsom_umap_knn_workspace_bytes(0, 5) == 0
    assert lib.vsom_umap_knn_workspace_bytes(70000, 15) >= 70000 * 15 * 8
    assert lib.vsom_umap_epoch(16, 16, 16, 16, 16, 16, 16, 32, 10, 5, 1.0, 1.0, 1.0, 1.0, 0, 0, None) == -3
    assert lib.vsom_umap_epoch(16, 16, 16, 16, 16, 16, 16, 16, 10, 2, 1.0, 1.0, 1.0, 1.0, 0, 0, None) == -1   # alias
    assert lib.vsom_umap_epoch(None, 16, 16, 16, 16, 16, 16, 32, 10, 2, 1.0, 1.0, 1.0, 1.0, 0, 0, None) == -1


def test_two_component_spectral_layout():
    """<= 2 dim components: component c around row c of [e_0 .. e_{m-1}, -e_0 .. -e_{m-1}] (m = ceil(components / 2);
    no centroids needed), scaled to half the smallest distance between those positions."""
    from vit_som_amd.umap import fuzzy_simplicial_set, spectral_init
    rng = np.random.default_rng(4)
    X = np.concatenate([rng.normal(size=(60, 3)), 100.0 + rng.normal(size=(60, 3))])
    idx, dist = knn_table(X, 10)
    G = fuzzy_simplicial_set(idx, dist, 1.0, 1.0)[0]
    emb = spectral_init(G, 2, np.random.RandomState(0), None)
    assert emb.shape == (120, 2) and np.isfinite(emb).all()
    for part, meta in ((emb[:60], [1.0, 0.0]), (emb[60:], [-1.0, 0.0])):    # e_0 and -e_0, 2 apart
        assert abs(np.abs(part - meta).max() - 1.0) < 1e-12
