"""Host pieces of UMAP.transform (vit_som_amd/umap.py steps 9-13) against the numpy restatement in umap_transform_ref.py:
the bipartite graph and its pruning, the n_epochs rule, argument validation and the C entry's refusals.  No GPU."""
import numpy as np
import pytest
import torch

import umap_transform_ref as R
from test_umap_cpu import neg_sample


def _table(k, seed=0, M=40, N=90, dim=5):
    """kNN table of M new points among N training points (float64, ascending (distance, ordinal)): row 0 coincides with
    a training row (a zero distance), row 1 is equally far from all its neighbours."""
    rng = np.random.default_rng(seed)
    train, new = rng.normal(size=(N, dim)), rng.normal(size=(M, dim))
    new[0] = train[7]
    D = np.sqrt(((new[:, None, :] - train[None, :, :]) ** 2).sum(-1))
    idx = np.stack([np.lexsort((np.arange(N), D[i]))[:k] for i in range(M)])
    dist = np.take_along_axis(D, idx, axis=1)
    dist[1] = dist[1, 0]
    return idx, dist


@pytest.mark.parametrize("lc", [1.0, 2.5])
@pytest.mark.parametrize("k", [2, 15, 64])
@pytest.mark.parametrize("n_epochs", [100, 3])
def test_transform_graph_matches_restatement(lc, k, n_epochs):
    from vit_som_amd.umap import transform_graph
    idx, dist = _table(k, seed=k)
    assert dist[0, 0] == 0.0 and (dist[1] == dist[1, 0]).all() and dist[1, 0] > 0
    w, eps = transform_graph(idx, dist, lc, n_epochs)
    rw, reps = R.graph(dist, lc, n_epochs)
    assert w.dtype == np.float64 and eps.dtype == np.float64 and w.shape == eps.shape == (40, k)
    assert np.array_equal(w, rw) and np.array_equal(eps, reps)
    assert np.allclose(w.sum(axis=1), 1.0, rtol=0, atol=1e-14) and (w > 0).all()
    assert (w[1] == w[1, 0]).all() and abs(w[1, 0] - 1.0 / k) < 1e-15      # all-equal distances: equal memberships
    assert w[0, 0] == w[0].max()                                           # the coincident training row
    pruned = w < w.max() / n_epochs                                        # the pruning rule, and +inf on what it prunes
    assert np.array_equal(np.isinf(eps), pruned)
    assert np.array_equal(eps[~pruned], w.max() / w[~pruned]) and eps.min() == 1.0
    if n_epochs == 3 and k > 2:
        assert pruned.any() and not pruned.all()


def test_transform_graph_zero_epochs_and_shapes():
    from vit_som_amd.umap import transform_graph
    idx, dist = _table(15)
    w, eps = transform_graph(idx, dist, 1.0, 0)
    assert np.array_equal(w, R.graph(dist, 1.0, 0)[0]) and np.isinf(eps).all()
    with pytest.raises(ValueError, match="same"):
        transform_graph(idx[:, :5], dist, 1.0, 10)


def test_n_epochs_rule():
    from vit_som_amd.umap import transform_n_epochs
    assert transform_n_epochs(None, 10000) == 100 and transform_n_epochs(None, 10001) == 30
    assert transform_n_epochs(200, 5) == 66 and transform_n_epochs(2, 5) == 0
    for n, M in [(None, 10000), (None, 10001), (200, 5), (2, 5), (500, 70000)]:
        assert transform_n_epochs(n, M) == R.n_epochs_rule(n, M)


def test_restatement_hashes_arrays_as_scalars_and_chains():
    """The restatement's own footing: neg_sample on a uint64 array is neg_sample per element, and its layout over
    [0, 3) then [3, 6) is its layout over [0, 6)."""
    edges = np.array([0, 1, 7 * 8 + 3, (1 << 40) + 5, (1 << 63) + 11], dtype=np.uint64)
    for seed, n, p, N in [(0x1234_5678_9ABC_DEF1, 5, 3, 80), ((1 << 64) - 1, 99, 0, 2000), (0, 0, 0, 3)]:
        assert neg_sample(seed, n, edges, p, N).tolist() == [neg_sample(seed, n, int(e), p, N) for e in edges]
    idx, dist = _table(8, seed=3)
    w, eps = R.graph(dist, 1.0, 30)
    Yt = np.random.default_rng(0).uniform(0, 10, size=(90, 2)).astype(np.float32)
    args = (idx, w, eps, Yt, 1.577, 0.895, 1.0, 0.25, 30)
    for T in (np.float64, np.float32):
        whole = R.layout(*args, 0, 6, 5, 77, T)
        part = R.layout(*args, 0, 3, 5, 77, T)
        rest = R.layout(*args, 3, 6, 5, 77, T, Y=part[0], state=part[1:3])
        assert all(np.array_equal(x, y) for x, y in zip(whole[:3], rest[:3]))
        assert whole[3] == part[3] + rest[3] > 0 and whole[4] == part[4] + rest[4] > 0
        assert np.array_equal(R.layout(*args, 0, 0, 5, 77, T)[0], R.init(idx, w, eps, Yt, T))


def test_transform_argument_validation():
    from vit_som_amd import UMAP
    with pytest.raises(ValueError, match="fit"):
        UMAP().transform(torch.zeros(3, 4))
    m = UMAP()
    m._raw_data, m.embedding_ = torch.zeros(100, 4), torch.zeros(100, 2)     # as fit leaves them (no GPU here)
    assert m.transform(m._raw_data) is m.embedding_
    with pytest.raises(ValueError, match="columns"):
        m.transform(torch.zeros(3, 5))
    with pytest.raises(ValueError, match="GPU"):
        m.transform(torch.zeros(3, 4))
    with pytest.raises(ValueError, match="float32"):
        m.transform(torch.zeros(3, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match="rows"):
        m.transform(torch.zeros(0, 4))
    with pytest.raises(ValueError):
        m.transform(np.zeros((3, 4), np.float32))


def test_c_abi_rejects_bad_transform_calls():
    from vit_som_amd._lib import last_error, lib
    big = 1 << 20

    def call(idx=16, w=16, eps=16, yt=32, N=80, y=48, M=70, k=8, dim=2, n_epochs=30, e0=0, e1=6, rate=5, status=16, ws=64,
             ws_bytes=big):
        return lib.vsom_umap_transform_layout(idx, w, eps, yt, N, y, M, k, dim, 1.5, 0.9, 1.0, 0.25, n_epochs, e0, e1, rate, 7,
                                              status, ws, ws_bytes, None)
    for name in ("idx", "w", "eps", "yt", "y", "status"):
        assert call(**{name: None}) == -1 and "null" in last_error()
    assert call(dim=0) == -3 and call(dim=5) == -3 and "dim=5" in last_error()
    assert call(k=0) == -1
    assert call(k=65) == -3 and "k=65" in last_error()
    assert call(M=0) == -1 and call(N=0) == -1
    assert call(e0=7, e1=6) == -1                                # epoch_begin > epoch_end
    assert call(e1=31) == -1 and "epochs" in last_error()        # epoch_end > n_epochs
    assert call(e0=-1) == -1
    assert call(rate=0) == -1 and "negative_sample_rate" in last_error()
    assert call(y=32) == -1                                      # Y aliases Y_train
    assert call(ws=None) == -4
    assert call(ws_bytes=2 * 8 * 70 * 8 - 1) == -4 and "workspace" in last_error()
    assert lib.vsom_umap_transform_workspace_bytes(0, 8) == 0 and lib.vsom_umap_transform_workspace_bytes(70, 0) == 0
    for M, k in [(1, 1), (70, 8), (1600, 15), (40000, 64)]:
        assert lib.vsom_umap_transform_workspace_bytes(M, k) >= 2 * 8 * M * k
