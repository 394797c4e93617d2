"""PCA without a GPU: the numpy restatement of the algorithm (pca_ref.py) against sklearn in fp64, the host-only parts of
pca.py / evaluation.py / som.py, and the refusals of the new C-ABI entries, which happen on the host before any launch."""
import copy
import warnings

import numpy as np
import pytest
import torch

import pca_ref as R
from helpers import load_golden

P = 4096                    # stands for a non-null, 16-byte aligned device pointer: nothing is launched, nothing dereferenced
BIG = 1 << 40


# ------------------------------------------------------------------ the algorithm, before any kernel
@pytest.mark.parametrize("fx", R.SOLVER_FIXTURES + [R.WIDE_FIXTURE], ids=lambda f: f"{f[0]}x{f[1]}k{f[5]}")
def test_restatement_against_sklearn_fp64(fx):
    N, D, r, ratio, noise, k = fx
    X = R.fixture(N, D, r, ratio, noise)
    sk32, sk64 = R.sklearn_pair(*fx)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = R.pca_restated(X, k)
    assert got["width"] == min(k + 8, N, D)
    lam1 = sk64.explained_variance_[0]
    ev_err = float(np.max(np.abs(got["explained_variance"] - sk64.explained_variance_)) / lam1)
    ev_bound = R.bound(sk32.explained_variance_, sk64.explained_variance_)
    print(f"explained variance: {ev_err:.2e} (bound {ev_bound:.2e})")
    assert ev_err <= ev_bound
    assert R.rel_err(got["explained_variance_ratio"], sk64.explained_variance_ratio_) <= \
        R.bound(sk32.explained_variance_ratio_, sk64.explained_variance_ratio_)
    assert R.rel_err(got["mean"], sk64.mean_) <= R.bound(sk32.mean_, sk64.mean_)
    assert R.ortho_err(got["components"]) <= 4 * max(R.ortho_err(sk32.components_), R.EPS32)
    assert float(got["residuals"].max()) <= 1e-3
    if fx is not R.WIDE_FIXTURE:            # the 57th direction of the wide fixture is conditioned by its gap, not by the algorithm
        cos = R.one_minus_cos(got["components"], sk64.components_)
        cos_bound = 4 * max(R.one_minus_cos(sk32.components_, sk64.components_), R.EPS32)
        print(f"1 - |cos|: {cos:.2e} (bound {cos_bound:.2e})")
        assert cos <= cos_bound
    big = np.argmax(np.abs(got["components"]), axis=1)
    assert (got["components"][np.arange(k), big] > 0).all()


def test_restatement_on_a_rank_deficient_set():
    N, D, r, ratio, noise, k = R.RANK_FIXTURE
    X = R.fixture(N, D, r, ratio, noise)
    sk32, sk64 = R.sklearn_pair(*R.RANK_FIXTURE)
    got = R.pca_restated(X, k)
    lam1 = sk64.explained_variance_[0]
    assert np.max(np.abs(got["explained_variance"][:4] - sk64.explained_variance_[:4])) / lam1 <= \
        R.bound(sk32.explained_variance_[:4], sk64.explained_variance_[:4])
    assert got["explained_variance"][4] <= R.EPS32 * lam1
    assert np.isfinite(got["components"]).all()
    assert R.ortho_err(got["components"]) <= 4 * max(R.ortho_err(sk32.components_), R.EPS32)


# ------------------------------------------------------------------ host-only parts
def test_orthonormalising_transform_and_ritz():
    from vit_som_amd.pca import orthonormalising_transform, ritz
    rng = np.random.RandomState(3)
    l, D = 12, 300
    # one pass of the iteration on a covariance whose spectrum spans six decades: Zt = B C with B orthonormal rows
    V = np.linalg.qr(rng.standard_normal((D, D)))[0]
    C = (V * 10.0 ** -np.linspace(0, 6, D)) @ V.T
    B = np.linalg.qr(rng.standard_normal((D, l)))[0].T
    Zt = B @ C
    G, H = Zt @ Zt.T, B @ Zt.T
    theta, S, res = ritz(H, G)
    assert (np.diff(theta) <= 0).all() and S.shape == (l, l) and res.shape == (l,) and (res >= 0).all()
    assert np.allclose(S.T @ ((H + H.T) / 2) @ S, np.diag(theta), atol=1e-9 * abs(theta).max())
    T = orthonormalising_transform(G, S)
    assert T.shape == (l, l)
    W = T @ Zt
    assert np.max(np.abs(W @ W.T - np.eye(l))) <= 1e-12
    # without a rotation: rows of very different length are only scaled
    Zt = rng.standard_normal((l, D)) * (10.0 ** -np.arange(l))[:, None]
    T = orthonormalising_transform(Zt @ Zt.T)
    assert T.shape == (l, l)
    W = T @ Zt
    assert np.max(np.abs(W @ W.T - np.eye(l))) <= 1e-12
    # a zero row: its direction is dropped, the others stay orthonormal
    Zt[5] = 0.0
    T = orthonormalising_transform(Zt @ Zt.T)
    assert T.shape == (l - 1, l)
    W = T @ Zt
    assert np.isfinite(T).all() and np.max(np.abs(W @ W.T - np.eye(l - 1))) <= 1e-12


def test_sign_rule():
    from vit_som_amd.pca import sign_rule
    c = torch.tensor([[0.1, -3.0, 2.0], [0.5, 0.2, -0.1], [0.0, 0.0, 0.0], [-1.0, 1.0, 0.5]])
    want = torch.tensor([[-0.1, 3.0, -2.0], [0.5, 0.2, -0.1], [0.0, 0.0, 0.0], [1.0, -1.0, -0.5]])
    assert torch.equal(sign_rule(c.clone()), want)


def test_components_for_and_effective_rank():
    from vit_som_amd.evaluation import components_for, effective_rank
    ratio = np.array([0.4, 0.3, 0.15, 0.06, 0.04])
    got = components_for(np.cumsum(ratio))
    assert got == {0.5: 2, 0.9: 4, 0.95: 5, 0.99: None}
    assert components_for(np.array([0.995])) == {0.5: 1, 0.9: 1, 0.95: 1, 0.99: 1}
    assert effective_rank([3.0, 3.0, 3.0, 3.0]) == pytest.approx(4.0, rel=1e-14)
    assert effective_rank([7.0, 0.0, 0.0]) == pytest.approx(1.0, rel=1e-14)
    p = np.array([0.5, 0.25, 0.25])
    assert effective_rank(10 * p) == pytest.approx(float(np.exp(-(p * np.log(p)).sum())), rel=1e-14)
    assert effective_rank([0.0, 0.0]) == 0.0


def _som_layer(map_size, topology):
    from vit_som_amd import SOMLayer
    _, cfg = load_golden("ref_cluster_tiny")
    cfg = copy.deepcopy(cfg)
    cfg["hyperparameters"]["som"].update(map_size=list(map_size), topology=topology)
    return SOMLayer(cfg)


def test_grid_coordinates_square_3x5():
    uv = _som_layer((3, 5), "square").pca_grid_coordinates().numpy()
    assert uv.shape == (15, 2) and uv.min() == -1.0 and uv.max() == 1.0
    rows, cols = np.divmod(np.arange(15), 5)
    assert np.allclose(uv[:, 0], cols / 2.0 - 1.0, atol=1e-15)          # the five columns: the larger extent -> PC1
    assert np.allclose(uv[:, 1], rows - 1.0, atol=1e-15)


def test_grid_coordinates_hexagonal_4x3():
    uv = _som_layer((4, 3), "hexa").pca_grid_coordinates().numpy()
    assert uv.shape == (12, 2) and uv.min() == -1.0 and uv.max() == 1.0
    rows, cols = np.divmod(np.arange(12), 3)
    x = cols + 0.5 * (rows % 2)                                          # extent 2.5
    y = rows * np.sqrt(3) / 2                                            # extent 2.598: the larger one -> PC1
    assert np.allclose(uv[:, 0], 2 * y / y.max() - 1, atol=1e-6)
    assert np.allclose(uv[:, 1], 2 * x / 2.5 - 1, atol=1e-6)


def test_init_prototypes_refuses_bad_arguments():
    som = _som_layer((3, 5), "square")
    with pytest.raises(ValueError, match="latents must be"):
        som.init_prototypes(torch.zeros(10, 7))
    with pytest.raises(ValueError, match="unknown method"):
        som.init_prototypes(torch.zeros(10, som.prototypes.shape[1]), method="kmeans")


# ------------------------------------------------------------------ PCA's argument errors
def test_pca_argument_errors():
    from vit_som_amd import PCA
    X = torch.zeros(6, 4)
    for k in (0, 5, 7):
        with pytest.raises(ValueError, match=r"n_components=\d must be between 1 and min\(n_samples, n_features\)=4"):
            PCA(n_components=k).fit(X)
    with pytest.raises(ValueError, match="not fitted yet"):
        PCA().transform(X)
    with pytest.raises(AttributeError):
        PCA().inverse_transform(X[:, :2])
    with pytest.raises(ValueError, match="HIP device tensor"):
        PCA(n_components=2).fit(X)


# ------------------------------------------------------------------ refusals without a launch
N, D, W = 300, 40, 10


def _sized_entries():
    """name -> (count needed, call(buffer, count, N=, D=, l=, X=)) for every new entry that takes a sized buffer."""
    from vit_som_amd._lib import lib as L
    return {
        "vsom_pca_colstats": (lambda N, D, l: L.vsom_pca_colstats_parts(N, D),
                              lambda b, n, N=N, D=D, l=W, X=P: L.vsom_pca_colstats(X, D, N, D, P, P, b, n, None)),
        "vsom_pca_project": (lambda N, D, l: L.vsom_pca_slabs(N, D, l, 0),
                             lambda b, n, N=N, D=D, l=W, X=P: L.vsom_pca_project(X, D, N, D, P, P, D, l, None, P, l, b, n, None)),
        "vsom_pca_backproject": (lambda N, D, l: L.vsom_pca_slabs(N, D, l, 1),
                                 lambda b, n, N=N, D=D, l=W, X=P: L.vsom_pca_backproject(P, l, X, D, N, D, P, l, P, D, b, n, None)),
    }


@pytest.mark.parametrize("name", ["vsom_pca_colstats", "vsom_pca_project", "vsom_pca_backproject"])
def test_sized_buffers_are_refused_before_any_launch(name):
    from vit_som_amd._lib import last_error
    need_of, call = _sized_entries()[name]
    need = need_of(N, D, W)
    assert need > 0
    assert call(P, need - 1) == -4, last_error()
    msg = last_error()
    assert "too small" in msg or "<" in msg, msg
    assert call(P, 0) == -4 and call(None, BIG) == -4
    assert call(P + 8, BIG) in (-2, -4), last_error()
    assert call(P, BIG, X=None) == -1 and "null" in last_error()
    assert call(P, BIG, N=1) == -3, last_error()
    if name != "vsom_pca_colstats":
        assert call(P, BIG, l=257, D=300) == -3, last_error()
        assert call(P, BIG, l=D + 1) == -3, last_error()


def test_count_queries_are_host_arithmetic():
    from vit_som_amd._lib import lib as L
    for which in (0, 1):
        assert L.vsom_pca_slabs(0, 8, 2, which) == 0 and L.vsom_pca_slabs(8, 0, 2, which) == 0
        assert L.vsom_pca_slabs(8, 8, 0, which) == 0 and L.vsom_pca_slabs(-5, 8, 2, which) == 0
    assert L.vsom_pca_slabs(8, 8, 2, 2) == 0
    assert L.vsom_pca_colstats_parts(0, 8) == 0 and L.vsom_pca_colstats_parts(8, -1) == 0
    # whole slabs of the output, at least one; many splits where the output has few tiles
    assert L.vsom_pca_slabs(257, 12288, 10, 0) % (257 * 10) == 0 and L.vsom_pca_slabs(257, 12288, 10, 0) // (257 * 10) >= 32
    assert L.vsom_pca_slabs(257, 12288, 10, 1) % (10 * 12288) == 0
    assert L.vsom_pca_slabs(5, 40, 5, 0) == 5 * 5 * 2 and L.vsom_pca_slabs(5, 40, 5, 1) == 5 * 40
    # column statistics: at least two workgroups per CU (512) at the benchmark's shape, every split at least one row
    parts = L.vsom_pca_colstats_parts(10000, 12288)
    assert parts % 12288 == 0 and (parts // 12288) * (12288 // 64) >= 512
    assert L.vsom_pca_colstats_parts(5, 40) == 40


def test_the_other_entries_refuse_on_the_host():
    from vit_som_amd._lib import last_error, lib as L
    assert L.vsom_pca_gram(None, 40, None, 0, 10, 40, P, None, None) == -1 and "null" in last_error()
    assert L.vsom_pca_gram(P, 40, P, 40, 10, 40, P, None, None) == -1            # B without H
    assert L.vsom_pca_gram(P, 300, None, 0, 257, 300, P, None, None) == -3
    assert L.vsom_pca_rotate(None, 4, 10, P, 40, 40, P, 40, None) == -1
    assert L.vsom_pca_rotate(P, 4, 10, 1 << 20, 40, 40, 1 << 20, 40, None) == -1 and "overlaps" in last_error()
    assert L.vsom_pca_rotate(P, 4, 10, 1 << 20, 40, 40, (1 << 20) + 160 * 9, 40, None) == -1      # the last row of Zt
    assert L.vsom_pca_rotate(P, 257, 10, 1 << 20, 40, 40, 1 << 22, 40, None) == -3
    assert L.vsom_pca_reconstruct(None, 2, 5, 2, None, P, 40, 40, None, P, 40, None) == -1
    assert L.vsom_pca_reconstruct(P, 2, 5, 2, None, P, 39, 40, None, P, 40, None) == -1          # ldb < D
    assert L.vsom_pca_reconstruct(P, 300, 5, 257, None, P, 400, 400, None, P, 400, None) == -3
