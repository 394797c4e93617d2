"""t-SNE without a GPU: the numpy restatement (tsne_ref.py) against sklearn's own functions, the estimator's surface and
validation errors, the C-ABI entries' host-side refusals, and the host graph."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

import tsne_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ 1. the restatement against sklearn
def _sklearn_functions():
    try:
        from sklearn.manifold._t_sne import _joint_probabilities, _kl_divergence
        from sklearn.manifold._utils import _binary_search_perplexity
    except ImportError as e:                                 # a later sklearn has moved them
        pytest.skip(f"sklearn's private t-SNE functions are not where 1.7 has them: {e}")
    return _binary_search_perplexity, _joint_probabilities, _kl_divergence


def _sorted_sq_distances(N, k, seed):
    rs = np.random.RandomState(seed)
    X = rs.standard_normal((N, 8)) * rs.uniform(0.5, 3.0, size=(N, 1))
    return R.squared_f32(R.exact_knn(X, k, "euclidean")[1])


def test_conditional_p_matches_sklearn():
    bsp, _, _ = _sklearn_functions()
    d = _sorted_sq_distances(300, 63, 0)
    want = bsp(np.ascontiguousarray(d), 20.0, 0)
    got, beta, stop = R.conditional_p(d, 20.0)
    err = np.abs(got - want).max() / want.max()
    print(f"conditional P: max error {err:.3e} relative to the largest entry; stops {stop.min()}..{stop.max()}")
    assert err <= 1e-12
    assert np.abs(R.row_sums(got) - 1.0).max() <= 1e-12 and (beta > 0).all()


def test_joint_p_matches_sklearn():
    from scipy.spatial.distance import squareform
    _, joint, _ = _sklearn_functions()
    rs = np.random.RandomState(1)
    X = rs.standard_normal((64, 5))
    D = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1).astype(np.float32)
    want = squareform(joint(D, 15.0, 0))
    idx = np.array([[j for j in range(64) if j != i] for i in range(64)], dtype=np.int64)      # k = 63: every other row
    cond = R.conditional_p(np.take_along_axis(D, idx, axis=1), 15.0)[0]
    got = R.joint_p(idx, cond)
    err = np.abs(got - want).max() / want.max()
    print(f"joint P: max error {err:.3e} relative to the largest entry")
    assert err <= 1e-12


def test_gradient_and_kl_match_sklearn():
    from scipy.spatial.distance import squareform
    _, joint, kl_div = _sklearn_functions()
    rs = np.random.RandomState(2)
    X = rs.standard_normal((64, 5))
    D = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1).astype(np.float32)
    Pc = joint(D, 15.0, 0)
    Y = 1.5 * rs.standard_normal((64, 2))
    want_kl, want_grad = kl_div(Y.ravel().copy(), Pc, 1.0, 64, 2)
    kl, grad = R.kl_and_grad(squareform(Pc), Y)
    g_err = np.abs(grad.ravel() - want_grad).max() / np.abs(want_grad).max()
    print(f"gradient: max error {g_err:.3e} relative to the largest entry; KL {kl:.15f} against {want_kl:.15f}")
    assert g_err <= 1e-12 and abs(kl - want_kl) <= 1e-12 * abs(want_kl)
    # exaggeration multiplies P only, and the reported KL is the one of the multiplied P
    kl12, grad12 = R.kl_and_grad(squareform(Pc), Y, 12.0)
    want_kl12, want_grad12 = kl_div(Y.ravel().copy(), Pc * 12.0, 1.0, 64, 2)
    assert np.abs(grad12.ravel() - want_grad12).max() <= 1e-12 * np.abs(want_grad12).max()
    assert abs(kl12 - want_kl12) <= 1e-12 * abs(want_kl12)


def test_update_rule_matches_sklearn_in_float64():
    """One pass of sklearn's _gradient_descent body, written out, against update_step with a float64 state."""
    rs = np.random.RandomState(3)
    p, update, grad = rs.standard_normal((50, 2)), rs.standard_normal((50, 2)), rs.standard_normal((50, 2))
    gains = rs.uniform(0.005, 2.0, size=(50, 2))
    g = gains.copy()
    inc = update * grad < 0.0
    g[inc] += 0.2
    g[~inc] *= 0.8
    np.clip(g, 0.01, np.inf, out=g)
    u = 0.8 * update - 200.0 * (g * grad)
    Y2, u2, g2 = R.update_step(p, update, gains, grad, 0.8, 200.0)
    assert np.array_equal(g2, g) and np.allclose(u2, u, rtol=1e-15, atol=0) and np.allclose(Y2, p + u, rtol=1e-15, atol=0)
    Y3, u3, g3 = R.update_step(p.astype(np.float32), update.astype(np.float32), gains.astype(np.float32), grad, 0.8, 200.0)
    assert Y3.dtype == u3.dtype == g3.dtype == np.float32 and (g3 >= np.float32(0.01)).all()


# the shapes of the device test of the affinities: (N, k_eff, perplexity, seed of the clustered rows)
AFFINITY_CASES = [(64, 63, 15.0, 11), (257, 63, 20.0, 12), (300, 30, 10.0, 13)]


def affinity_rows(N, seed):
    """Clustered rows with three exact duplicates and one row 1e4 away from all others (the underflow / 1e-8 path)."""
    X, _ = R.blobs(N, 16, 4, seed, scale=3.0)
    X[5] = X[17]
    X[40] = X[17]
    X[N - 1] = 1e4 / 4.0                                    # 16 columns of 2500: 1e4 from the origin
    return X


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("N,k,perplexity,seed", AFFINITY_CASES)
def test_affinity_cases_stop_clear_of_the_tolerance(N, k, perplexity, seed, metric):
    """The device test allows a row to stop one step early or late when a differently rounded exp moves its entropy across
    the tolerance.  These seeds leave the restatement itself no such row: at no row's last two iterates does the entropy gap
    come within 1e-9 of the tolerance."""
    X = affinity_rows(N, seed)
    dist = R.exact_knn(X, k, metric)[1]
    d = R.squared_f32(dist) if metric == "euclidean" else dist
    _, gaps, stop = R.bisection_trace(d, perplexity)
    cols = np.arange(N)
    last = np.abs(gaps[stop, cols])
    before = np.abs(gaps[np.maximum(stop - 1, 0), cols])
    margin = min(np.abs(last - R.TOLERANCE).min(), np.abs(before - R.TOLERANCE).min())
    print(f"{metric} N={N} k={k}: stops {stop.min()}..{stop.max()}, closest approach to the tolerance {margin:.3e}")
    assert margin > 1e-9
    # every clustered row converges; only the far row (euclidean: 63 squared distances of 1e8 apart by f32 steps, sums that
    # underflow) may run into the step limit, which is a path of its own
    assert (stop[:N - 1] < R.N_STEPS - 1).all()
    P = R.conditional_p(d, perplexity)[0]
    assert np.abs(R.row_sums(P) - 1.0).max() <= 1e-12


# ------------------------------------------------------------------ 2. surface and ABI
def test_surface():
    import vit_som_amd
    from vit_som_amd import evaluation, tsne
    assert str(inspect.signature(vit_som_amd.TSNE.__init__)) == (
        "(self, n_components=2, perplexity=30.0, early_exaggeration=12.0, learning_rate='auto', max_iter=1000, "
        "n_iter_without_progress=300, min_grad_norm=1e-07, metric='euclidean', init='pca', random_state=None, **unsupported)")
    for name in ("fit", "fit_transform"):
        assert callable(getattr(vit_som_amd.TSNE, name))
    assert str(inspect.signature(tsne.visualize_tsne_progression)) == (
        "(model, config, dataloader, epoch=0, output_dir='experiments/plots/vit_som/tsne', perplexity=30.0)")
    assert str(inspect.signature(tsne.evaluate_tsne_quality)) == "(model, config, dataloader, n_neighbors=15, perplexity=30.0)"
    for name in ("visualize_tsne_progression", "evaluate_tsne_quality", "TSNEQualityReport"):
        obj = getattr(tsne, name)
        assert obj.__module__ == "vit_som_amd.tsne" and getattr(evaluation, name) is obj and getattr(vit_som_amd, name) is obj
    fields = {f for f in tsne.TSNEQualityReport.__dataclass_fields__}
    assert set(vit_som_amd.EmbeddingQuality.__dataclass_fields__) < fields
    assert {"embedding", "kl_divergence", "n_iter", "inference_time"} <= fields
    from vit_som_amd.train import _parser, main
    assert inspect.signature(main).parameters["tsne_quality"].default is False
    assert _parser().parse_args(["--config", "c", "--tsne-quality"]).tsne_quality is True


def test_validation_errors():
    from vit_som_amd import TSNE
    from vit_som_amd.tsne import neighbour_count
    X = torch.zeros(1000, 8)
    with pytest.raises(ValueError, match="must be 2.*degrees of freedom"):
        TSNE(n_components=3).fit(X)
    with pytest.raises(ValueError, match="barnes_hut.*the repulsion here is exact"):
        TSNE(method="barnes_hut")
    with pytest.raises(ValueError, match="angle.*the repulsion here is exact"):
        TSNE(angle=0.5)
    assert TSNE(method="exact").max_iter == 1000
    with pytest.raises(TypeError):
        TSNE(n_jobs=2)
    with pytest.raises(ValueError, match=r"perplexity \(63\) must be below the number of neighbours.*= 63"):
        TSNE(perplexity=63).fit(X)
    with pytest.raises(ValueError, match=r"perplexity \(70.5\) must be below the number of neighbours"):
        TSNE(perplexity=70.5).fit(X)
    with pytest.raises(ValueError, match=r"must be less than n_samples \(20\)"):
        TSNE(perplexity=20).fit(torch.zeros(20, 8))
    with pytest.raises(ValueError, match="below the number of neighbours"):
        TSNE(perplexity=19.5).fit(torch.zeros(20, 8))        # k = 19
    with pytest.raises(ValueError, match="metric must be one of"):
        TSNE(metric="manhattan").fit(X)
    with pytest.raises(ValueError, match="learning_rate"):
        TSNE(learning_rate=-1.0).fit(X)
    with pytest.raises(ValueError, match="init must be"):
        TSNE(init="spectral").fit(X)
    # with good parameters the data is what is refused: there is no CPU path
    with pytest.raises(ValueError, match="must be float32"):
        TSNE().fit(X.double())
    with pytest.raises(ValueError, match="must be on the GPU"):
        TSNE().fit(X)
    with pytest.raises(ValueError, match=r"float32 \[N, D\] tensor"):
        TSNE().fit(np.zeros((100, 4), dtype=np.float32))
    assert neighbour_count(1000, 30.0) == 63 and neighbour_count(1000, 5.0) == 15 and neighbour_count(40, 30.0) == 39
    assert TSNE(perplexity=62.9)._validate(1000) == 63 and TSNE(perplexity=5)._validate(1000) == 15


NEW_ENTRIES = ("vsom_tsne_affinities", "vsom_tsne_repulsion_parts", "vsom_tsne_repulsion", "vsom_tsne_step_parts", "vsom_tsne_step")


def test_entries_in_header_signatures_and_library():
    import ctypes
    from test_abi import header_functions
    from vit_som_amd._lib import LIB_PATH, SIGNATURES
    raw = ctypes.CDLL(LIB_PATH)
    for name in NEW_ENTRIES:
        assert name in header_functions() and name in SIGNATURES and hasattr(raw, name), name
    src = open(os.path.join(ROOT, "vit_som_amd", "csrc", "build.sh")).read()
    assert src.count("tsne") == 2                            # the compile list and the link list


def test_parts_queries_are_host_arithmetic():
    from vit_som_amd._lib import lib as L
    for q, per in ((L.vsom_tsne_repulsion_parts, 64), (L.vsom_tsne_step_parts, 16)):
        assert q(0) == 0 and q(-5) == 0 and q(1) >= 1
        prev = 0
        for N in (1, 2, per - 1, per, per + 1, 257, 3000, 20011, 60000, (1 << 31) - 2):
            assert q(N) >= prev and q(N) >= (N + per - 1) // per
            prev = q(N)
    assert L.vsom_tsne_repulsion_parts(60000) == 938 and L.vsom_tsne_step_parts(60000) == 7500


P, BIG = 4096, 1 << 40           # a non-null, 16-byte aligned stand-in for a device pointer: nothing is launched or dereferenced


def test_refusals_before_any_launch():
    from vit_som_amd._lib import last_error, lib as L
    N = 257
    nz, npart = L.vsom_tsne_repulsion_parts(N), L.vsom_tsne_step_parts(N)
    rep = lambda z, n: L.vsom_tsne_repulsion(P, N, P, P, z, n, None)                                    # noqa: E731
    assert rep(P, nz - 1) == -4 and "zpart" in last_error() and "too small" in last_error()
    assert rep(P, 0) == -4 and rep(None, BIG) == -4
    assert L.vsom_tsne_repulsion(P + 8, N, P, P, P, nz, None) == -2                                     # Y not 16-byte aligned
    assert L.vsom_tsne_repulsion(None, N, P, P, P, nz, None) == -1 and L.vsom_tsne_repulsion(P, 0, P, P, P, nz, None) == -1
    assert L.vsom_tsne_repulsion(P, (1 << 31) - 1, P, P, P, BIG, None) == -3
    step = lambda z, n_z, pt, n_p: L.vsom_tsne_step(P, P, P, P, 2 * P, P, P, N, P, z, n_z, 12.0, 0.5, 200.0, 1, pt, n_p, None)   # noqa: E731
    assert step(P, nz - 1, P, npart) == -4 and "zpart" in last_error()
    assert step(None, BIG, P, npart) == -4
    assert step(P, nz, P, npart - 1) == -4 and "part" in last_error() and "too small" in last_error()
    assert step(P, nz, None, BIG) == -4 and step(P, nz, P, 0) == -4
    assert L.vsom_tsne_step(P, P, P, P, P, P, P, N, P, P, nz, 12.0, 0.5, 200.0, 1, P, npart, None) == -1 and "alias" in last_error()
    aff = lambda k, first, ldk, perp: L.vsom_tsne_affinities(P, None, ldk, N, k, first, 1, perp, P, P, P, None)       # noqa: E731
    assert aff(64, 0, 64, 30.0) == -3 and "63" in last_error()
    assert aff(0, 1, 64, 30.0) == -1 and aff(63, 1, 63, 30.0) == -1 and aff(63, 1, 64, 0.0) == -1
    assert L.vsom_tsne_affinities(None, None, 64, N, 63, 1, 1, 30.0, P, P, P, None) == -1


def test_docs_and_evidence_are_there():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "t-SNE (`tsne.hip`; `tsne.py`)" in design
    assert "TSNE" in open(os.path.join(ROOT, "README.md")).read()


# ------------------------------------------------------------------ 3. host graph
def test_joint_probabilities_of_a_hand_made_table():
    from vit_som_amd.tsne import joint_probabilities
    idx = np.array([[1, 2], [0, 2], [3, 1], [4, 2], [3, 0]], dtype=np.int64)
    cond = np.array([[0.7, 0.3], [0.6, 0.4], [0.55, 0.45], [0.9, 0.1], [0.2, 0.8]])
    Pj = joint_probabilities(idx, cond)
    assert Pj.dtype == np.float64 and Pj.shape == (5, 5) and Pj.has_sorted_indices
    for i in range(5):
        row = Pj.indices[Pj.indptr[i]:Pj.indptr[i + 1]]
        assert (np.diff(row) > 0).all() and i not in row
    D = Pj.toarray()
    assert np.array_equal(D, D.T)                            # bit for bit
    assert abs(D.sum() - 1.0) <= 1e-15 and (Pj.data > 0).all()
    want = R.joint_p(idx, cond)
    assert np.abs(D - want).max() <= 1e-16
    assert D[0, 1] == D[1, 0] and abs(D[0, 1] - (0.7 + 0.6) / 10.0) <= 1e-16       # both directions present: the sum of the two
    assert abs(D[0, 2] - 0.3 / 10.0) <= 1e-16                                      # one direction only
    with pytest.raises(ValueError):
        joint_probabilities(idx, cond[:, :1])


def test_band_file_is_what_the_generator_describes():
    """tests/golden/tsne_fit_band.json holds inputs by seed and shape, and results only."""
    band = json.load(open(os.path.join(ROOT, "tests", "golden", "tsne_fit_band.json")))
    assert band["N"] == 600 and band["D"] == 50 and band["centres"] == 6 and band["perplexity"] == 30.0 and band["max_iter"] == 1000
    for metric in ("euclidean", "cosine"):
        runs = band["runs"][metric]
        assert len(runs["kl"]) == len(runs["trustworthiness"]) == 5
        assert all(0.0 < v < 5.0 for v in runs["kl"]) and all(0.5 < v <= 1.0 for v in runs["trustworthiness"])
