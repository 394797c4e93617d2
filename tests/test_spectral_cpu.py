"""Spectral embedding without a GPU: the package's own solver loop (spectral.chebyshev_subspace) driven by a scipy operator
reaches tol on the four fixtures and agrees with dense eigh and with sklearn; the filter is the polynomial it claims to be;
the parameter and refusal sentences; the C-ABI refusals of every new entry, none of which launches; header, SIGNATURES and
wrappers agree.  Every condition the GPU fits are held to is shown here to hold for the reference alone."""
import inspect
import os
import re
import warnings

import numpy as np
import pytest
import scipy.sparse
import scipy.sparse.csgraph

import spectral_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-8
WANTED = {"moons": 3, "circles": 3, "blobs5": 6, "cube": 4, "blobs700": 4}


def _solve(name):
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        return R.solve_host(R.fixture(name)[0], WANTED[name])


# ------------------------------------------------------------------ the solver, driven by scipy
@pytest.mark.parametrize("name", R.FOUR)
def test_the_host_loop_reaches_tol_and_the_dense_spectrum(name):
    theta, V, res, passes = _solve(name)
    lam, _ = R.dense_spectrum(name)
    n = WANTED[name]
    print(name, "passes", passes, "max residual", res.max(), "max |theta - lambda|", np.abs(theta - lam[:n]).max())
    assert passes <= 10 and res.max() <= TOL
    assert np.abs(theta - lam[:n]).max() <= TOL                   # |lambda - theta| <= |r|
    M, _, _ = R.operator(R.fixture(name)[0])
    assert np.abs(V.T @ V - np.eye(n)).max() <= 1e-12
    assert np.linalg.norm(M @ V - V * theta, axis=0).max() <= TOL * (1 + 1e-6)


def test_five_unit_eigenvalues_on_the_five_component_blobs():
    A = R.fixture("blobs5")[0]
    assert scipy.sparse.csgraph.connected_components(A, directed=False)[0] == 5
    theta, V, res, _ = _solve("blobs5")
    assert np.abs(theta[:5] - 1.0).max() <= TOL and theta[5] < 0.9
    # the unit-eigenvalue subspace by its projector: spanned by sqrt(d) on each component
    labels = scipy.sparse.csgraph.connected_components(A, directed=False)[1]
    _, d, _ = R.operator(A)
    B = np.stack([np.sqrt(d) * (labels == c) for c in range(5)], axis=1)
    B /= np.linalg.norm(B, axis=0)
    assert np.abs(V[:, :5] @ V[:, :5].T - B @ B.T).max() <= TOL / (1.0 - theta[5])


@pytest.mark.parametrize("name", ["blobs700", "cube"])
def test_vectors_agree_with_sklearn_within_davis_kahan(name):
    A = R.fixture(name)[0]
    assert scipy.sparse.csgraph.connected_components(A, directed=False)[0] == 1
    n = WANTED[name]
    theta, V, res, _ = _solve(name)
    lam, _ = R.dense_spectrum(name)
    U = R.sklearn_vectors(A, n)
    for j in range(n):
        gap = np.abs(np.delete(lam, j) - lam[j]).min()
        sine = np.linalg.norm(U[:, j] - (V[:, j] @ U[:, j]) * V[:, j])
        print(name, j, "sine", sine, "bound", res.max() / gap)
        assert sine <= res.max() / gap


def test_the_filter_is_the_scaled_chebyshev_polynomial():
    from vit_som_amd import spectral as S
    A = R.fixture("circles")[0]
    M, _, _ = R.operator(A)
    lam, vec = R.dense_spectrum("circles")
    pick = [0, 5, 100, 300, 599]
    for a in (0.0, 0.7):
        got = R.filter_block(M, vec[:, pick], a, 20)
        want = vec[:, pick] * R.filter_scalar(lam[pick], a, 20)
        assert np.abs(got - want).max() <= 1e-12
        inside = lam[lam <= a]
        assert np.abs(R.filter_scalar(inside, a, 20)).max() <= abs(R.filter_scalar(np.array([a]), a, 20)[0]) * (1 + 1e-9)
        # the package's recurrence is the restatement's
        Y = np.random.RandomState(1).standard_normal((600, 5))
        bufs, keep = [np.empty_like(Y) for _ in range(3)], Y.copy()
        out, rest = S.chebyshev_filter(R.host_apply(M), Y, bufs, 5, a, 20)
        assert np.abs(out - R.filter_block(M, Y, a, 20)).max() <= 1e-12 * np.abs(out).max()
        assert np.array_equal(Y, keep) and len(rest) == 2 and all(b is not out and b is not Y for b in rest)


@pytest.mark.parametrize("N,d,k,n,seed", [(64, 8, 15, 20, 0), (40, 3, 15, 24, 2), (33, 3, 5, 24, 3)])
def test_small_dense_graphs_whose_wanted_eigenvalues_reach_below_zero(N, d, k, n, seed):
    """Fewer than l = n + 8 eigenvalues lie above 0, the first pass's lower bound: the filtered block loses rank, and the
    loop filters the kept block again with a lower bound (and, with l close to N, a lower degree) instead of failing."""
    X = np.random.RandomState(seed).standard_normal((N, d)).astype(np.float32)
    A = R.knn_affinity(X, k)
    M, _, _ = R.operator(A)
    lam = np.linalg.eigvalsh(M.toarray())[::-1]
    assert (lam > 0).sum() < min(n + 8, N)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        theta, V, res, passes = R.solve_host(A, n)
    assert passes <= 10 and res.max() <= TOL and np.abs(theta - lam[:n]).max() <= TOL


def test_a_short_run_warns_with_the_residual():
    from vit_som_amd import spectral as S
    A = R.fixture("cube")[0]
    with pytest.warns(S.ConvergenceWarning, match=r"largest residual of the 4 wanted eigenpairs is \d\.\d+e-\d+ > tol = 1\.0e-08 after 1 passes"):
        R.solve_host(A, 4, max_iter=1)


def test_sign_rule_and_eigengap():
    from vit_som_amd import spectral as S
    U = np.array([[1.0, -3.0, 0.0], [-2.0, 3.0, 0.0], [2.0, 1.0, 0.0]])
    flipped, sg = R.sign_flip(U)
    assert sg.tolist() == [-1.0, -1.0, 1.0] and flipped[1, 0] == 2.0 and flipped[0, 1] == 3.0      # ties: the first row decides
    assert S.eigengap_k([1.0, 1.0, 0.99, 0.5, 0.4]) == 3 and S.eigengap_k([1.0]) == 1


# ------------------------------------------------------------------ parameters and refusals
def test_signatures_follow_sklearn():
    import vit_som_amd as V
    se = list(inspect.signature(V.SpectralEmbedding.__init__).parameters.items())[1:]
    assert [(k, p.default) for k, p in se] == [("n_components", 2), ("affinity", "nearest_neighbors"), ("n_neighbors", None),
                                               ("metric", "euclidean"), ("random_state", None), ("eigen_solver", None),
                                               ("eigen_tol", 1e-8), ("n_jobs", None)]
    sc = list(inspect.signature(V.SpectralClustering.__init__).parameters.items())[1:]
    assert [(k, p.default) for k, p in sc][:8] == [("n_clusters", 8), ("n_components", None), ("affinity", "nearest_neighbors"),
                                                   ("n_neighbors", 10), ("metric", "euclidean"), ("n_init", 10),
                                                   ("assign_labels", "kmeans"), ("random_state", None)]
    assert list(inspect.signature(V.evaluate_spectral).parameters) == ["model", "config", "dataloader", "n_clusters", "n_neighbors",
                                                                        "metric", "max_rows"]
    from vit_som_amd import evaluation, spectral
    assert evaluation.evaluate_spectral is spectral.evaluate_spectral and evaluation.SpectralReport is spectral.SpectralReport
    assert evaluation.visualize_spectral_map is spectral.visualize_spectral_map
    assert "REFUSED" in V.SpectralEmbedding.__doc__ and "rbf" in V.SpectralEmbedding.__doc__


def test_refusal_sentences():
    import vit_som_amd as V
    A = R.fixture("circles")[0]
    with pytest.raises(ValueError, match="affinity='rbf' is a dense N x N matrix and is not offered"):
        V.SpectralEmbedding(affinity="rbf").fit(None)
    with pytest.raises(ValueError, match="affinity='rbf' is a dense N x N matrix"):
        V.SpectralClustering(2, affinity="rbf").fit(None)
    with pytest.raises(ValueError, match="affinity must be 'nearest_neighbors' or 'precomputed', got 'poly'"):
        V.SpectralEmbedding(affinity="poly").fit(None)
    for solver in ("arpack", "lobpcg", "amg"):
        with pytest.raises(ValueError, match=f"eigen_solver='{solver}' is a host solver and is not offered"):
            V.SpectralEmbedding(eigen_solver=solver).fit(None)
    with pytest.raises(ValueError, match="eigen_solver must be None or 'chebyshev'"):
        V.SpectralEmbedding(eigen_solver="power").fit(None)
    for how in ("discretize", "cluster_qr"):
        with pytest.raises(ValueError, match=f"assign_labels='{how}' is a host procedure"):
            V.SpectralClustering(2, assign_labels=how).fit(None)
    with pytest.raises(ValueError, match="n_components must be a positive integer, got 0"):
        V.SpectralEmbedding(0).fit(None)
    with pytest.raises(ValueError, match=r"n_components \+ 8 = 33 > 32"):
        V.SpectralEmbedding(24, affinity="precomputed").fit(A)
    with pytest.raises(ValueError, match="X must be a float32 .N, D. tensor on the GPU"):
        V.SpectralEmbedding().fit(np.zeros((10, 2), np.float32))
    B = A.tolil(copy=True)
    B[3, 7] = 0.25
    B[7, 3] = 0.5
    B[9, 2] = 1.0
    with pytest.raises(ValueError, match=r"not symmetric: A\[2, 9\] = .*0\.0.* but A\[9, 2\] = .*1\.0"):
        V.SpectralEmbedding(affinity="precomputed").fit(B.tocsr())
    C = A.copy()
    C.data[5] = -1.0
    with pytest.raises(ValueError, match="must be non-negative and finite"):
        V.SpectralEmbedding(affinity="precomputed").fit(C)
    with pytest.raises(ValueError, match="must be a scipy sparse matrix or a device"):
        V.SpectralEmbedding(affinity="precomputed").fit(A.toarray())
    with pytest.raises(ValueError, match="must be square"):
        V.SpectralEmbedding(affinity="precomputed").fit(A[:10])


def test_the_reference_graph_is_sklearns():
    from sklearn.neighbors import kneighbors_graph
    X = R.moons()[0]
    C = kneighbors_graph(X.astype(np.float64), 10, include_self=True)
    want = 0.5 * (C + C.T)
    assert abs(want - R.fixture("moons")[0]).max() == 0


def test_train_takes_spectral_eval_and_keeps_gmm_eval_last():
    from vit_som_amd import train
    names = list(inspect.signature(train.main).parameters)
    assert "spectral_eval" in names and names[-1] == "gmm_eval"


# ------------------------------------------------------------------ the C-ABI, without a launch
P = 4096                    # stands for a device pointer: every call below is refused before anything is launched
Q = 1 << 30                 # another one, far enough for any block of these shapes


def test_argument_refusals_without_a_launch():
    from vit_som_amd._lib import last_error, lib as L
    # degrees
    assert L.vsom_spectral_degrees(None, P, P, 10, 20, P, P, P, P, None) == -1 and "null" in last_error()
    assert L.vsom_spectral_degrees(P, None, P, 10, 20, P, P, P, P, None) == -1
    assert L.vsom_spectral_degrees(P, P, P, 0, 20, P, P, P, P, None) == -1
    assert L.vsom_spectral_degrees(P, P, P, 10, -1, P, P, P, P, None) == -1
    assert L.vsom_spectral_degrees(P, P, P, 131073, 20, P, P, P, P, None) == -3
    # spmm
    spmm = lambda **k: L.vsom_spectral_spmm(*[{**dict(indptr=P, indices=P, data=P, s=P, N=10, nnz=20, heavy=None, n_heavy=0, Y1=P,      # noqa: E731
                                                      Y0=None, Yout=Q, ld=4, l=4, alpha=1.0, c=0.0, beta=0.0, stream=None), **k}[a]
                                              for a in ("indptr", "indices", "data", "s", "N", "nnz", "heavy", "n_heavy", "Y1", "Y0",
                                                        "Yout", "ld", "l", "alpha", "c", "beta", "stream")])
    assert spmm(Y1=None) == -1 and spmm(Yout=None) == -1 and spmm(s=None) == -1 and spmm(data=None) == -1
    assert spmm(l=0) == -1 and spmm(ld=3) == -1 and spmm(N=0) == -1
    assert spmm(l=33, ld=33) == -3 and "l <= 32" in last_error()
    assert spmm(N=131073) == -3
    assert spmm(n_heavy=1) == -1 and spmm(n_heavy=-1, heavy=P) == -1 and spmm(n_heavy=11, heavy=P) == -1
    assert spmm(Yout=P) == -1 and "overlaps" in last_error()
    assert spmm(Yout=P + 8 * (9 * 4 + 3)) == -1                   # the last element of Y1 is the first of Yout
    assert spmm(Y0=Q + 8) == -1 and "overlaps" in last_error()
    # the workspace of gram and residual
    assert L.vsom_spectral_ws_size(1000, 16, 4) == 4 * 2 * 16 * 16 * 8          # 4 slabs of 256 rows
    assert L.vsom_spectral_ws_size(1000, 16, 1000) == 16 * 2 * 16 * 16 * 8      # slabs are multiples of 64 rows: 16 of them
    assert L.vsom_spectral_ws_size(1, 1, 1) == 16
    for bad in ((0, 4, 1), (10, 0, 1), (10, 33, 1), (10, 4, 0), (10, 4, 1025), (131073, 4, 1)):
        assert L.vsom_spectral_ws_size(*bad) == 0
    need = L.vsom_spectral_ws_size(1000, 16, 4)
    gram = lambda ws, n, **k: L.vsom_spectral_gram(P, k.get("W"), 16, 1000, k.get("l", 16), k.get("slabs", 4), P, k.get("H"), ws, n, None)  # noqa: E731
    assert gram(Q, need - 1) == -4 and "too small" in last_error() and "vsom_spectral_gram" in last_error()
    assert gram(Q, 0) == -4 and gram(None, 1 << 40) == -4
    assert gram(Q + 4, need) == -2
    assert gram(Q, need, W=P) == -1 and gram(Q, need, H=P) == -1
    assert gram(Q, need, slabs=0) == -1 and gram(Q, need, slabs=1025) == -1
    assert gram(Q, need, l=33) in (-1, -3)
    resid = lambda ws, n, **k: L.vsom_spectral_residual(P, k.get("W", P), 16, 1000, 16, k.get("theta", P), 4, P, ws, n, None)      # noqa: E731
    assert resid(Q, need - 1) == -4 and "too small" in last_error() and "vsom_spectral_residual" in last_error()
    assert resid(Q, 0) == -4 and resid(None, 1 << 40) == -4 and resid(Q + 4, need) == -2
    assert resid(Q, need, theta=None) == -1 and resid(Q, need, W=None) == -1
    # rotate
    assert L.vsom_spectral_rotate(P, 8, 100, 8, P, 8, P, 8, None) == -1 and "overlaps" in last_error()
    assert L.vsom_spectral_rotate(P, 8, 100, 8, None, 8, Q, 8, None) == -1
    assert L.vsom_spectral_rotate(P, 8, 100, 8, P, 33, Q, 33, None) == -3
    assert L.vsom_spectral_rotate(P, 8, 100, 8, P, 4, Q, 3, None) == -1
    # embed
    assert L.vsom_spectral_embed(P, 8, P, 100, 7, 2, Q, 2, P, None) == -1         # columns [7, 9) of 8
    assert L.vsom_spectral_embed(P, 8, P, 100, 0, 2, Q, 1, P, None) == -1
    assert L.vsom_spectral_embed(P, 8, None, 100, 0, 2, Q, 2, P, None) == -1
    assert L.vsom_spectral_embed(P, 40, P, 100, 31, 2, Q, 2, P, None) == -3
    assert L.vsom_spectral_embed(P, 8, P, 131073, 0, 2, Q, 2, P, None) == -3


def test_header_signatures_wrappers_and_build_agree():
    from vit_som_amd import ops
    from vit_som_amd._lib import SIGNATURES
    src = open(os.path.join(ROOT, "include", "vitsom_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = {name: params for name, params in re.findall(r"\b(vsom_spectral_[a-z0-9_]+)\s*\(([^)]*)\)", src)}
    assert sorted(declared) == ["vsom_spectral_degrees", "vsom_spectral_embed", "vsom_spectral_gram", "vsom_spectral_residual",
                                "vsom_spectral_rotate", "vsom_spectral_spmm", "vsom_spectral_ws_size"]
    ops_src = inspect.getsource(ops)
    for name, params in declared.items():
        assert len(SIGNATURES[name][1]) == len(params.split(",")), name
        assert callable(getattr(ops, name[5:])) and f"lib.{name}(" in ops_src, name
        assert not re.search(r"\b(ws_bytes|part_bytes|planes_bytes|scratch_bytes)\b", params), name
    # the wrappers stand at the end of ops.py, after the DBSCAN ones
    assert ops_src.index("def spectral_degrees") > ops_src.index("def dbscan_finish")
    hip = open(os.path.join(ROOT, "vit_som_amd", "csrc", "spectral.hip")).read()
    assert "aligned16(" not in hip and "& 15" not in hip and "atomicAdd(float" not in hip
    build = open(os.path.join(ROOT, "vit_som_amd", "csrc", "build.sh")).read()
    assert build.count("spectral") == 2
