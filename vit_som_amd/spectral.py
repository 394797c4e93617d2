"""Spectral embedding and spectral clustering on the device (sklearn.manifold.SpectralEmbedding and
sklearn.cluster.SpectralClustering's interface; no counterpart in the reference).

The graph is a symmetric affinity A in CSR whose diagonal is ignored; d are its row sums, s = d^-1/2 and
M = diag(s) A diag(s), with spectrum in [-1, 1].  Wanted are the n largest eigenvalues of M, the n smallest of the
normalised Laplacian I - M.  The graph is assembled on the host, as the UMAP and t-SNE graphs are, and copied to the device
once; after that only [l, l] matrices and one [l] record cross per pass.  Everything on the device is fp64
(csrc/spectral.hip): eigenvalues 1e-4 apart do not survive an f32 basis, and the product is bound by its gathers, not by
its arithmetic.  A fit is bitwise reproducible for a given ``random_state``.

The solver (`chebyshev_subspace`) is Chebyshev-filtered subspace iteration (Zhou and Saad 2007), a block method, so it finds
repeated eigenvalues -- a graph of c components has c eigenvalues 1 and all of them are returned:

1. Block width l = n + 8.  Column 0 starts at sqrt(d), the eigenvector of eigenvalue 1 of a connected graph; the other
   columns are normal draws from the estimator's RandomState.  The block is orthonormalised (step 3).
2. One pass filters the block with the scaled Chebyshev polynomial of degree m that damps [-1, a] and is 1 at 1:
   c = (a - 1) / 2, e = (a + 1) / 2, sigma_1 = e / (1 - c); Y_1 = (sigma_1 / e) (M - c) Y_0;
   Y_{i+1} = 2 (sigma_{i+1} / e) (M - c) Y_i - sigma_i sigma_{i+1} Y_{i-1} with sigma_{i+1} = 1 / (2 / sigma_1 - sigma_i).
   Each step is one vsom_spectral_spmm.  a = 0 in the first pass, afterwards the smallest Ritz value of the block, held
   inside [-0.9, 1 - 1e-9] (e = 0 at a = -1).  The smallest Ritz value of an l-dimensional space is at most the l-th
   eigenvalue, so it never cuts into the wanted ones; the first pass's 0 can -- a small dense graph has fewer than l
   eigenvalues above 0 -- and then the filtered block loses rank (step 3 drops directions): a is moved halfway to -1 and
   the block, which the filter only reads, is filtered again, until the block keeps its width or a is -0.9; a block
   that spans most of the spectrum (l close to N) then gets half the degree for that pass, down to 1.
3. Orthonormalise by Gram and rotate: G = Y^T Y on the device, T from pca.orthonormalising_transform on the host (the
   symmetric inverse square root of the scaled Gram matrix: the columns stay with their Ritz vectors), V = Y T^T.
4. W = M V, then G = V^T V and H = V^T W in one launch.  The [l, l] Ritz problem is solved on the host in fp64 with V's
   remaining departure from orthonormality folded in: R = orthonormalising_transform(G), (theta, S) = pca.ritz(R H R^T),
   and the rotation applied to V and W is R^T S.
5. Residuals |W_j - theta_j V_j| from the differences themselves (vsom_spectral_residual), not from Gram entries, which
   cancel at 1e-16 and floor the residual at 1e-8.  Stop when the largest of the n wanted is <= tol.  |lambda - theta| <=
   |r| for a unit Ritz vector, so the eigenvalues are then within tol.

Departures from sklearn: `affinity="rbf"` (its default, a dense N x N matrix) and the solvers "arpack", "lobpcg" and "amg"
are refused with the reason; `metric` is an addition; N <= 131 072 and n_components + 8 <= 32.
"""
import numbers
import time
import warnings
from dataclasses import dataclass

import numpy as np
import scipy.sparse
import scipy.sparse.csgraph
import torch

from . import ops
from .pca import orthonormalising_transform, ritz

OVERSAMPLE = 8
MAX_N = ops.SPECTRAL_MAX_N
MAX_WIDTH = ops.SPECTRAL_MAX_WIDTH
METRICS = {"euclidean": ops.DIST_EUCLIDEAN, "cosine": ops.DIST_COSINE}
A_MIN, A_MAX = -0.9, 1.0 - 1e-9
DISCONNECTED = "Graph is not fully connected, spectral embedding may not work as expected."


class ConvergenceWarning(UserWarning):
    """The solver stopped at max_iter with a residual above tol (sklearn.exceptions.ConvergenceWarning's name)."""


# ------------------------------------------------------------------------------------ the solver
def chebyshev_filter(apply, Y, bufs, w, a, degree):
    """Step 2 on the first w columns of Y, which is only read, through three buffers of its shape -> (the buffer that holds
    the filtered block, the other two).  apply(Y1, Y0, alpha, c, beta, out) writes alpha (M Y1 - c Y1) - beta Y0 (Y0 may be
    None) into out and returns it."""
    c, e = (a - 1.0) / 2.0, (a + 1.0) / 2.0
    sigma1 = e / (1.0 - c)
    sigma = sigma1
    y0, y1, spare = Y, bufs[0], [bufs[1], bufs[2]]
    apply(Y[:, :w], None, sigma1 / e, c, 0.0, y1[:, :w])
    for _ in range(2, degree + 1):
        new = 1.0 / (2.0 / sigma1 - sigma)
        out = spare.pop(0)
        apply(y1[:, :w], y0[:, :w], 2.0 * new / e, c, sigma * new, out[:, :w])
        if y0 is not Y:
            spare.append(y0)
        y0, y1, sigma = y1, out, new
    return y1, [b for b in bufs if b is not y1]


def chebyshev_subspace(apply, dense, Y, n, tol=1e-8, degree=20, max_iter=60):
    """Steps 1-5 from the start block Y [N, l] -> (theta [l'] descending, V [N, l'] the Ritz vectors, residual norms [l'],
    passes).  `dense` supplies the block's dense algebra: empty_like(Y), grams(V, W or None) -> host (G, H),
    rotate(V, T [l, l_out] host, out) -> out[:, :l_out] = V T, residual(V, W, theta host) -> host squared norms.  The device
    and a scipy operator on the host run this same loop.  Four buffers of Y's shape are all the loop holds."""
    w = Y.shape[1]
    if not 1 <= n <= w:
        raise ValueError(f"chebyshev_subspace: n = {n} wanted of a block of {w}")

    def transform(src, w):
        T = orthonormalising_transform(dense.grams(src[:, :w], None)[0])      # [w_out, w]: the rows of T src^T are orthonormal
        if T.shape[0] < n:
            raise np.linalg.LinAlgError(f"chebyshev_subspace: the block spans {T.shape[0]} directions, {n} are wanted")
        return np.ascontiguousarray(T.T)

    Vb, free = dense.empty_like(Y), [Y, dense.empty_like(Y), dense.empty_like(Y)]
    T = transform(Y, w)
    dense.rotate(Y[:, :w], T, Vb)
    w = T.shape[1]
    a, theta, res = 0.0, None, None
    for it in range(1, max_iter + 1):
        m = degree
        while True:
            Yb, (f0, f1) = chebyshev_filter(apply, Vb, free, w, a, m)
            try:
                T = transform(Yb, w)
            except np.linalg.LinAlgError:
                if a <= A_MIN and m == 1:
                    raise
                T = None
            if T is not None and (T.shape[1] == w or (a <= A_MIN and m == 1)):
                break
            if a > A_MIN:                              # the filter cut into the block itself: damp less, filter V again
                a = max(A_MIN, (a - 1.0) / 2.0)
            else:                                      # the block spans most of the spectrum: a weaker polynomial for this pass
                m = max(1, m // 2)
        Q = dense.rotate(Yb[:, :w], T, f0)
        w = T.shape[1]
        W = apply(Q, None, 1.0, 0.0, 0.0, f1[:, :w])
        G, H = dense.grams(Q, W)
        R = orthonormalising_transform(G)                          # Q's remaining departure from orthonormality
        theta, S, _ = ritz(R @ H @ R.T, np.eye(R.shape[0]))
        T = np.ascontiguousarray(R.T @ S)
        V = dense.rotate(Q, T, Vb)                                 # the block before the filter is no longer needed
        W = dense.rotate(W, T, Yb)
        w = T.shape[1]
        res = np.sqrt(np.maximum(dense.residual(V, W, theta), 0.0))
        free = [f0, f1, Yb]
        if float(res[:n].max()) <= tol:
            break
        a = min(max(float(theta[-1]), A_MIN), A_MAX)
    else:
        warnings.warn(f"spectral: the largest residual of the {n} wanted eigenpairs is {float(res[:n].max()):.3e} > tol = {tol:.1e} "
                      f"after {max_iter} passes of degree {degree}", ConvergenceWarning)
    return theta, Vb[:, :w], res, it


# ------------------------------------------------------------------------------------ the graph on the device
class DeviceGraph:
    """A CSR affinity on the device with its degrees: indptr / indices int64, data fp64, d, s = d^-1/2 fp64 [N], the list of
    long rows.  Refuses, with ValueError, what vsom_spectral_degrees counts as bad."""

    def __init__(self, indptr, indices, data, who="spectral"):
        dev = indptr.device
        N = indptr.shape[0] - 1
        self.indptr, self.indices, self.data, self.N = indptr, indices, data, N
        self.d = torch.empty(N, dtype=torch.float64, device=dev)
        self.s = torch.empty(N, dtype=torch.float64, device=dev)
        self.heavy = torch.empty(N, dtype=torch.int32, device=dev)
        status = torch.empty(ops.SPECTRAL_STATUS, dtype=torch.int64, device=dev)
        ops.spectral_degrees(indptr, indices, data, self.d, self.s, self.heavy, status)
        st = status.tolist()
        if st[ops.SPECTRAL_BAD_INDPTR] or st[ops.SPECTRAL_BAD_INDEX]:
            raise ValueError(f"{who}: the CSR matrix is malformed ({st[ops.SPECTRAL_BAD_INDPTR]} bad indptr pairs, "
                             f"{st[ops.SPECTRAL_BAD_INDEX]} indices outside [0, {N}))")
        if st[ops.SPECTRAL_BAD_WEIGHT]:
            raise ValueError(f"{who}: the affinity matrix has {st[ops.SPECTRAL_BAD_WEIGHT]} entries that are negative or not finite")
        self.n_isolated, self.n_heavy = st[ops.SPECTRAL_ISOLATED], st[ops.SPECTRAL_HEAVY]
        if self.n_heavy:                                          # a fixed order, so that the launch is the same every fit
            self.heavy[:self.n_heavy] = torch.sort(self.heavy[:self.n_heavy]).values

    @classmethod
    def from_scipy(cls, A, device, who="spectral"):
        A = scipy.sparse.csr_matrix(A, dtype=np.float64)
        A.sort_indices()
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(device)      # noqa: E731
        return cls(t(A.indptr, np.int64), t(A.indices, np.int64), t(A.data, np.float64), who)

    def apply(self, Y1, Y0, alpha, c, beta, out):
        return ops.spectral_spmm(self.indptr, self.indices, self.data, self.s, Y1, Y0, out, alpha, c, beta,
                                 self.heavy if self.n_heavy else None, self.n_heavy)


class _DeviceDense:
    """chebyshev_subspace's dense algebra on fp64 device blocks."""

    @staticmethod
    def empty_like(Y):
        return torch.empty(Y.shape[0], Y.shape[1], dtype=torch.float64, device=Y.device)

    @staticmethod
    def grams(V, W):
        l = V.shape[1]
        GH = torch.empty(2, l, l, dtype=torch.float64, device=V.device)
        ops.spectral_gram(V, W, GH[0], GH[1] if W is not None else None)
        GH = GH.cpu().numpy()
        return GH[0], (GH[1] if W is not None else None)

    @staticmethod
    def rotate(V, T, out):
        return ops.spectral_rotate(V, torch.from_numpy(np.ascontiguousarray(T, dtype=np.float64)).to(V.device), out[:, :T.shape[1]])

    @staticmethod
    def residual(V, W, theta):
        l = V.shape[1]
        out = torch.empty(l, dtype=torch.float64, device=V.device)
        ops.spectral_residual(V, W, torch.from_numpy(np.ascontiguousarray(theta[:l], dtype=np.float64)).to(V.device), out)
        return out.cpu().numpy()


def _random_state(seed):
    if seed is None or seed is np.random:
        return np.random.mtrand._rand
    if isinstance(seed, np.random.RandomState):
        return seed
    if isinstance(seed, numbers.Integral) and not isinstance(seed, bool):
        return np.random.RandomState(int(seed))
    raise ValueError(f"{seed!r} cannot be used to seed a numpy.random.RandomState instance")


def start_block(d, l, rs):
    """Step 1's block on the host: column 0 = sqrt(d), the others normal draws."""
    Y = np.empty((d.shape[0], l))
    Y[:, 0] = np.sqrt(d)
    if not Y[:, 0].any():
        Y[:, 0] = 1.0
    Y[:, 1:] = rs.standard_normal((d.shape[0], l - 1))
    return Y


def solve(graph, n, random_state=None, tol=1e-8, degree=20, max_iter=60):
    """The n leading eigenpairs of M for a DeviceGraph -> (theta [n] host descending, V fp64 [N, n] device view, residuals
    [n] host, passes)."""
    if n + OVERSAMPLE > MAX_WIDTH:
        raise ValueError(f"spectral: n_components + {OVERSAMPLE} = {n + OVERSAMPLE} > {MAX_WIDTH}, the widest block the kernels take")
    l = min(n + OVERSAMPLE, graph.N)
    if n > l:
        raise ValueError(f"spectral: {n} eigenvectors wanted of a graph of {graph.N} rows")
    Y = torch.from_numpy(start_block(graph.d.cpu().numpy(), l, _random_state(random_state))).to(graph.d.device)
    theta, V, res, it = chebyshev_subspace(graph.apply, _DeviceDense, Y, n, tol, degree, max_iter)
    return theta[:n], V[:, :n], res[:n], it


# ------------------------------------------------------------------------------------ the affinity
def _check_x(X, who):
    if not isinstance(X, torch.Tensor) or X.dim() != 2 or not X.is_cuda or X.dtype != torch.float32:
        raise ValueError(f"{who}: X must be a float32 [N, D] tensor on the GPU")
    return X if X.stride(1) == 1 else X.contiguous()


def knn_affinity(X, n_neighbors, metric="euclidean", who="spectral"):
    """sklearn's "nearest_neighbors" affinity: 0.5 (C + C^T) with C the kNN connectivity, the row itself included, from
    vsom_umap_knn's table -> scipy CSR float64 on the host."""
    if not isinstance(metric, str) or metric not in METRICS:
        raise ValueError(f"{who}: metric must be one of {sorted(METRICS)}, got {metric!r}")
    N = X.shape[0]
    k = n_neighbors
    if isinstance(k, bool) or not isinstance(k, numbers.Integral) or k < 1:
        raise ValueError(f"{who}: n_neighbors must be a positive integer, got {k!r}")
    if k > ops.UMAP_MAX_K or k >= N:
        raise ValueError(f"{who}: n_neighbors = {k} must be at most {ops.UMAP_MAX_K} (the exact search keeps one list entry per "
                         f"lane) and below the number of rows, {N}")
    idx = torch.empty(N, int(k), dtype=torch.int64, device=X.device)
    dist = torch.empty(N, int(k), dtype=torch.float32, device=X.device)
    ops.umap_knn(X, int(k), METRICS[metric], idx, dist)
    idx = idx.cpu().numpy()
    if (idx < 0).any():
        raise ValueError(f"{who}: X has rows without neighbours (a value that is not finite)")
    C = scipy.sparse.csr_matrix((np.ones(N * k), idx.ravel(), np.arange(0, N * k + 1, k)), shape=(N, N))
    A = (0.5 * (C + C.T)).tocsr()
    A.sort_indices()
    return A


def check_affinity(A, who="spectral"):
    """A precomputed affinity on the host: square, non-negative, finite, symmetric -> CSR float64.  An asymmetric matrix is
    refused with its first offending pair."""
    if not scipy.sparse.issparse(A):
        raise ValueError(f"{who}: a precomputed affinity must be a scipy sparse matrix or a device (indptr, indices, data) triple; "
                         f"a dense N x N matrix is what this estimator avoids")
    A = scipy.sparse.csr_matrix(A, dtype=np.float64)
    if A.shape[0] != A.shape[1]:
        raise ValueError(f"{who}: the affinity matrix must be square, got {A.shape}")
    A.sum_duplicates()
    A.sort_indices()
    if A.nnz and (not np.isfinite(A.data).all() or (A.data < 0).any()):
        raise ValueError(f"{who}: the affinity matrix must be non-negative and finite")
    D = (A - A.T).tocoo()
    bad = np.abs(D.data) > 1e-10
    if bad.any():
        order = np.lexsort((D.col[bad], D.row[bad]))[0]
        i, j = int(D.row[bad][order]), int(D.col[bad][order])
        raise ValueError(f"{who}: the affinity matrix is not symmetric: A[{i}, {j}] = {A[i, j]!r} but A[{j}, {i}] = {A[j, i]!r}")
    return A


def _triple_to_scipy(triple, who):
    indptr, indices, data = triple
    for t, name, dt in ((indptr, "indptr", torch.int64), (indices, "indices", torch.int64), (data, "data", torch.float64)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dt or t.dim() != 1:
            raise ValueError(f"{who}: {name} of a device triple must be a 1-D {str(dt)[6:]} tensor on the GPU")
    N = indptr.shape[0] - 1
    try:
        return scipy.sparse.csr_matrix((data.cpu().numpy(), indices.cpu().numpy(), indptr.cpu().numpy()), shape=(N, N))
    except ValueError as e:
        raise ValueError(f"{who}: the device triple is not a CSR matrix ({e})") from None


class _Fit:
    """What the two estimators and evaluate_spectral share: the graph, its components, the eigenpairs."""

    def __init__(self, X, affinity, n_neighbors, metric, n, random_state, eigen_solver, tol, who):
        if eigen_solver not in (None, "chebyshev"):
            if eigen_solver in ("arpack", "lobpcg", "amg"):
                raise ValueError(f"{who}: eigen_solver={eigen_solver!r} is a host solver and is not offered; the device solver is "
                                 f"'chebyshev' (Chebyshev-filtered subspace iteration), also taken for None")
            raise ValueError(f"{who}: eigen_solver must be None or 'chebyshev', got {eigen_solver!r}")
        if affinity == "rbf":
            raise ValueError(f"{who}: affinity='rbf' is a dense N x N matrix and is not offered; pass affinity='nearest_neighbors' "
                             f"(the default here) or a sparse 'precomputed' affinity")
        if affinity not in ("nearest_neighbors", "precomputed"):
            raise ValueError(f"{who}: affinity must be 'nearest_neighbors' or 'precomputed', got {affinity!r}")
        if isinstance(n, bool) or not isinstance(n, numbers.Integral) or n < 1:
            raise ValueError(f"{who}: n_components must be a positive integer, got {n!r}")
        if isinstance(tol, str) or not tol > 0:
            raise ValueError(f"{who}: eigen_tol must be a positive number, got {tol!r}")
        if n + OVERSAMPLE > MAX_WIDTH:
            raise ValueError(f"{who}: n_components + {OVERSAMPLE} = {n + OVERSAMPLE} > {MAX_WIDTH}, the widest block the kernels take")
        if affinity == "precomputed":
            if isinstance(X, (tuple, list)) and len(X) == 3:
                device = X[0].device if isinstance(X[0], torch.Tensor) else None
                A = check_affinity(_triple_to_scipy(X, who), who)
            else:
                A = check_affinity(X, who)
                device = torch.device("cuda", torch.cuda.current_device())
            self.n_neighbors = None
        else:
            X = _check_x(X, who)
            device = X.device
            self.n_neighbors = max(X.shape[0] // 10, 1) if n_neighbors is None else n_neighbors
            A = knn_affinity(X, self.n_neighbors, metric, who)
        N = A.shape[0]
        if N > MAX_N:
            raise ValueError(f"{who}: N = {N} rows > {MAX_N}")
        if n > N:
            raise ValueError(f"{who}: {n} eigenvectors wanted of a graph of {N} rows")
        self.affinity, self.N, self.device = A, N, device
        self.n_components_connected = int(scipy.sparse.csgraph.connected_components(A, directed=False)[0])
        if self.n_components_connected > 1:
            warnings.warn(DISCONNECTED, UserWarning)
        self.graph = DeviceGraph.from_scipy(A, device, who)
        self.theta, self.V, self.res, self.passes = solve(self.graph, int(n), random_state, float(tol))

    def embed(self, first, n):
        E = torch.empty(self.N, n, dtype=torch.float32, device=self.device)
        sign = torch.empty(n, dtype=torch.float64, device=self.device)
        ops.spectral_embed(self.V, self.graph.s, first, E, sign)
        return E

    def f64(self, a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.device)


# ------------------------------------------------------------------------------------ the estimators
class SpectralEmbedding:
    """sklearn.manifold.SpectralEmbedding on the device: fit / fit_transform.

    NOT sklearn's default affinity: ``affinity="rbf"``, sklearn's default, is a dense N x N matrix and is REFUSED with that
    reason; the default here is ``"nearest_neighbors"`` -- 0.5 (C + C^T) of the kNN connectivity with the row itself included,
    sklearn's construction on the exact device search (``metric``: "euclidean" or "cosine", an addition) -- or
    ``"precomputed"``: a scipy sparse matrix, or a device (indptr int64, indices int64, data float64) CSR triple, symmetric
    and non-negative (an asymmetric matrix is refused with its first offending pair).  ``eigen_solver`` None or "chebyshev";
    "arpack", "lobpcg" and "amg" are refused.  N <= 131 072, n_components + 1 + 8 <= 32.  ``n_jobs`` is accepted and ignored.

    Fitted: ``embedding_`` f32 [N, n_components] on the device (sklearn's: the first vector dropped, u = D^-1/2 x, sklearn's
    deterministic sign); ``vectors_`` fp64 [N, n_components + 1] on the device, the unit eigenvectors of
    M = D^-1/2 A D^-1/2 before scaling, signs and rounding, the first one included; ``eigenvalues_`` fp64 [n_components + 1]
    on the device, those of M, descending (1 - them are the Laplacian's); ``residuals_`` likewise, |M v - theta v|;
    ``n_iter_`` passes; ``affinity_matrix_`` scipy CSR; ``n_neighbors_``; ``n_connected_components_``.  A disconnected
    graph draws sklearn's warning and the fit continues."""

    def __init__(self, n_components=2, affinity="nearest_neighbors", n_neighbors=None, metric="euclidean", random_state=None,
                 eigen_solver=None, eigen_tol=1e-8, n_jobs=None):
        self.n_components, self.affinity, self.n_neighbors, self.metric = n_components, affinity, n_neighbors, metric
        self.random_state, self.eigen_solver, self.eigen_tol, self.n_jobs = random_state, eigen_solver, eigen_tol, n_jobs

    def fit(self, X, y=None):
        who = "SpectralEmbedding"
        k = self.n_components
        if isinstance(k, bool) or not isinstance(k, numbers.Integral) or k < 1:
            raise ValueError(f"{who}: n_components must be a positive integer, got {k!r}")
        f = _Fit(X, self.affinity, self.n_neighbors, self.metric, int(k) + 1, self.random_state, self.eigen_solver, self.eigen_tol, who)
        self.embedding_ = f.embed(1, int(k))
        self.vectors_, self.eigenvalues_, self.residuals_ = f.V, f.f64(f.theta), f.f64(f.res)
        self.n_iter_, self.affinity_matrix_, self.n_neighbors_ = f.passes, f.affinity, f.n_neighbors
        self.n_connected_components_ = f.n_components_connected
        return self

    def fit_transform(self, X, y=None):
        return self.fit(X).embedding_


class SpectralClustering:
    """sklearn.cluster.SpectralClustering on the device: the spectral embedding WITHOUT dropping the first vector, as sklearn
    does, then the project's KMeans on its rows.  ``affinity`` as in SpectralEmbedding -- "rbf", sklearn's default, is
    REFUSED -- with sklearn's n_neighbors = 10; ``n_components`` None takes n_clusters; ``assign_labels`` "kmeans" only:
    "discretize" and "cluster_qr" are refused with the reason.  Fitted: ``labels_`` int64 [N] on the device,
    ``affinity_matrix_``, ``embedding_`` f32 [N, n_components], ``eigenvalues_``, ``residuals_``, ``n_iter_``,
    ``n_connected_components_``."""

    def __init__(self, n_clusters=8, n_components=None, affinity="nearest_neighbors", n_neighbors=10, metric="euclidean", n_init=10,
                 assign_labels="kmeans", random_state=None, eigen_solver=None, eigen_tol=1e-8, n_jobs=None):
        self.n_clusters, self.n_components, self.affinity, self.n_neighbors = n_clusters, n_components, affinity, n_neighbors
        self.metric, self.n_init, self.assign_labels, self.random_state = metric, n_init, assign_labels, random_state
        self.eigen_solver, self.eigen_tol, self.n_jobs = eigen_solver, eigen_tol, n_jobs

    def fit(self, X, y=None):
        from .kmeans import KMeans
        who = "SpectralClustering"
        if self.assign_labels != "kmeans":
            if self.assign_labels in ("discretize", "cluster_qr"):
                raise ValueError(f"{who}: assign_labels={self.assign_labels!r} is a host procedure on the whole embedding and is not "
                                 f"offered; 'kmeans' runs on the device")
            raise ValueError(f"{who}: assign_labels must be 'kmeans', got {self.assign_labels!r}")
        kc = self.n_clusters
        if isinstance(kc, bool) or not isinstance(kc, numbers.Integral) or kc < 1:
            raise ValueError(f"{who}: n_clusters must be a positive integer, got {kc!r}")
        n = kc if self.n_components is None else self.n_components
        rs = _random_state(self.random_state)
        f = _Fit(X, self.affinity, self.n_neighbors, self.metric, n, rs, self.eigen_solver, self.eigen_tol, who)
        self.embedding_ = f.embed(0, int(n))
        seed = int(rs.randint(np.iinfo(np.int32).max))
        self.labels_ = KMeans(n_clusters=int(kc), n_init=int(self.n_init), random_state=seed).fit(self.embedding_).labels_.to(torch.int64)
        self.eigenvalues_, self.residuals_, self.n_iter_ = f.f64(f.theta), f.f64(f.res), f.passes
        self.affinity_matrix_, self.n_connected_components_ = f.affinity, f.n_components_connected
        return self

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_


def eigenmap_device(G, dim, device, tol=1e-8):
    """UMAP's step 7 on one connected graph G (scipy sparse, symmetric): the eigenvectors of eigenvalues 2..dim+1 of
    I - D^-1/2 G D^-1/2 -> float64 [N, dim] on the host, from the device solver with a fixed start (seed 0)."""
    A = scipy.sparse.csr_matrix(G, dtype=np.float64)
    A.sort_indices()
    with warnings.catch_warnings():
        warnings.simplefilter("error", ConvergenceWarning)
        _, V, _, _ = solve(DeviceGraph.from_scipy(A, device, "UMAP"), dim + 1, 0, tol)
    return V[:, 1:].cpu().numpy()


# ------------------------------------------------------------------------------------ the latents' spectral clusters
@dataclass
class SpectralReport:
    """Host values of one evaluate_spectral pass (labels and the embedding stay on the device)."""
    n_clusters: int
    n_neighbors: int
    metric: str
    purity: float
    nmi: float
    eigenvalues: np.ndarray              # float64, the leading eigenvalues of D^-1/2 A D^-1/2, descending
    eigengap_k: int                      # the k after which the largest gap of `eigenvalues` lies
    n_connected_components: int
    n_iter: int
    max_residual: float
    labels: torch.Tensor                 # int64 [N] on the device, loader order
    embedding: torch.Tensor              # f32 [N, n_clusters] on the device
    n_samples: int
    graph_time: float
    solver_time: float
    inference_time: float


def eigengap_k(eigenvalues):
    """The number of leading eigenvalues before the largest gap of a descending spectrum (1 for fewer than two values)."""
    ev = np.asarray(eigenvalues, np.float64)
    return int(np.argmax(ev[:-1] - ev[1:])) + 1 if ev.size > 1 else 1


@torch.no_grad()
def evaluate_spectral(model, config, dataloader, n_clusters=None, n_neighbors=15, metric=None, max_rows=None):
    """Spectral clustering of the latents the SOM layer sees (the rows of evaluate_silhouette) -> SpectralReport: purity and
    NMI against the loader's labels at k = n_clusters (None: data.num_classes, the number of distinct labels when the config
    has none), the leading eigenvalues of the kNN graph,
    the k its largest eigengap suggests and its number of components.  metric: "cosine" or "euclidean"; None takes the
    SOM's distance_fcn when it is one of the two and "euclidean" otherwise.  At most max_rows rows (the first ones).
    model.world_size > 1 is refused with ValueError, like the linear probe: there is no sharded fit."""
    from . import evaluation as E
    who = "evaluate_spectral"
    if E._world(model) > 1:
        raise ValueError(f"{who}: model.world_size > 1 is not supported; run it on one rank")
    som = model.som_layer
    if metric is None:
        metric = som.distance_fcn if som.distance_fcn in ("cosine", "euclidean") else "euclidean"
    if metric not in METRICS:
        raise ValueError(f"{who}: metric must be one of {sorted(METRICS)}, got {metric!r}")
    from .kmeans import KMeans
    start = time.time()
    arch = E._Arch(model, config, who).require("som_input")
    X, y = E._whole_set(arch, dataloader, lambda x: arch.som_input(x)[0], labels=True)
    if max_rows is not None:
        X, y = X[:int(max_rows)].contiguous(), y[:int(max_rows)].contiguous()
    N = X.shape[0]
    k = int(config["data"].get("num_classes", 0)) if n_clusters is None else int(n_clusters)
    if k < 1:                                                     # a clustering config: the distinct labels, as evaluate_kmeans counts them
        hist = E._Table(1, E._label_count(config, None, True), X.device)
        hist.add(torch.zeros_like(y), y)
        k = int((hist.numpy() > 0).sum())
    n = max(min(2 * k, MAX_WIDTH - OVERSAMPLE, N), k)             # eigenvalues past k, for the gap
    t0 = time.time()
    with warnings.catch_warnings():
        warnings.filterwarnings("ignore", message=DISCONNECTED)
        f = _Fit(X, "nearest_neighbors", int(n_neighbors), metric, n, 0, None, 1e-8, who)
    torch.cuda.synchronize()
    t1 = time.time()
    emb = f.embed(0, k)
    labels = KMeans(n_clusters=k, n_init=10, random_state=0).fit(emb).labels_.to(torch.int64)
    table = E._Table(k, E._label_count(config, None, True), X.device)
    table.add(labels, y)
    w = table.numpy()
    purity, nmi = E.purity_from_table(w), E.nmi_from_table(w)
    inference_time = time.time() - start
    report = SpectralReport(n_clusters=k, n_neighbors=int(n_neighbors), metric=metric, purity=purity, nmi=nmi,
                            eigenvalues=np.asarray(f.theta, np.float64), eigengap_k=eigengap_k(f.theta),
                            n_connected_components=f.n_components_connected, n_iter=f.passes, max_residual=float(f.res.max()),
                            labels=labels, embedding=emb, n_samples=N, graph_time=float(t0 - start), solver_time=float(t1 - t0),
                            inference_time=float(inference_time))
    print(f"Spectral ({metric}, {n_neighbors} neighbours, k {k}): Purity (spectral): {purity:.3f}, NMI (spectral): {nmi:.3f}, "
          f"eigengap k {report.eigengap_k}, {report.n_connected_components} components, Inference Time: {inference_time:.3f}")
    return report


@torch.no_grad()
def visualize_spectral_map(model, config, dataloader, n_neighbors=15, metric=None, epoch=0,
                           output_dir="experiments/plots/vit_som/spectral", max_rows=None):
    """The 2-D eigenmap (SpectralEmbedding(2) of the latents' kNN graph) coloured by label, with visualize_pca_map's scatter
    -> output_dir/som_spectral_map_epoch_{epoch}.png (rank 0 only; skipped with a warning when matplotlib is missing).
    Returns (embedding [N, 2] float32, labels [N]) as host arrays."""
    from . import evaluation as E
    from .plots import _save_scatter
    who = "visualize_spectral_map"
    if E._world(model) > 1:
        raise ValueError(f"{who}: model.world_size > 1 is not supported; run it on one rank")
    som = model.som_layer
    if metric is None:
        metric = som.distance_fcn if som.distance_fcn in ("cosine", "euclidean") else "euclidean"
    arch = E._Arch(model, config, who).require("som_input")
    X, y = E._whole_set(arch, dataloader, lambda x: arch.som_input(x)[0], labels=True)
    if max_rows is not None:
        X, y = X[:int(max_rows)].contiguous(), y[:int(max_rows)].contiguous()
    with warnings.catch_warnings():
        warnings.filterwarnings("ignore", message=DISCONNECTED)
        se = SpectralEmbedding(2, n_neighbors=int(n_neighbors), metric=metric, random_state=0).fit(X)
    emb, labels = se.embedding_.cpu().numpy(), y.cpu().numpy()
    ev = se.eigenvalues_.cpu().numpy()
    if E._rank(model) == 0:
        axes = (f"eigenvector 2 (Laplacian eigenvalue {1 - ev[1]:.3g})", f"eigenvector 3 (Laplacian eigenvalue {1 - ev[2]:.3g})")
        _save_scatter(who, output_dir, f"som_spectral_map_epoch_{epoch}.png", emb, labels, axis_labels=axes, bbox_inches="tight", dpi=400)
    return emb, labels
