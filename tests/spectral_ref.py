"""An fp64 numpy / scipy restatement of vit_som_amd/spectral.py and csrc/spectral.hip on the host: the graph construction,
the operator, dense eigh of M for N <= 3000, the filter recurrence, the dense algebra of the solver's loop, sklearn's sign
rule, and the fixtures the CPU and GPU tests share."""
import functools

import numpy as np
import scipy.sparse
import scipy.sparse.csgraph

EPS = 2.0 ** -52
CHUNK = 512


# ------------------------------------------------------------------ fixtures
def moons(n=600, noise=0.05, seed=0):
    from sklearn.datasets import make_moons
    X, y = make_moons(n_samples=n, noise=noise, random_state=seed)
    return X.astype(np.float32), y


def circles(n=600, noise=0.03, factor=0.4, seed=0):
    from sklearn.datasets import make_circles
    X, y = make_circles(n_samples=n, noise=noise, factor=factor, random_state=seed)
    return X.astype(np.float32), y


def blobs(n=1000, d=16, centers=5, std=1.0, seed=0, box=(-10.0, 10.0)):
    from sklearn.datasets import make_blobs
    X, y = make_blobs(n_samples=n, n_features=d, centers=centers, cluster_std=std, random_state=seed, center_box=box)
    return X.astype(np.float32), y


def cube(n=3000, d=3, seed=0):
    return np.random.RandomState(seed).uniform(size=(n, d)).astype(np.float32), None


# name -> (rows, n_neighbors); the four fixtures of the solver's tests
FIXTURES = {"moons": (lambda: moons()[0], 10), "circles": (lambda: circles()[0], 10),
            "blobs5": (lambda: blobs(1000, 16, 5, 1.0, 0)[0], 10), "cube": (lambda: cube()[0], 15),
            "blobs700": (lambda: blobs(700, 8, 3, 3.0, 1)[0], 15)}
FOUR = ("moons", "circles", "blobs5", "cube")                     # the solver's fixtures; blobs700 and cube are connected


def knn_affinity(X, k):
    """sklearn's nearest_neighbors affinity: 0.5 (C + C^T), C the kNN connectivity with the row itself, distances in fp64
    on the f32 rows, ties to the smaller index."""
    X = np.asarray(X, np.float64)
    N = X.shape[0]
    sq = (X * X).sum(1)
    D = sq[:, None] + sq[None, :] - 2.0 * X @ X.T
    D[np.arange(N), np.arange(N)] = -1.0
    idx = np.argsort(D, axis=1, kind="stable")[:, :k]
    C = scipy.sparse.csr_matrix((np.ones(N * k), idx.ravel(), np.arange(0, N * k + 1, k)), shape=(N, N))
    A = (0.5 * (C + C.T)).tocsr()
    A.sort_indices()
    return A


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(A scipy CSR, n_neighbors) of a named fixture, computed once."""
    make, k = FIXTURES[name]
    return knn_affinity(make(), k), k


# ------------------------------------------------------------------ the operator
def degrees(A):
    """(d, s): row sums without the diagonal in CSR order, s = d^-1/2 with 0 for an isolated row."""
    A = scipy.sparse.csr_matrix(A, dtype=np.float64)
    N = A.shape[0]
    d = np.zeros(N)
    for i in range(N):
        acc = 0.0
        for p in range(A.indptr[i], A.indptr[i + 1]):
            if A.indices[p] != i:
                acc += A.data[p]
        d[i] = acc
    with np.errstate(divide="ignore"):
        s = np.where(d > 0, 1.0 / np.sqrt(d), 0.0)
    return d, s


def operator(A):
    """M = diag(s) (A - diag A) diag(s) as scipy CSR, and (d, s)."""
    A = scipy.sparse.csr_matrix(A, dtype=np.float64)
    A = (A - scipy.sparse.diags(A.diagonal())).tocsr()
    A.eliminate_zeros()
    d = np.asarray(A.sum(axis=1)).ravel()
    with np.errstate(divide="ignore"):
        s = np.where(d > 0, 1.0 / np.sqrt(d), 0.0)
    S = scipy.sparse.diags(s)
    return (S @ A @ S).tocsr(), d, s


@functools.lru_cache(maxsize=None)
def dense_spectrum(name):
    """(eigenvalues descending, eigenvectors as columns) of M of a named fixture by dense eigh (N <= 3000)."""
    M, _, _ = operator(fixture(name)[0])
    assert M.shape[0] <= 3000
    lam, vec = np.linalg.eigh(M.toarray())
    return lam[::-1].copy(), vec[:, ::-1].copy()


def spmm(A, s, Y1, Y0, alpha, c, beta):
    """vsom_spectral_spmm in the kernel's order -> (out, bound): every row's sum cut into chunks of 512 entries in CSR order,
    a chunk one chain, the chunks added in order.  bound[i, t] = nnz_row 2^-52 sum |terms| + a few ulps of the epilogue's
    own operations: the error any order of the same terms can have."""
    A = scipy.sparse.csr_matrix(A, dtype=np.float64)
    N, l = Y1.shape
    out, bound = np.zeros((N, l)), np.zeros((N, l))
    for i in range(N):
        p0, p1 = A.indptr[i], A.indptr[i + 1]
        total, mag, first = np.zeros(l), np.zeros(l), True
        for q in range(p0, p1, CHUNK):
            part = np.zeros(l)
            for p in range(q, min(q + CHUNK, p1)):
                j = A.indices[p]
                if j == i:
                    continue
                w = A.data[p] * s[j]
                part = part + w * Y1[j]
                mag += np.abs(w * Y1[j])
            total, first = (part if first else total + part), False
        m = s[i] * total
        r = alpha * (m - c * Y1[i])
        big = np.abs(alpha) * (s[i] * mag + np.abs(c * Y1[i]))
        if Y0 is not None:
            r = r - beta * Y0[i]
            big = big + np.abs(beta * Y0[i])
        out[i] = r
        bound[i] = (p1 - p0) * EPS * np.abs(alpha) * s[i] * mag + 8 * EPS * big
    return out, bound


def filter_block(M, Y, a, degree):
    """The scaled Chebyshev filter of spectral.chebyshev_filter, with a scipy operator."""
    c, e = (a - 1.0) / 2.0, (a + 1.0) / 2.0
    sigma1 = e / (1.0 - c)
    sigma = sigma1
    y0, y1 = Y, (sigma1 / e) * (M @ Y - c * Y)
    for _ in range(2, degree + 1):
        new = 1.0 / (2.0 / sigma1 - sigma)
        y0, y1 = y1, 2.0 * (new / e) * (M @ y1 - c * y1) - sigma * new * y0
        sigma = new
    return y1


def filter_scalar(x, a, degree):
    """The filter's polynomial at the numbers x: 1 at 1, within [-1/T_m, 1/T_m] on [-1, a]."""
    c, e = (a - 1.0) / 2.0, (a + 1.0) / 2.0
    t = (np.asarray(x, np.float64) - c) / e
    cheb = lambda z: np.where(np.abs(z) <= 1, np.cos(degree * np.arccos(np.clip(z, -1, 1))),      # noqa: E731
                              np.sign(z) ** degree * np.cosh(degree * np.arccosh(np.maximum(np.abs(z), 1))))
    return cheb(t) / cheb((1.0 - c) / e)


class HostDense:
    """The dense algebra chebyshev_subspace asks for, on numpy blocks."""

    @staticmethod
    def empty_like(Y):
        return np.empty_like(Y)

    @staticmethod
    def grams(V, W):
        return V.T @ V, (V.T @ W if W is not None else None)

    @staticmethod
    def rotate(V, T, out):
        out[:, :T.shape[1]] = V @ T
        return out[:, :T.shape[1]]

    @staticmethod
    def residual(V, W, theta):
        E = W - V * theta[None, :V.shape[1]]
        return (E * E).sum(0)


def host_apply(M):
    def apply(Y1, Y0, alpha, c, beta, out):
        out[...] = alpha * (M @ Y1 - c * Y1) - (beta * Y0 if Y0 is not None else 0.0)
        return out
    return apply


def solve_host(A, n, seed=0, tol=1e-8, degree=20, max_iter=60):
    """spectral.solve with the host operator: the very loop of the package, driven by scipy."""
    from vit_som_amd import spectral as S
    M, d, _ = operator(A)
    Y = S.start_block(d, min(n + S.OVERSAMPLE, A.shape[0]), np.random.RandomState(seed))
    theta, V, res, it = S.chebyshev_subspace(host_apply(M), HostDense, Y, n, tol, degree, max_iter)
    return theta[:n], V[:, :n], res[:n], it


# ------------------------------------------------------------------ sklearn's conventions
def sign_flip(U):
    """sklearn's _deterministic_vector_sign_flip on the COLUMNS of U [N, n]: the entry of largest magnitude positive, the
    first row on a tie -> (flipped, signs)."""
    at = np.argmax(np.abs(U), axis=0)
    sg = np.sign(U[at, np.arange(U.shape[1])])
    sg[sg == 0] = 1.0
    return U * sg, sg


def sklearn_vectors(A, n, seed=0):
    """The n leading unit eigenvectors of M from sklearn's spectral embedding (what SpectralEmbedding(affinity="precomputed",
    eigen_solver="arpack") runs, with the first vector kept): its output is u = D^-1/2 x, so x = sqrt(d) u, normalised."""
    from sklearn.manifold import spectral_embedding
    _, d, _ = operator(A)
    emb = spectral_embedding(A, n_components=n, eigen_solver="arpack", random_state=seed, drop_first=False)
    X = emb * np.sqrt(d)[:, None]
    return X / np.linalg.norm(X, axis=0)


def sklearn_embedding(A, n, seed=0, drop_first=True):
    """sklearn's embedding itself: float64 [N, n], its deterministic sign applied."""
    from sklearn.manifold import spectral_embedding
    return spectral_embedding(A, n_components=n, eigen_solver="arpack", random_state=seed, drop_first=drop_first)
