"""References for the PCA tests: the seeded fixture generator, the tolerance rule, sklearn's answers, and a numpy
restatement of the algorithm of vit_som_amd/pca.py, step for step (f32 products where the device uses f32, fp64 where
it uses fp64; the summation ORDER inside a product is numpy's, so the restatement pins the algorithm, not the bits)."""
import functools

import numpy as np

EPS32 = 2.0 ** -23

# (N, D, r, ratio, noise, k): the solver fixtures, then the wide-basis one (l = 65) and the rank-deficient one
SOLVER_FIXTURES = [(257, 12288, 12, 0.7, 1e-3, 8), (333, 1003, 12, 0.7, 1e-3, 2), (130, 3, 3, 0.7, 0.0, 2),
                   (257, 200, 30, 0.8, 1e-4, 24)]
WIDE_FIXTURE = (300, 520, 60, 0.9, 1e-5, 57)
RANK_FIXTURE = (5, 40, 4, 0.7, 0.0, 5)


@functools.lru_cache(maxsize=None)
def fixture(N, D, r, ratio, noise, seed=0):
    """X = U diag(ratio^j sqrt(N)) V^T + noise randn + 5 randn(D), float32: a rank-r signal with geometric singular values,
    isotropic noise, and a column mean that is large against the spread.  Cached and read-only."""
    rng = np.random.RandomState(seed)
    U = np.linalg.qr(rng.standard_normal((N, r)))[0]
    V = np.linalg.qr(rng.standard_normal((D, r)))[0]
    s = ratio ** np.arange(r) * np.sqrt(N)
    X = (U * s) @ V.T + noise * rng.standard_normal((N, D)) + 5.0 * rng.standard_normal(D)
    X = X.astype(np.float32)
    X.setflags(write=False)
    return X


def rel_err(got, ref64):
    """The rule's measure: the largest absolute error over the largest absolute fp64 value."""
    ref64 = np.asarray(ref64, np.float64)
    return float(np.max(np.abs(np.asarray(got, np.float64) - ref64)) / np.max(np.abs(ref64)))


def bound(ref32, ref64):
    """4 x max(e32, 2^-23): e32 is the float32 reference's error against the same fp64 value by the same measure."""
    return 4.0 * max(rel_err(ref32, ref64), EPS32)


def one_minus_cos(A, B):
    """max over the rows of 1 - |cos| between matching rows, in fp64."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    c = np.abs(np.sum(A * B, axis=1)) / (np.linalg.norm(A, axis=1) * np.linalg.norm(B, axis=1))
    return float(np.max(1.0 - c))


def ortho_err(W):
    W = np.asarray(W, np.float64)
    return float(np.max(np.abs(W @ W.T - np.eye(W.shape[0]))))


@functools.lru_cache(maxsize=None)
def sklearn_pair(N, D, r, ratio, noise, k):
    """(sklearn PCA(svd_solver="full") fitted on the float32 fixture, the same on the fixture cast to fp64)."""
    from sklearn.decomposition import PCA as SkPCA
    X = fixture(N, D, r, ratio, noise)
    return SkPCA(n_components=k, svd_solver="full").fit(X), SkPCA(n_components=k, svd_solver="full").fit(X.astype(np.float64))


# ------------------------------------------------------------------------------------ the restatement
def _ritz(H, G):
    theta, S = np.linalg.eigh((H + H.T) / 2)
    theta, S = theta[::-1], S[:, ::-1]
    q = np.array([S[:, i] @ G @ S[:, i] for i in range(len(theta))])
    return theta, S, np.sqrt(np.maximum(q - theta ** 2, 0.0)) / (theta[0] if theta[0] > 0 else 1.0)


def _transform(G, S):
    Gp = S.T @ G @ S
    Gp = (Gp + Gp.T) / 2
    d = np.sqrt(np.maximum(np.diag(Gp), 0.0))
    d[d == 0] = 1.0
    w, V = np.linalg.eigh(Gp / np.outer(d, d))
    keep = w > 2.0 ** -40 * w.max()
    if keep.all():                                          # symmetric: the rows stay with their Ritz vectors
        return V @ np.diag(w ** -0.5) @ V.T @ np.diag(1.0 / d) @ S.T
    return np.diag(w[keep] ** -0.5) @ V[:, keep].T @ np.diag(1.0 / d) @ S.T


def _orthonormalise(Zt, G, S=None):
    """With S: R = S^T Zt (fp64, rounded to f32) and its own Gram matrix first.  Then T R in fp64 rounded once to f32, and
    once more on the result itself."""
    Z64 = Zt.astype(np.float64)
    if S is not None:
        Z64 = (S.T @ Z64).astype(np.float32).astype(np.float64)
        G = Z64 @ Z64.T
    eye = np.eye(Z64.shape[0])
    B64 = (_transform(G, eye) @ Z64).astype(np.float32).astype(np.float64)
    return (_transform(B64 @ B64.T, np.eye(B64.shape[0])) @ B64).astype(np.float32)


def pca_restated(X, k, n_iter=10, n_oversamples=8, seed=0):
    """-> dict(components, explained_variance, explained_variance_ratio, singular_values, mean, residuals, width)."""
    X = np.asarray(X, np.float32)
    N, D = X.shape
    l = min(k + n_oversamples, N, D)
    mean = (X.astype(np.float64).sum(axis=0) / N).astype(np.float32)                    # step 1
    Xc = X - mean                                                                        # centred BEFORE any product
    var = ((X.astype(np.float64) - mean.astype(np.float64)) ** 2).sum(axis=0) / (N - 1)
    Z0 = np.random.RandomState(seed).standard_normal((l, D)).astype(np.float32)         # step 2
    Z064 = Z0.astype(np.float64)
    B = _orthonormalise(Z0, Z064 @ Z064.T)

    def one_pass(B):                                                                     # steps 3 and 4
        Y = Xc @ B.T                                                                     # f32
        Zt = Y.T @ Xc                                                                    # f32
        Z64, B64 = Zt.astype(np.float64), B.astype(np.float64)
        H, G = B64 @ Z64.T, Z64 @ Z64.T
        return Zt, G, _ritz(H, G)

    for _ in range(n_iter):
        Zt, G, (theta, S, res) = one_pass(B)
        B = _orthonormalise(Zt, G, S)                                                    # step 5
    Zt, G, (theta, S, res) = one_pass(B)                                                 # step 6
    kk = min(k, B.shape[0])
    comps = (S.T[:kk] @ B.astype(np.float64)).astype(np.float32)
    big = np.argmax(np.abs(comps), axis=1)
    sign = np.sign(comps[np.arange(kk), big])
    sign[sign == 0] = 1
    comps = comps * sign[:, None].astype(np.float32)
    lam = np.maximum(theta[:kk], 0.0)
    return dict(components=comps, explained_variance=lam / (N - 1), explained_variance_ratio=lam / (N - 1) / var.sum(),
                singular_values=np.sqrt(lam), mean=mean, residuals=res[:kk], width=B.shape[0], total_variance=var.sum())
