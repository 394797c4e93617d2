"""References for the Gaussian-mixture kernels and estimator (tests/test_gmm_cpu.py, tests/test_gmm_gpu.py); no tests here.

1. fp64 numpy restatements of the E-step (direct form), the M-step and sklearn's BaseMixture.fit_predict loop.
2. A plain-fp32 torch restatement of the same direct form -- the f32 sum over D, then an f32 log-softmax -- and of the
   M-step: the error YARDSTICK only.
3. An f32 host emulation of the device solver (f32 terms, f32 sums over segments of 128 columns, fp64 across segments, an
   fp64 log-sum-exp, an M-step shifted at the old means): the yardstick of a whole fit.

The rule is the project's (numeric_edges.py): a device value may differ from fp64 by
max(FLOOR, 4 x the error of the plain-fp32 restatement on the same input).  FLOOR is eval_edges.FLOOR["kmeans"] = 1e-5, the
tolerance of the k-means kernels' own GPU test: the mixture is the soft sibling of that Lloyd step and errors are measured the
same way, relative to the largest reference value of the output."""
import functools

import numpy as np
import torch

from eval_edges import FLOOR as _FLOORS
from numeric_edges import E32_MAX, FACTOR, accepts, bound  # noqa: F401  (re-exported)

FLOOR = _FLOORS["kmeans"]
LOG_2PI = float(np.log(2.0 * np.pi))
EPS10 = 10 * np.finfo(np.float64).eps
GAP = 1e-4                                       # labels are compared where the fp64 top-two gap exceeds this
MAX_UNCLEAR = 0.01                               # and at most this share of the rows may be left out

# (N, D, K) of the kernel tests: one row; fewer rows than a wave's block; odd D; a K chunk tail (7 = 8 - 1); D one past
# the 128-column segment with two K chunks; many chunks and more than one workgroup; the latent width (six LDS tiles);
# the widest K; element loads with two LDS tiles and two K chunks.
SHAPES = [(1, 1, 1), (63, 5, 2), (257, 37, 3), (1001, 128, 7), (1000, 129, 16), (2000, 784, 100), (300, 12288, 10),
          (130, 10, 1024), (40, 2101, 9)]
# (seed, n, d, k, cluster_std, offset, covariance_type) of the whole-fit tests
FIXTURES = [(0, 3000, 20, 5, 4.0, 0.0, "diag"), (2, 1500, 37, 3, 3.0, 0.0, "spherical"), (3, 600, 3072, 4, 8.0, 50.0, "diag")]
TOL = 1e-3


def err(a, ref):
    """max |a - ref| relative to the largest |ref| (1 when the reference is all zero)."""
    a = np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    if ref.size == 0:
        return 0.0
    scale = float(np.abs(ref).max()) or 1.0
    return float(np.abs(a - ref).max()) / scale


def logsumexp(a):
    m = a.max(axis=1, keepdims=True)
    return (m + np.log(np.exp(a - m).sum(axis=1, keepdims=True)))[:, 0]


# ------------------------------------------------------------------------------------------------ fp64 restatements
def full_prec(prec, D):
    """[K, D] precisions of a diag [K, D] or spherical [K] parameter."""
    prec = np.asarray(prec, dtype=np.float64)
    return prec if prec.ndim == 2 else np.repeat(prec[:, None], D, axis=1)


def logc64(weights, prec, D):
    return np.log(np.asarray(weights, np.float64)) + 0.5 * np.log(full_prec(prec, D)).sum(axis=1) - 0.5 * D * LOG_2PI


def log_gaussian64(X, means, prec):
    """sklearn's _estimate_log_gaussian_prob in the direct form, fp64."""
    X, means = np.asarray(X, np.float64), np.asarray(means, np.float64)
    P = full_prec(prec, X.shape[1])
    out = np.empty((X.shape[0], means.shape[0]))
    for k in range(means.shape[0]):
        d = X - means[k]
        out[:, k] = -0.5 * (d * d * P[k]).sum(axis=1)
    return out + 0.5 * np.log(P).sum(axis=1) - 0.5 * X.shape[1] * LOG_2PI


def estep64(X, means, prec, weights):
    """-> dict(logp, lpn, resp, labels, gap): gap is the difference of the two largest log p of a row (inf for K = 1)."""
    logp = log_gaussian64(X, means, prec) + np.log(np.asarray(weights, np.float64))
    lpn = logsumexp(logp)
    top = np.sort(logp, axis=1)
    gap = top[:, -1] - top[:, -2] if logp.shape[1] > 1 else np.full(len(logp), np.inf)
    return dict(logp=logp, lpn=lpn, resp=np.exp(logp - lpn[:, None]), labels=logp.argmax(axis=1), gap=gap)


def mstep64(X, resp, reg_covar, covariance_type):
    """_estimate_gaussian_parameters about the weighted means (two passes, fp64) -> (nk, means, covariances)."""
    X, resp = np.asarray(X, np.float64), np.asarray(resp, np.float64)
    nk = resp.sum(axis=0) + EPS10
    means = resp.T @ X / nk[:, None]
    cov = np.empty_like(means)
    for k in range(means.shape[0]):
        d = X - means[k]
        cov[k] = (resp[:, k, None] * d * d).sum(axis=0) / nk[k]
    cov += reg_covar
    return nk, means, (cov.mean(axis=1) if covariance_type == "spherical" else cov)


def fit64(X, resp0, covariance_type, means_init=None, tol=TOL, reg_covar=1e-6, max_iter=100):
    """BaseMixture.fit_predict for one initialisation from responsibilities, fp64 -> dict."""
    X = np.asarray(X, np.float64)
    n = X.shape[0]
    nk, means, cov = mstep64(X, resp0, reg_covar, covariance_type)
    weights = nk / n
    if means_init is not None:
        means = np.asarray(means_init, np.float64)
    lower_bound, bounds, converged = -np.inf, [], False
    for n_iter in range(1, max_iter + 1):
        prev = lower_bound
        e = estep64(X, means, 1.0 / cov, weights)
        nk, means, cov = mstep64(X, e["resp"], reg_covar, covariance_type)
        weights = nk / nk.sum()
        lower_bound = e["lpn"].mean()
        bounds.append(lower_bound)
        if abs(lower_bound - prev) < tol:
            converged = True
            break
    return dict(weights=weights, means=means, cov=cov, n_iter=n_iter, converged=converged, lower_bounds=bounds)


# ------------------------------------------------------------------------------------------------ plain fp32 (yardstick)
def _t32(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32)


def estep32(X, means, prec, logc):
    """The direct form in plain torch fp32: one f32 sum over D, an f32 log-softmax -> (lpn, resp) as fp64 numpy."""
    X, means = _t32(X), _t32(means)
    P = _t32(full_prec(prec, X.shape[1]))
    logp = torch.empty(X.shape[0], means.shape[0], dtype=torch.float32)
    for k in range(means.shape[0]):
        d = X - means[k]
        logp[:, k] = -0.5 * (d * d * P[k]).sum(dim=1)
    logp = logp + _t32(logc)
    lpn = torch.logsumexp(logp, dim=1)
    return lpn.double().numpy(), torch.exp(logp - lpn[:, None]).double().numpy()


def mstep32(X, resp, reg_covar, covariance_type):
    """mstep64 in plain torch fp32 -> (nk, means, covariances) as fp64 numpy."""
    X, resp = _t32(X), _t32(resp)
    nk = resp.sum(dim=0) + torch.tensor(EPS10, dtype=torch.float32)
    means = resp.T @ X / nk[:, None]
    cov = torch.empty_like(means)
    for k in range(means.shape[0]):
        d = X - means[k]
        cov[k] = (resp[:, k, None] * d * d).sum(dim=0) / nk[k]
    cov = cov + torch.tensor(reg_covar, dtype=torch.float32)
    cov = cov.mean(dim=1) if covariance_type == "spherical" else cov
    return nk.double().numpy(), means.double().numpy(), cov.double().numpy()


# ------------------------------------------------------------------------------------------------ the device solver, emulated
def _estep_emulated(X32, means32, prec32, logc):
    N, D = X32.shape
    pad = (-D) % 128
    lpn_terms = np.empty((N, means32.shape[0]))
    for k in range(means32.shape[0]):
        d = X32 - means32[k]
        t = (d * d) * prec32[k]                                       # f32 terms
        t = np.pad(t, ((0, 0), (0, pad))).reshape(N, -1, 128)
        lpn_terms[:, k] = t.sum(axis=2, dtype=np.float32).astype(np.float64).sum(axis=1)
    logp = logc - 0.5 * lpn_terms
    lpn = logsumexp(logp)
    return lpn, np.exp(logp - lpn[:, None]).astype(np.float32)


def _mstep_emulated(X32, resp32, mu_old32, reg_covar, covariance_type, n_norm):
    nk = resp32.astype(np.float64).sum(axis=0) + EPS10
    K, D = mu_old32.shape
    means, cov = np.empty((K, D), np.float32), np.empty((K, D))
    for k in range(K):
        d = X32.astype(np.float64) - mu_old32[k].astype(np.float64)   # everything fp64: the difference is exact
        rd = resp32[:, k, None].astype(np.float64) * d
        a = rd.sum(axis=0) / nk[k]
        means[k] = (mu_old32[k].astype(np.float64) + a).astype(np.float32)
        cov[k] = (rd * d).sum(axis=0) / nk[k] - a * a + reg_covar
    cov = cov.mean(axis=1) if covariance_type == "spherical" else cov
    weights = nk / (n_norm if n_norm else nk.sum())
    prec32 = full_prec(1.0 / cov, D).astype(np.float32)
    logc = np.log(weights) + 0.5 * np.log(full_prec(1.0 / cov, D)).sum(axis=1) - 0.5 * D * LOG_2PI
    return weights, means, cov, prec32, logc


def fit32_emulated(X, resp0, covariance_type, means_init=None, tol=TOL, reg_covar=1e-6, max_iter=100):
    """The device fit on the host, from the same initial responsibilities -> dict like fit64."""
    X32 = np.asarray(X, np.float32)
    n, D = X32.shape
    resp = np.asarray(resp0, np.float32)
    colmean = X32.astype(np.float64).mean(axis=0).astype(np.float32)
    weights, means, cov, prec32, logc = _mstep_emulated(X32, resp, np.repeat(colmean[None], resp.shape[1], axis=0), reg_covar,
                                                        covariance_type, n)
    if means_init is not None:
        means = np.asarray(means_init, np.float32)
    lower_bound, bounds, converged = -np.inf, [], False
    for n_iter in range(1, max_iter + 1):
        prev = lower_bound
        lpn, resp = _estep_emulated(X32, means, prec32, logc)
        weights, means, cov, prec32, logc = _mstep_emulated(X32, resp, means, reg_covar, covariance_type, 0)
        lower_bound = lpn.mean()
        bounds.append(lower_bound)
        if abs(lower_bound - prev) < tol:
            converged = True
            break
    return dict(weights=weights, means=means.astype(np.float64), cov=cov, n_iter=n_iter, converged=converged, lower_bounds=bounds)


# ------------------------------------------------------------------------------------------------ inputs
def mixture_case(N, D, K, covariance_type="diag", seed=0, offset=0.0, spread=1.0):
    """(X f32 [N, D], means f32 [K, D], prec fp64 ([K, D] or [K]), weights fp64 [K]): rows drawn around means that OVERLAP --
    the means lie 2 / sqrt(D) standard deviations apart per column and the precisions vary by 4 / sqrt(D), so the log odds
    between two components are a few units at every D and the responsibilities are soft -- while the top-two gap of nearly
    every row stays far above GAP."""
    rs = np.random.RandomState(seed + 7 * N + 13 * D + 17 * K)
    means = (offset + rs.randn(K, D) * (2.0 / np.sqrt(D)) * spread).astype(np.float32)
    X = (means[rs.randint(0, K, N)] + rs.randn(N, D) * spread).astype(np.float32)
    vary = min(0.5, 2.0 / np.sqrt(D))
    prec = (1.0 + rs.uniform(-vary, vary, size=(K,) if covariance_type == "spherical" else (K, D))) / spread ** 2
    w = rs.uniform(0.5, 1.5, size=K)
    return X, means, prec, w / w.sum()


@functools.lru_cache(maxsize=None)
def blobs(i):
    """Fixture i -> (X f32, means_init f32, k, covariance_type): make_blobs(...).astype(float32), the rows default_rng picks."""
    from sklearn.datasets import make_blobs
    seed, n, d, k, std, offset, ctype = FIXTURES[i]
    X, _ = make_blobs(n_samples=n, n_features=d, centers=k, cluster_std=std, random_state=seed)
    X = (X + offset).astype(np.float32)
    X.setflags(write=False)
    init = X[np.random.default_rng(seed).choice(n, k, replace=False)].copy()
    init.setflags(write=False)
    return X, init, k, ctype


@functools.lru_cache(maxsize=None)
def sklearn_fit(i):
    """sklearn's GaussianMixture on the float64 copy of fixture i, from means_init (random_state = the fixture's seed)."""
    from sklearn.mixture import GaussianMixture
    X, init, k, ctype = blobs(i)
    return GaussianMixture(k, covariance_type=ctype, tol=TOL, means_init=init.astype(np.float64),
                           random_state=FIXTURES[i][0]).fit(X.astype(np.float64))


@functools.lru_cache(maxsize=None)
def kmeans_resp(i):
    """The one-hot responsibilities sklearn's initialisation of fixture i starts from."""
    from sklearn.cluster import KMeans
    X, _, k, _ = blobs(i)
    label = KMeans(n_clusters=k, n_init=1, random_state=np.random.RandomState(FIXTURES[i][0])).fit(X.astype(np.float64)).labels_
    resp = np.zeros((X.shape[0], k))
    resp[np.arange(X.shape[0]), label] = 1
    return resp
