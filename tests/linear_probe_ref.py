"""References for the linear-probe tests: the seeded fixtures, the fp64 objective and gradient of
vit_som_amd/linear_probe.py in numpy, its fp64 optimum by scipy (L-BFGS-B, gtol 1e-10), sklearn's pipeline, the kernels'
arithmetic in fp64 numpy, the textbook two-loop recursion, and a host emulation of the device's solver (f32 contractions,
fp64 everywhere else; numpy's summation order, so it pins the algorithm and its error level, not the bits)."""
import functools

import numpy as np

# name -> (N, D, C, seed, shift, row padding on the device).  The last one has D % 4 != 0 and is given a padded row stride
# that is no multiple of four either in the GPU tests: the contractions then load element-wise.
FIXTURES = {
    "odd": (257, 131, 5, 1, 0.0, 0),
    "shifted": (300, 64, 3, 2, 50.0, 0),
    "wide": (515, 260, 17, 3, 0.0, 0),
    "elementwise": (130, 37, 4, 4, 0.0, 2),
}
HELD_OUT = 200


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(X f32 [N, D], y int64 [N], X_held f32 [200, D], y_held): rows are class mean plus unit noise, the means drawn from
    N(0, 0.25), every value shifted by `shift`.  Every class occurs.  Cached and read-only."""
    N, D, C, seed, shift, _ = FIXTURES[name]
    rng = np.random.RandomState(seed)
    means = rng.normal(0.0, 0.5, (C, D))
    y = rng.randint(0, C, N + HELD_OUT)
    y[:C] = np.arange(C)
    X = (means[y] + rng.standard_normal((N + HELD_OUT, D)) + shift).astype(np.float32)
    y = y.astype(np.int64)
    for a in (X, y):
        a.setflags(write=False)
    return X[:N], y[:N], X[N:], y[N:]


def standardise(X):
    """(mean, scale) in fp64 as StandardScaler has them: the population std, 1 for a constant column."""
    X = np.asarray(X, np.float64)
    mean, std = X.mean(axis=0), X.std(axis=0)
    return mean, np.where(std == 0, 1.0, std)


def softmax_parts(Z):
    """fp64 (P, log-sum-exp) of the rows of Z, the row maximum subtracted."""
    Z = np.asarray(Z, np.float64)
    zmax = Z.max(axis=1, keepdims=True)
    E = np.exp(Z - zmax)
    s = E.sum(axis=1, keepdims=True)
    return E / s, (np.log(s) + zmax)[:, 0]


def objective(theta, Xs, y, C, C_reg, intercept=True):
    """F and its gradient at theta = (W [C, D] row-major, b [C]) on the standardised fp64 rows Xs."""
    N, D = Xs.shape
    W = theta[:C * D].reshape(C, D)
    b = theta[C * D:] if intercept else np.zeros(C)
    P, lse = softmax_parts(Xs @ W.T + b)
    lam = 1.0 / (C_reg * N)
    F = float((lse - (Xs @ W.T + b)[np.arange(N), y]).sum() / N + 0.5 * lam * (W * W).sum())
    R = P
    R[np.arange(N), y] -= 1.0
    g = [(R.T @ Xs / N + lam * W).ravel()]
    if intercept:
        g.append(R.sum(axis=0) / N)
    return F, np.concatenate(g)


def objective_at(W, b, X, y, mean, scale, C_reg):
    """F and max |gradient| in fp64 at parameters fitted with the statistics (mean, scale)."""
    Xs = (np.asarray(X, np.float64) - np.asarray(mean, np.float64)) / np.asarray(scale, np.float64)
    W, b = np.asarray(W, np.float64), np.asarray(b, np.float64)
    F, g = objective(np.concatenate([W.ravel(), b]), Xs, np.asarray(y), W.shape[0], C_reg)
    return F, float(np.abs(g).max())


@functools.lru_cache(maxsize=None)
def optimum(name, C_reg):
    """(W, b, F) of the fp64 optimum: scipy's L-BFGS-B to gtol 1e-10 on the rows standardised in fp64."""
    from scipy.optimize import minimize
    X, y, _, _ = fixture(name)
    C = FIXTURES[name][2]
    mean, scale = standardise(X)
    Xs = (X.astype(np.float64) - mean) / scale
    D = Xs.shape[1]
    res = minimize(objective, np.zeros(C * D + C), args=(Xs, y, C, C_reg), jac=True, method="L-BFGS-B",
                   options=dict(gtol=1e-10, ftol=1e-16, maxiter=20000, maxfun=40000, maxcor=20))
    W, b = res.x[:C * D].reshape(C, D), res.x[C * D:]
    return W, b, float(res.fun)


def margins(W, b, Xs):
    """The fp64 top-two margin of every row's decision values."""
    Z = np.sort(Xs @ W.T + b, axis=1)
    return Z[:, -1] - Z[:, -2]


@functools.lru_cache(maxsize=None)
def sklearn_pipeline(name, C_reg):
    from sklearn.linear_model import LogisticRegression
    from sklearn.pipeline import make_pipeline
    from sklearn.preprocessing import StandardScaler
    X, y, _, _ = fixture(name)
    return make_pipeline(StandardScaler(), LogisticRegression(C=C_reg, tol=1e-10, max_iter=20000)).fit(X.astype(np.float64), y)


# ------------------------------------------------------------------ the kernels in fp64 numpy
def residual(Z32, b, y):
    """(R f32, summed CE, column sums of the rounded R, first argmax, softmax) of vsom_probe_residual on the f32 logits;
    rows whose label is outside [0, C) contribute nothing and have a zero row of R."""
    Z = np.asarray(Z32, np.float64) + (0.0 if b is None else np.asarray(b, np.float64))
    N, C = Z.shape
    y = np.asarray(y)
    ok = (y >= 0) & (y < C)
    P, lse = softmax_parts(Z)
    R = P.copy()
    R[np.nonzero(ok)[0], y[ok]] -= 1.0
    R[~ok] = 0.0
    R32 = R.astype(np.float32)
    loss = float((lse[ok] - Z[np.nonzero(ok)[0], y[ok]]).sum())
    return R32, loss, R32.astype(np.float64).sum(axis=0), Z.argmax(axis=1), P


def ladder(Z32, Zp32, b, pb, y, alpha0, nsteps):
    """phi[j] of vsom_probe_linesearch: the summed CE at Z + a_j Zp, b + a_j pb, a_j = alpha0 2^-j, in fp64."""
    out = []
    for j in range(nsteps):
        a = alpha0 * 2.0 ** -j
        Z = np.asarray(Z32, np.float64) + a * np.asarray(Zp32, np.float64)
        out.append(residual(Z, None if b is None else np.asarray(b) + a * np.asarray(pb), y)[1])
    return np.array(out)


def armijo(phi, alpha0, f0, pen, gtp, N, lam, c1=1e-4):
    """(alpha, status, F(alpha), j) as vsom_probe_step chooses them, in plain fp64."""
    ww, wp, pp = (float(v) for v in pen)
    F0 = f0 * (1.0 / N) + 0.5 * lam * ww
    if not gtp < 0.0:
        return 0.0, 2, F0, -1
    for j in range(len(phi)):
        a = alpha0 * 2.0 ** -j
        F = phi[j] * (1.0 / N) + 0.5 * lam * (ww + 2.0 * a * wp + a * a * pp)
        if F <= F0 + c1 * a * gtp:
            return a, 0, F, j
    return 0.0, 1, F0, -1


def two_loop(pairs, g):
    """The textbook two-loop recursion: -H g for the (s, y) pairs given oldest first, H0 = (s.y / y.y) I of the newest."""
    q = -np.asarray(g, np.float64)
    alphas = []
    for s, yv in reversed(pairs):
        a = (s @ q) / (s @ yv)
        alphas.append(a)
        q = q - a * yv
    if pairs:
        s, yv = pairs[-1]
        q = q * ((s @ yv) / (yv @ yv))
    for (s, yv), a in zip(pairs, reversed(alphas)):
        beta = (yv @ q) / (s @ yv)
        q = q + (a - beta) * s
    return q


# ------------------------------------------------------------------ the device's solver on the host
def emulate(X32, y, C, C_reg, tol, max_iter, m=10, refresh=10, nsteps=16, c1=1e-4):
    """linear_probe.LogisticRegression.fit with numpy standing in for the kernels: the two contractions in float32 on rows
    centred in float32, everything else in fp64.  -> (W, b, mean f32, scale, iterations, converged)."""
    X32 = np.asarray(X32, np.float32)
    N, D = X32.shape
    mean = X32.astype(np.float64).mean(axis=0).astype(np.float32)
    std = np.sqrt(((X32.astype(np.float64) - mean) ** 2).sum(axis=0) / N)
    invstd = np.where(std == 0, 0.0, 1.0 / np.where(std == 0, 1.0, std))
    Xc = X32 - mean
    lam = 1.0 / (C_reg * N)
    W, b = np.zeros((C, D)), np.zeros(C)
    project = lambda A: Xc @ (A * invstd).astype(np.float32).T                  # noqa: E731

    def gradient(Z):
        R32, loss, gb, _, _ = residual(Z, b, y)
        Zt = R32.T @ Xc
        return loss, np.concatenate([(Zt.astype(np.float64) * invstd / N + lam * W).ravel(), gb / N])

    Z = project(W)
    loss, g = gradient(Z)
    pairs, it, failed_last, converged = [], 0, False, bool(np.abs(g).max() <= tol)
    while not converged and it < max_iter:
        it += 1
        p = two_loop(pairs, g)
        P, pb = p[:C * D].reshape(C, D), p[C * D:]
        Zp = project(P)
        alpha0 = 1.0 if pairs else min(1.0, 1.0 / np.sqrt(g @ g))
        phi = ladder(Z, Zp, b, pb, y, alpha0, nsteps)
        alpha, status, _, _ = armijo(phi, alpha0, loss, ((W * W).sum(), (W * P).sum(), (P * P).sum()), float(g @ p), N, lam, c1)
        if status:
            if failed_last:
                break
            failed_last, pairs = True, []
            Z = project(W)
            loss, g = gradient(Z)
            continue
        failed_last = False
        W, b = W + alpha * P, b + alpha * pb
        fresh = it % refresh == 0
        Z = project(W) if fresh else (Z.astype(np.float64) + alpha * Zp.astype(np.float64)).astype(np.float32)
        loss, g_new = gradient(Z)
        s, yv = alpha * p, g_new - g
        if s @ yv > 0:
            pairs = (pairs + [(s, yv)])[-m:]
        g = g_new
        if np.abs(g).max() <= tol:
            if fresh:
                converged = True
            else:
                Z = project(W)
                loss, g_fresh = gradient(Z)
                converged = bool(np.abs(g_fresh).max() <= tol)
    return W, b, mean, np.where(std == 0, 1.0, std), it, converged
