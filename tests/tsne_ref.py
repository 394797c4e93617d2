"""An fp64 numpy restatement of t-SNE as vit_som_amd/tsne.py states it (sklearn 1.7's TSNE): the perplexity bisection, the
joint P, gradient and KL, the update rule, and whole trajectories with a float64 or a float32 state.  No device, nothing
from the package: test_tsne_cpu.py holds it against sklearn's own functions, test_tsne_gpu.py holds the kernels against it."""
import numpy as np
import scipy.sparse

EPS = np.finfo(np.double).eps
EPSILON_DBL = np.float64(np.float32(1e-8))           # sklearn/manifold/_utils.pyx keeps both constants as C floats
TOLERANCE = np.float64(np.float32(1e-5))
N_STEPS = 100
EXPLORATION_ITERS, N_ITER_CHECK = 250, 50


# ------------------------------------------------------------------ affinities
def row_sums(a):
    """Row sums in ascending column order (the scalar loop's order, not numpy's pairwise one)."""
    s = np.zeros(a.shape[0])
    for j in range(a.shape[1]):
        s += a[:, j]
    return s


def entropy_gap(d, beta, perplexity):
    """-> (e, S, H - log perplexity) of every row at its beta; d float32 [N, k]."""
    d = np.asarray(d, dtype=np.float32)
    with np.errstate(under="ignore"):
        e = np.exp((-d).astype(np.float64) * beta[:, None])
    S = row_sums(e)
    S = np.where(S == 0.0, EPSILON_DBL, S)
    sdp = row_sums(d.astype(np.float64) * (e / S[:, None]))
    return e, S, (np.log(S) + beta * sdp) - np.log(np.float64(np.float32(perplexity)))


def bisection_trace(d, perplexity, steps=N_STEPS):
    """The bisection run for all `steps` steps without stopping -> (betas [steps, N], gaps [steps, N], stop [N]): the beta
    evaluated at each step, its entropy gap, and the step at which sklearn's loop stops (the first gap within the tolerance,
    else the last step).  Up to its stop a row's iterates are those of the stopping loop."""
    d = np.asarray(d, dtype=np.float32)
    N = d.shape[0]
    beta, lo, hi = np.ones(N), np.full(N, -np.inf), np.full(N, np.inf)
    betas, gaps = np.empty((steps, N)), np.empty((steps, N))
    for l in range(steps):
        gap = entropy_gap(d, beta, perplexity)[2]
        betas[l], gaps[l] = beta, gap
        up = gap > 0.0
        lo = np.where(up, beta, lo)
        hi = np.where(up, hi, beta)
        with np.errstate(invalid="ignore", over="ignore"):
            beta = np.where(up, np.where(np.isinf(hi), beta * 2.0, (beta + hi) / 2.0),
                            np.where(np.isinf(lo), beta / 2.0, (beta + lo) / 2.0))
    hit = np.abs(gaps) <= TOLERANCE
    stop = np.where(hit.any(axis=0), hit.argmax(axis=0), steps - 1)
    return betas, gaps, stop


def conditional_p_at(d, beta, perplexity=2.0):
    e, S, _ = entropy_gap(d, beta, perplexity)
    return e / S[:, None]


def conditional_p(d, perplexity):
    """_binary_search_perplexity -> (P float64 [N, k], beta [N], stop [N])."""
    betas, _, stop = bisection_trace(d, perplexity)
    beta = betas[stop, np.arange(betas.shape[1])]
    return conditional_p_at(d, beta), beta, stop


def squared_f32(dist):
    """Euclidean distances squared as sklearn squares them: in float32."""
    dist = np.asarray(dist, dtype=np.float32)
    return dist * dist


def joint_p(knn_idx, cond):
    """(C + C^T) / sum as a dense float64 [N, N]."""
    N, k = knn_idx.shape
    C = np.zeros((N, N))
    C[np.arange(N)[:, None], knn_idx] = cond
    P = C + C.T
    return P / max(P.sum(), EPS)


# ------------------------------------------------------------------ gradient, KL, update
def pair_terms(Y):
    """-> (q [N, N] with a zero diagonal, dx, dy) in float64 from Y [N, 2] (any float type; differences taken in fp64)."""
    Y = np.asarray(Y).astype(np.float64)
    dx = Y[:, 0][:, None] - Y[:, 0][None, :]
    dy = Y[:, 1][:, None] - Y[:, 1][None, :]
    q = 1.0 / (1.0 + (dx * dx + dy * dy))
    np.fill_diagonal(q, 0.0)
    return q, dx, dy


def repulsion(Y):
    """-> (rep [N, 2], sumq [N], Z): sum_j q^2 (y_i - y_j), sum_j q over j != i, and their total."""
    q, dx, dy = pair_terms(Y)
    q2 = q * q
    return np.stack([(q2 * dx).sum(axis=1), (q2 * dy).sum(axis=1)], axis=1), q.sum(axis=1), q.sum()


def kl_and_grad(P, Y, exaggeration=1.0):
    """P: dense or scipy-sparse symmetric joint P -> (KL with P * exaggeration as sklearn reports it, grad [N, 2])."""
    P = np.asarray(P.todense()) if scipy.sparse.issparse(P) else np.asarray(P)
    P = P * float(exaggeration)
    q, dx, dy = pair_terms(Y)
    Z = q.sum()
    pq, q2 = P * q, q * q
    grad = 4.0 * np.stack([(pq * dx).sum(axis=1) - (q2 * dx).sum(axis=1) / Z, (pq * dy).sum(axis=1) - (q2 * dy).sum(axis=1) / Z], axis=1)
    nz = P > 0.0
    kl = float((P[nz] * np.log(np.maximum(P[nz], EPS) / np.maximum(q[nz] / Z, EPS))).sum())
    return kl, grad


def update_step(Y, update, gains, grad, momentum, lr):
    """One application of the update rule; the state's dtype (float32 or float64) is Y's.  float32: gains in f32, the update
    computed in fp64 and rounded once, Y + update in f32 -- vsom_tsne_step's arithmetic."""
    dt = Y.dtype.type
    inc = update.astype(np.float64) * grad < 0.0
    gains = np.maximum(np.where(inc, gains + dt(0.2), gains * dt(0.8)).astype(dt), dt(0.01))
    update = (momentum * update.astype(np.float64) - (lr * gains.astype(np.float64)) * grad).astype(dt)
    return (Y + update).astype(dt), update, gains


def run(P, Y, n_iter, lr, exaggeration, momentum, update=None, gains=None):
    """n_iter iterations of one stage -> (Y, update, gains, KL and |grad| at the last iteration's start)."""
    Pd = np.asarray(P.todense()) if scipy.sparse.issparse(P) else np.asarray(P)
    update = np.zeros_like(Y) if update is None else update
    gains = np.ones_like(Y) if gains is None else gains
    kl = gn = float("nan")
    for _ in range(n_iter):
        kl, grad = kl_and_grad(Pd, Y, exaggeration)
        gn = float(np.sqrt((grad * grad).sum()))
        Y, update, gains = update_step(Y, update, gains, grad, momentum, lr)
    return Y, update, gains, kl, gn


def fit(P, Y0, max_iter=1000, early_exaggeration=12.0, lr=None, n_iter_without_progress=300, min_grad_norm=1e-7):
    """sklearn's two stages with its stopping rules -> (Y, last KL computed, last iteration)."""
    Pd = np.asarray(P.todense()) if scipy.sparse.issparse(P) else np.asarray(P)
    N = Pd.shape[0]
    lr = max(N / early_exaggeration / 4.0, 50.0) if lr is None else lr
    Y, it, kl = Y0.copy(), 0, float("nan")
    for end, exag, mom, window in ((min(EXPLORATION_ITERS, max_iter), early_exaggeration, 0.5, EXPLORATION_ITERS),
                                   (max_iter, 1.0, 0.8, n_iter_without_progress)):
        update, gains = np.zeros_like(Y), np.ones_like(Y)
        best, best_it, i = np.finfo(float).max, it, it - 1
        for i in range(it, end):
            check = (i + 1) % N_ITER_CHECK == 0
            kl_i, grad = kl_and_grad(Pd, Y, exag)
            Y, update, gains = update_step(Y, update, gains, grad, mom, lr)
            if check or i == end - 1:
                kl = kl_i
            if check:
                if kl < best:
                    best, best_it = kl, i
                elif i - best_it > window:
                    break
                if np.sqrt((grad * grad).sum()) <= min_grad_norm:
                    break
        it = i + 1
    return Y, kl, it - 1


# ------------------------------------------------------------------ data and host-side neighbours
def exact_knn(X, k, metric):
    """The k nearest OTHER rows of every row in fp64 -> (idx int64 [N, k], dist float32 [N, k]) ascending by (distance, index)."""
    X = np.asarray(X, dtype=np.float64)
    if metric == "cosine":
        Xn = X / np.maximum(np.linalg.norm(X, axis=1, keepdims=True), 1e-300)
        D = np.maximum(1.0 - Xn @ Xn.T, 0.0)
    else:
        sq = (X * X).sum(axis=1)
        D = np.sqrt(np.maximum(sq[:, None] + sq[None, :] - 2.0 * (X @ X.T), 0.0))
    np.fill_diagonal(D, np.inf)
    idx = np.argsort(D, axis=1, kind="stable")[:, :k]
    return idx.astype(np.int64), np.take_along_axis(D, idx, axis=1).astype(np.float32)


def blobs(N, D, centres, seed, scale=4.0):
    """N rows around `centres` blob centres scale * N(0, 1) with unit noise -> (X float32 [N, D], labels)."""
    rs = np.random.RandomState(seed)
    C = scale * rs.standard_normal((centres, D))
    lab = rs.randint(0, centres, size=N)
    return (C[lab] + rs.standard_normal((N, D))).astype(np.float32), lab


def pca_init(X):
    """sklearn's default init from an exact SVD: the first two principal coordinates / std(first) * 1e-4, float32."""
    X = np.asarray(X, dtype=np.float64)
    Xc = X - X.mean(axis=0)
    U, S, _ = np.linalg.svd(Xc, full_matrices=False)
    E = (U[:, :2] * S[:2]).astype(np.float32)
    return (E / np.std(E[:, 0]) * np.float32(1e-4)).astype(np.float32)
