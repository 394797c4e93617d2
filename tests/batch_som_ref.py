"""Reference for the batch-SOM tests: the seeded fixture, the grid, and an fp64 restatement of one epoch of Kohonen's batch
map as SOMLayer.fit_batch runs it -- BMU search, per-unit sums, the shifted neighbourhood update, the cosine normalisation.
The same formulas evaluated in numpy float32 give the e32 of the project's tolerance rule (pca_ref.bound)."""
import functools

import numpy as np

# (N, D, (rows, cols)): the smallest shapes that reach every code path of the two kernels
SHAPES = [(257, 12288, (4, 4)), (333, 1003, (5, 7)), (130, 3, (3, 3)), (5, 40, (2, 3)), (5, 40, (1, 1)), (2100, 192, (40, 40))]
TRAIN_SHAPES = [(600, 40, (6, 5)), (2100, 192, (40, 40))]


@functools.lru_cache(maxsize=None)
def fixture(N, D, K):
    """(X [N, D], W0 [K, D]) float32, read-only: X = C[lab] + 0.6 randn + 0.5 with 7 centres C ~ N(0, 1), RandomState(3);
    W0 = X[choice(N, K, replace=N < K)] + 0.01 randn, RandomState(4)."""
    rng = np.random.RandomState(3)
    C = rng.standard_normal((7, D))
    lab = rng.randint(0, 7, size=N)
    X = (C[lab] + 0.6 * rng.standard_normal((N, D)) + 0.5).astype(np.float32)
    rng = np.random.RandomState(4)
    W0 = (X[rng.choice(N, K, replace=N < K)] + 0.01 * rng.standard_normal((K, D))).astype(np.float32)
    X.setflags(write=False)
    W0.setflags(write=False)
    return X, W0


def random_bmu(N, K, seed, empty_share=0.3):
    """Random assignments of N rows to K units of which about `empty_share` (at least one when K > 1) get no row."""
    rng = np.random.RandomState(seed)
    alive = np.flatnonzero(rng.uniform(size=K) >= empty_share)
    if K > 1 and len(alive) == K:
        alive = alive[1:]
    if len(alive) == 0:
        alive = np.array([K // 2])
    return alive[rng.randint(0, len(alive), size=N)].astype(np.int64)


def grid_positions(rows, cols, topology):
    """SOMLayer.create_grid_positions, float32 [K, 2]."""
    K = rows * cols
    pos = np.zeros((K, 2), dtype=np.float32)
    for i in range(K):
        r, c = divmod(i, cols)
        if topology == "square":
            pos[i] = (r, c)
        else:
            pos[i] = (c + (0.5 if r % 2 == 1 else 0.0), np.float32(r * np.sqrt(3) / 2))
    return pos


def schedule(hi, lo, T):
    """hi (lo / hi)^(t / (T - 1)); hi alone when T = 1."""
    if T == 1:
        return np.array([float(hi)])
    return float(hi) * (float(lo) / float(hi)) ** (np.arange(T, dtype=np.float64) / (T - 1))


# ------------------------------------------------------------------------------------ the four steps
def inv_norm32(X):
    """ops.row_inv_norm: 1 / max(|row|, 1e-12), float32 (the norm from an fp64 sum of squares, rounded once)."""
    n = np.sqrt((np.asarray(X, np.float64) ** 2).sum(axis=1))
    return (1.0 / np.maximum(n, 1e-12)).astype(np.float32)


def bmu_search(X, W, distance):
    """-> (bmu [N] int64, dist [N, K] float64) in fp64; first index on a tie."""
    X, W = np.asarray(X, np.float64), np.asarray(W, np.float64)
    if distance == "cosine":
        Xn = X / np.maximum(np.linalg.norm(X, axis=1, keepdims=True), 1e-12)
        Wn = W / np.maximum(np.linalg.norm(W, axis=1, keepdims=True), 1e-12)
        dist = 1.0 - Xn @ Wn.T
    else:
        dist = np.sqrt(np.maximum((X * X).sum(1)[:, None] - 2.0 * X @ W.T + (W * W).sum(1)[None, :], 0.0))
    return dist.argmin(axis=1).astype(np.int64), dist


def accumulate(X, bmu, K, inv_norm=None, sums=None, counts=None):
    """np.add.at in fp64 over the rows in ascending index: the bits vsom_som_batch_accumulate must give."""
    X = np.asarray(X)
    Y = X.astype(np.float64)
    if inv_norm is not None:
        Y = Y * np.asarray(inv_norm).astype(np.float64)[:, None]       # exact: two f32 factors
    sums = np.zeros((K, X.shape[1]), dtype=np.float64) if sums is None else sums
    counts = np.zeros(K, dtype=np.int64) if counts is None else counts
    np.add.at(sums, bmu, Y)
    counts += np.bincount(bmu, minlength=K)
    return sums, counts


def grid_d2(pos, dtype=np.float64):
    p = np.asarray(pos).astype(dtype)
    d = p[:, None, :] - p[None, :, :]
    return (d * d).sum(axis=2)


def update(sums, counts, pos, sigma, normalize=False, dtype=np.float64, shifted=True):
    """W_k = sum_c h(k,c) S_c / sum_c h(k,c) n_c over the hit units, h = exp(-(d2 - m_k) / (2 sigma^2)), m_k the smallest d2
    of row k among the hit units (0 when shifted=False).  dtype=np.float32: every value and operation in float32."""
    hit = np.asarray(counts) > 0
    d2 = grid_d2(pos, dtype)
    m = np.where(hit[None, :], d2, np.inf).min(axis=1).astype(dtype) if shifted else np.zeros(len(hit), dtype=dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        arg = -(d2 - m[:, None]) / dtype(2.0 * dtype(sigma) * dtype(sigma))
    with np.errstate(under="ignore"):
        h = np.exp(np.where(hit[None, :], arg, -np.inf).astype(dtype)).astype(dtype)         # exactly 0 for a unit without hits
    S = np.where(hit[:, None], np.asarray(sums).astype(dtype), dtype(0))
    num = h @ S
    den = h @ np.asarray(counts).astype(dtype)
    W = (num / den[:, None]).astype(dtype)
    if normalize:
        W = (W / np.maximum(np.sqrt((W * W).sum(axis=1, keepdims=True)), dtype(1e-12))).astype(dtype)
    return W


def update_limit_small(sums, counts, pos, dtype=np.float64):
    """sigma -> 0 on a grid whose d2 are exact (square): a hit unit is the mean of its rows, a unit without hits the pooled
    mean of its equidistant nearest hit units."""
    hit = np.asarray(counts) > 0
    d2 = np.where(hit[None, :], grid_d2(pos, np.float64), np.inf)
    near = d2 == d2.min(axis=1, keepdims=True)
    S, n = np.asarray(sums).astype(dtype), np.asarray(counts).astype(dtype)
    return ((near.astype(dtype) @ S) / (near.astype(dtype) @ n)[:, None]).astype(dtype)


def epoch(X, W, pos, sigma, distance, bmu=None):
    """One epoch in fp64 -> (W_new64, W_new32, bmu): teacher-forced when `bmu` is given.  W_new32 is the update (and the
    normalisation) evaluated in float32 from the same fp64 sums: the e32 of the rule."""
    if bmu is None:
        bmu, _ = bmu_search(X, W, distance)
    cosine = distance == "cosine"
    sums, counts = accumulate(X, bmu, len(W), inv_norm32(X) if cosine else None)
    return (update(sums, counts, pos, sigma, normalize=cosine), update(sums, counts, pos, sigma, normalize=cosine, dtype=np.float32),
            bmu)


def quantization_error(X, W, bmu, distance):
    """Mean distance of every row to the unit `bmu` names, fp64."""
    _, dist = bmu_search(X, W, distance)
    return float(dist[np.arange(len(bmu)), bmu].mean())
