"""numpy restatement of the on-device DBSCAN in two parts: (1) the bit matrix of csrc/knn.hip's DBSCAN section from a given
distance matrix -- bit j & 63 of word [i, j >> 6] set iff the pair has a distance <= eps, the diagonal set, the tail bits
clear --, (2) the labelling rule of vsom_dbscan_init / _round / _finish: the components of the core rows numbered by
their smallest core row, a border row given the smallest number among its core neighbours.  Plus the lattice fixtures and
the e32 condition the GPU tests put on them."""
import numpy as np

COSINE, EUCLIDEAN = 0, 1                       # VSOM_DIST_*


def words(N):
    return (int(N) + 63) // 64


# ------------------------------------------------------------------ (1) the bit matrix
def adjacency(D, eps):
    """bool [N, N] from a distance matrix (any float dtype; NaN: no distance): (double)d <= eps, the diagonal set -- except
    for a row whose diagonal entry is NaN (a bad row of the contraction: no bit anywhere)."""
    D = np.asarray(D)
    with np.errstate(invalid="ignore"):
        A = D.astype(np.float64) <= float(eps)
    idx = np.arange(D.shape[0])
    A[idx, idx] = ~np.isnan(D[idx, idx])
    return A


def pack(A):
    """bool [N, N] -> uint64 [N, ceil(N / 64)], bit j & 63 of word j >> 6, tail bits clear."""
    N = A.shape[0]
    W = words(N)
    padded = np.zeros((N, W * 64), dtype=bool)
    padded[:, :N] = A
    return np.packbits(padded.reshape(N, W, 64), axis=2, bitorder="little").view(np.uint64).reshape(N, W)


def unpack(words_, N):
    """uint64 (or int64) [N, W] -> bool [N, W * 64]: every bit, the tail included."""
    w = np.ascontiguousarray(words_).view(np.uint64)
    return np.unpackbits(w.view(np.uint8).reshape(N, -1), axis=1, bitorder="little").astype(bool)


def bit_matrix(D, eps):
    return pack(adjacency(D, eps))


def popcounts(words_, N):
    return unpack(words_, N).sum(axis=1).astype(np.int32)


def check_structure(words_, N, bad=()):
    """What holds of every bit matrix of the contract: symmetric, the diagonal set (clear for a bad row), zero tail bits."""
    bits = unpack(words_, N)
    assert not bits[:, N:].any(), "tail bits"
    A = bits[:, :N]
    assert np.array_equal(A, A.T), "symmetry"
    want = np.ones(N, dtype=bool)
    want[list(bad)] = False
    assert np.array_equal(np.diag(A), want), "diagonal"
    return A


# ------------------------------------------------------------------ (2) the labelling rule
def labels_from_adjacency(A, min_samples):
    """-> (labels int64 [N], core bool [N], record [clusters, core, border, noise]) by the rule of vsom_dbscan_finish: core =
    row popcount >= min_samples; a cluster is a connected component of the core rows, numbered by the rank of its smallest
    core row; a row that is not core takes the least number among its core neighbours, -1 without one."""
    A = np.asarray(A, dtype=bool)
    N = A.shape[0]
    core = A.sum(axis=1) >= int(min_samples)
    root = np.full(N, -1, dtype=np.int64)
    for i in np.flatnonzero(core):                                   # a search from every unvisited core row, in index order
        if root[i] >= 0:
            continue
        root[i] = i
        stack = [i]
        while stack:
            a = stack.pop()
            for b in np.flatnonzero(A[a] & core & (root < 0)):
                root[b] = i
                stack.append(b)
    roots = np.flatnonzero(core & (root == np.arange(N)))
    number = {int(r): n for n, r in enumerate(roots)}
    labels = np.full(N, -1, dtype=np.int64)
    for i in range(N):
        if core[i]:
            labels[i] = number[int(root[i])]
    core_labels = labels.copy()
    for i in np.flatnonzero(~core):
        near = np.flatnonzero(A[i] & core)
        if near.size:
            labels[i] = core_labels[near].min()
    border = int(((labels >= 0) & ~core).sum())
    return labels, core, [len(roots), int(core.sum()), border, int((labels < 0).sum())]


def same_partition(a, b):
    """Two labellings agree up to the numbering of the clusters (noise to noise)."""
    a, b = np.asarray(a), np.asarray(b)
    if not np.array_equal(a < 0, b < 0):
        return False
    pairs = set(zip(a[a >= 0].tolist(), b[b >= 0].tolist()))
    return len(pairs) == len({p[0] for p in pairs}) == len({p[1] for p in pairs})


# ------------------------------------------------------------------ fixtures
def distances64(X, metric):
    """fp64 distance matrix in the direct form (euclidean) / from normalised rows (cosine), zero diagonal."""
    X = np.asarray(X, dtype=np.float64)
    if metric == EUCLIDEAN:
        D = np.zeros((X.shape[0], X.shape[0]))
        for c in range(0, X.shape[1], 1024):                         # sum of squared differences, column blocks
            blk = X[:, c:c + 1024]
            sq = (blk * blk).sum(1)
            D += np.maximum(sq[:, None] + sq[None, :] - 2.0 * (blk @ blk.T), 0.0)
        D = np.sqrt(D)
    else:
        U = X / np.sqrt((X * X).sum(1))[:, None]
        D = np.maximum(1.0 - U @ U.T, 0.0)
    np.fill_diagonal(D, 0.0)
    return D


def lattice(N, D, offset, metric, seed=11):
    """Five 2-D blobs plus N // 12 uniform outliers, rounded to multiples of 1/4, embedded into D dimensions by two
    orthonormal columns, plus `offset` on every coordinate -> (X float32 [N, D], the 2-D points float64 [N, 2]).  For D >= 8
    the two columns are disjoint signed indicator vectors scaled by a power of two, so the embedding itself is exact in
    fp32; D = 3 uses the first two axes.
    The euclidean fixture spreads its blobs (sigma 0.45) over a square of side 7 about the origin: eps = 0.5295 then reaches
    two lattice steps.  About the origin, because the contraction sums a pair's D products in ONE fp32 chain and its error
    grows with the norms: with the blobs at 0 .. 7 and the offset 0.05 at D = 12 288 (squared norms up to 170) a host
    emulation of that chain is off by 0.07 in a distance, 65 x the e32 of torch's blocked sums, and flips 20 pairs.
    The cosine fixture puts them on a circle of radius 1.5 about the origin (sigma 0.3, outliers within +-2.5): a cosine
    distance sees directions only, and this close to the origin the lattice has few of them, so the sorted distances have
    gaps that dwarf fp32's error (the condition of test_dbscan_gpu.py, checked on the host before any launch)."""
    rng = np.random.default_rng(seed)
    n_out = N // 12
    n_in = N - n_out
    which = rng.integers(0, 5, n_in)
    if metric == EUCLIDEAN:
        centres = np.array([[-3.5, -3.5], [2.5, -2.5], [-2.5, 3.5], [3.5, 3.5], [0.0, 0.0]])
        pts = centres[which] + 0.45 * rng.standard_normal((n_in, 2))
        out = rng.uniform(-5.5, 5.5, (n_out, 2))
    else:
        ang = 2 * np.pi * (np.arange(5) / 5.0) + 0.3
        centres = 1.5 * np.stack([np.cos(ang), np.sin(ang)], 1)
        pts = centres[which] + 0.3 * rng.standard_normal((n_in, 2))
        out = rng.uniform(-2.5, 2.5, (n_out, 2))
    P = np.round(np.concatenate([pts, out]) * 4.0) / 4.0
    P = P[rng.permutation(N)]
    E = np.zeros((2, D))
    if D >= 8:
        m = 1 << int(np.floor(np.log2(D // 2)))                      # a power of two: 1 / sqrt(m) squares to an exact 1 / m
        m = m if int(np.log2(m)) % 2 == 0 else m // 2                # an even power: sqrt(m) itself is a power of two
        s = rng.choice([-1.0, 1.0], 2 * m)
        E[0, :m] = s[:m] / np.sqrt(m)
        E[1, m:2 * m] = s[m:] / np.sqrt(m)
    else:
        E[0, 0] = E[1, 1] = 1.0
    X = (P @ E + offset).astype(np.float32)
    return X, P


def e32_error(X, metric, eps):
    """The project's e32: the largest error of plain-fp32 torch (norms + matmul) against fp64 over the pairs with fp64 distance
    in [eps / 2, 2 eps] -> (e32, D64).  On the host."""
    import torch
    D64 = distances64(X, metric)
    T = torch.from_numpy(np.asarray(X, dtype=np.float32))
    G = T @ T.t()
    sq = (T * T).sum(1)
    if metric == EUCLIDEAN:
        D32 = torch.sqrt(torch.clamp(sq[:, None] + sq[None, :] - 2.0 * G, min=0.0))
    else:
        D32 = torch.clamp(1.0 - G / (torch.sqrt(sq)[:, None] * torch.sqrt(sq)[None, :]), min=0.0)
    D32 = D32.numpy().astype(np.float64)
    band = (D64 >= eps / 2) & (D64 <= 2 * eps)
    np.fill_diagonal(band, False)
    return (float(np.abs(D32 - D64)[band].max()) if band.any() else 0.0), D64


def cosine_eps(D64):
    """The midpoint of the widest gap of the sorted fp64 distances between their 3 % and 6 % quantiles."""
    d = np.sort(D64[np.triu_indices(D64.shape[0], 1)])
    lo, hi = int(0.03 * d.size), int(0.06 * d.size)
    seg = d[lo:hi + 1]
    g = int(np.argmax(np.diff(seg)))
    return float(0.5 * (seg[g] + seg[g + 1]))


def margin(D64, eps):
    """The least |d - eps| over the pairs (the diagonal apart)."""
    off = ~np.eye(D64.shape[0], dtype=bool)
    return float(np.abs(D64[off] - eps).min())
