"""numpy restatement of the silhouette coefficient in three parts: (1) the fp64 definition (what sklearn computes), (2) the
device's arithmetic from a given float32 distance matrix -- the power-of-two unit, rint to int64, integer sums --, (3) the
finishing expressions of csrc/knn.hip's sil_finish_kernel / sil_means_kernel, term for term."""
import numpy as np

COSINE, EUCLIDEAN = 0, 1                       # VSOM_DIST_*
FRAC = 40                                      # SIL_FRAC


# ------------------------------------------------------------------ (1) the definition, fp64
def distances(X, metric):
    """fp64 [N, N] distance matrix, zero diagonal (cosine of a zero row: 0 against a zero row, 1 against any other)."""
    X = np.asarray(X, dtype=np.float64)
    if metric == EUCLIDEAN:
        sq = (X * X).sum(1)
        D = np.sqrt(np.maximum(sq[:, None] + sq[None, :] - 2.0 * (X @ X.T), 0.0))
    else:
        n = np.sqrt((X * X).sum(1))
        with np.errstate(divide="ignore", invalid="ignore"):
            D = 1.0 - (X @ X.T) / (n[:, None] * n[None, :])
        zero = n == 0
        D[zero[:, None] & zero[None, :]] = 0.0
        D[zero[:, None] ^ zero[None, :]] = 1.0
        D = np.maximum(D, 0.0)
    np.fill_diagonal(D, 0.0)
    return D


def silhouette_fp64(D, labels):
    """-> (s, a, b) float64 [N] from a distance matrix: a = mean distance to the other members of the own cluster, b = the
    smallest mean distance to another cluster, s = (b - a) / max(a, b); s = 0 for a singleton and where 0 / 0 arises."""
    D = np.asarray(D, dtype=np.float64)
    names, dense = np.unique(np.asarray(labels), return_inverse=True)
    N, C = len(dense), len(names)
    onehot = np.zeros((N, C))
    onehot[np.arange(N), dense] = 1.0
    counts = onehot.sum(0)
    sums = D @ onehot
    own = sums[np.arange(N), dense]
    with np.errstate(divide="ignore", invalid="ignore"):
        a = own / (counts[dense] - 1.0)
        means = sums / counts[None, :]
        means[np.arange(N), dense] = np.inf
        b = means.min(1)
        s = (b - a) / np.maximum(a, b)
    s[counts[dense] == 1] = 0.0
    return np.nan_to_num(s), a, b


# ------------------------------------------------------------------ (2) the device's sums
def bound_exponent(max_sqnorm, metric):
    """e with 2^e the smallest power of two > 4 sqrt(max squared norm) (frexp: M < 2^x, e = ceil((x + 4) / 2)); cosine: 2."""
    if metric == COSINE:
        return 2
    M = np.float32(max_sqnorm)
    if M == 0:
        return 0
    x = int(np.frexp(M)[1])
    return (x + 5) >> 1


def fixed_sums(D32, labels, n_clusters, e):
    """S int64 [N, C]: per row and cluster the sum of rint(d 2^(40 - e)) over the cluster's members other than the row
    itself, from the float32 distances D32 [N, N].  A label outside [0, C) neither gives nor receives."""
    D32 = np.asarray(D32)
    assert D32.dtype == np.float32
    labels = np.asarray(labels, dtype=np.int64)
    N = len(labels)
    q = np.rint(D32.astype(np.float64) * 2.0 ** (FRAC - e))
    assert q.max() < 2.0 ** FRAC
    q = q.astype(np.int64)
    np.fill_diagonal(q, 0)
    ok = (labels >= 0) & (labels < n_clusters)
    S = np.zeros((N, n_clusters), dtype=np.int64)
    for c in range(n_clusters):
        members = ok & (labels == c)
        if members.any():
            S[:, c] = q[:, members].sum(1)
    S[~ok] = 0
    return S


# ------------------------------------------------------------------ (3) the finishing expressions
def finish(S, labels, n_clusters, e):
    """-> dict(sil, a, b, nearest, counts, cluster_mean, score, status) as the device computes them from the sums."""
    labels = np.asarray(labels, dtype=np.int64)
    N, C = len(labels), n_clusters
    ok = (labels >= 0) & (labels < C)
    counts = np.bincount(labels[ok], minlength=C).astype(np.int64)
    unit = 2.0 ** (e - FRAC)
    sil, a, b = np.full(N, np.nan), np.full(N, np.nan), np.full(N, np.nan)
    nearest = np.full(N, -1, dtype=np.int64)
    for i in np.flatnonzero(ok):
        own = labels[i]
        best, arg = np.inf, -1
        for c in range(C):
            if c == own or counts[c] == 0:
                continue
            v = float(S[i, c]) * unit / float(counts[c])
            if v < best:
                best, arg = v, c
        n_own = counts[own]
        a[i] = float(S[i, own]) * unit / float(n_own - 1) if n_own > 1 else 0.0
        b[i] = best if arg >= 0 else np.nan
        nearest[i] = arg
        s = 0.0
        if n_own > 1 and arg >= 0:
            m = max(a[i], b[i])
            if m > 0.0:
                s = (b[i] - a[i]) / m
        sil[i] = s
    q = np.rint(np.where(ok, sil, 0.0) * 2.0 ** FRAC).astype(np.int64)
    acc = np.zeros(C, dtype=np.int64)
    np.add.at(acc, labels[ok], q[ok])
    with np.errstate(divide="ignore", invalid="ignore"):
        cluster_mean = np.where(counts > 0, acc.astype(np.float64) * 2.0 ** -FRAC / counts, np.nan)
    counted = int(ok.sum())
    score = float(int(q.sum())) * 2.0 ** -FRAC / counted if counted else np.nan
    status = [int((~ok).sum()), 0, int((counts > 0).sum()), int((counts == 1).sum())]
    return dict(sil=sil, a=a, b=b, nearest=nearest, counts=counts, cluster_mean=cluster_mean, score=score, status=status)


def device_restatement(D32, labels, n_clusters, max_sqnorm, metric):
    """(S, finish(...)) for the float32 distances D32."""
    e = bound_exponent(max_sqnorm, metric)
    S = fixed_sums(D32, labels, n_clusters, e)
    return S, finish(S, labels, n_clusters, e)


def exact_euclidean32(X):
    """Integer rows whose dot products and norms stay below 2^24: (float32 distances, max squared norm), both exactly what
    the device computes -- every squared distance is an integer exact in fp32 and sqrtf is correctly rounded."""
    X = np.asarray(X, dtype=np.int64)
    G = X @ X.T
    sq = np.diag(G)
    assert np.abs(G).max() < 2 ** 24 and (sq[:, None] + sq[None, :]).max() < 2 ** 24
    D2 = sq[:, None] + sq[None, :] - 2 * G
    return np.sqrt(D2.astype(np.float32)), int(sq.max())
