"""numpy restatement of trustworthiness / continuity (vit_som_amd/embedding_quality.py, include/vitsom_hip.h:
vsom_knn_ranks) on full distance matrices, float64 or integer: the neighbours by (distance, index), the less / tied counts
of listed neighbours, the three tie policies, the penalties and sklearn's formula.  O(N^2 k) and plain on purpose: it is
what the kernels are compared against."""
import numpy as np

TIES = ("min", "max", "average")


def sq_distances(X):
    """Exact squared euclidean distances of integer rows, int64 [N, N]."""
    X = np.asarray(X)
    assert np.array_equal(X, np.round(X)), "integer-valued rows only"
    X = X.astype(np.int64)
    sq = (X * X).sum(1)
    return sq[:, None] + sq[None, :] - 2 * (X @ X.T)


def neighbours(D, k):
    """int64 [N, k]: every row's k nearest OTHER rows of the distance matrix D [N, N], ascending by (distance, index)."""
    D = np.asarray(D)
    N = D.shape[0]
    order = np.argsort(D, axis=1, kind="stable")                 # stable: equal distances keep ascending index
    out = np.empty((N, k), dtype=np.int64)
    for i in range(N):
        row = order[i]
        out[i] = row[row != i][:k]
    return out


def counts(D, nbr):
    """(less, tied) int64 [N, k] for the listed neighbours nbr [N, k] (-1 = empty): the rows l other than i and n = nbr[i, j]
    with D[i, l] < D[i, n], and with D[i, l] == D[i, n]; -1 in both for an empty slot and for n == i."""
    D, nbr = np.asarray(D), np.asarray(nbr)
    N, k = nbr.shape
    rows = np.arange(N)
    less = np.full((N, k), -1, dtype=np.int64)
    tied = np.full((N, k), -1, dtype=np.int64)
    diag = D[rows, rows]
    for j in range(k):
        n = nbr[:, j]
        valid = (n >= 0) & (n != rows)
        thr = D[rows, np.where(valid, n, 0)]
        lt = (D < thr[:, None]).sum(1) - (diag < thr)            # the neighbour's own column is never below itself
        eq = (D == thr[:, None]).sum(1) - (diag == thr) - 1      # ... and always equal to itself
        less[:, j] = np.where(valid, lt, -1)
        tied[:, j] = np.where(valid, eq, -1)
    return less, tied


def ranks(less, tied, ties="min"):
    """The rank of every listed neighbour among the other N - 1 rows (1 = nearest), float64 (halves for "average");
    NaN for an empty slot."""
    assert ties in TIES
    r = 1.0 + less + {"min": 0.0, "max": 1.0, "average": 0.5}[ties] * tied
    return np.where(less >= 0, r, np.nan)


def penalties(less, tied, k, ties="min"):
    """float64 [N]: per row the sum over its slots of max(rank - k, 0)."""
    r = ranks(less, tied, ties)
    return np.where(np.isnan(r), 0.0, np.maximum(r - k, 0.0)).sum(1)


def score(total, N, k):
    return 1.0 - total * (2.0 / (N * k * (2.0 * N - 3.0 * k - 1.0)))


def trustworthiness(DX, DE, k, ties="min"):
    """Neighbours in the embedding (DE), ranks in the data (DX); continuity is trustworthiness(DE, DX, k)."""
    less, tied = counts(DX, neighbours(DE, k))
    return score(penalties(less, tied, k, ties).sum(), DX.shape[0], k)


def counts_with_window(D, nbr, tol):
    """For the comparison of fp32 counts against float64 distances: (less, unsure) where unsure[i, j] is the number of rows
    l (other than i and n) with |D[i, l] - D[i, n]| <= max(tol[i, l], tol[i, n]): tol [N, N] is the tolerance of each entry
    of D, and two entries are told apart only when they differ by more than the larger of their tolerances."""
    D, nbr, tol = np.asarray(D), np.asarray(nbr), np.asarray(tol)
    N, k = nbr.shape
    rows = np.arange(N)
    less, _ = counts(D, nbr)
    unsure = np.zeros((N, k), dtype=np.int64)
    for j in range(k):
        n = nbr[:, j]
        valid = (n >= 0) & (n != rows)
        nn = np.where(valid, n, 0)
        thr, tn = D[rows, nn], tol[rows, nn]
        near = np.abs(D - thr[:, None]) <= np.maximum(tol, tn[:, None])
        near[rows, rows] = False
        near[rows, nn] = False
        unsure[:, j] = np.where(valid, near.sum(1), 0)
    return less, unsure
