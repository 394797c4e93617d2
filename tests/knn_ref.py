"""numpy float64 restatement of the kNN probe (include/vitsom_hip.h: vsom_knn_query, vsom_knn_vote): brute-force
distances with the header's conventions, the (distance, index) top-k with streaming, exclusion and the (+inf, -1) tail,
and the three vote rules with their fixed summation order.  Slow and plain on purpose: it is what the kernels are
compared against."""
import numpy as np

COSINE, EUCLIDEAN = 0, 1                       # VSOM_DIST_*
UNIFORM, DISTANCE, SOFTMAX = 0, 1, 2           # VSOM_KNN_*


def distances(Q, X, metric):
    """float64 [Nq, Nb].  euclidean: the true distance.  cosine: 1 - cos clamped at 0; 0 between two zero rows, 1 between a
    zero row and any other; exactly 0 between identical rows."""
    Q, X = np.asarray(Q, dtype=np.float64), np.asarray(X, dtype=np.float64)
    if metric == EUCLIDEAN:
        return np.sqrt(((Q[:, None, :] - X[None, :, :]) ** 2).sum(-1))
    assert metric == COSINE
    nq, nx = np.sqrt((Q * Q).sum(1)), np.sqrt((X * X).sum(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.maximum(1.0 - (Q @ X.T) / (nq[:, None] * nx[None, :]), 0.0)
    zq, zx = (nq == 0)[:, None], (nx == 0)[None, :]
    d = np.where(zq & zx, 0.0, np.where(zq | zx, 1.0, d))
    same = (Q[:, None, :] == X[None, :, :]).all(-1)
    return np.where(same & ~(zq | zx), 0.0, d)


def empty_lists(Nq, k):
    return np.full((Nq, k), -1, dtype=np.int64), np.full((Nq, k), np.inf, dtype=np.float64)


def fold(idx, dist, D, index_base=0, exclude=None):
    """Fold the distance block D [Nq, Nb] of bank rows index_base .. index_base + Nb - 1 into the lists (idx, dist):
    per query the k smallest of list and block by (distance, ordinal); exclude[i] is an ordinal query i never receives.
    Returns new (idx, dist); empty slots are (-1, +inf)."""
    Nq, k = idx.shape
    out_i, out_d = empty_lists(Nq, k)
    for i in range(Nq):
        cand = [(float(dist[i, j]), int(idx[i, j])) for j in range(k) if idx[i, j] >= 0]
        for j in range(D.shape[1]):
            g = index_base + j
            if exclude is not None and int(exclude[i]) == g:
                continue
            if not np.isnan(D[i, j]):
                cand.append((float(D[i, j]), g))
        cand.sort()
        for j, (dv, g) in enumerate(cand[:k]):
            out_i[i, j], out_d[i, j] = g, dv
    return out_i, out_d


def topk(D, k, index_base=0, exclude=None):
    idx, dist = empty_lists(D.shape[0], k)
    return fold(idx, dist, D, index_base, exclude)


def vote(idx, dist, bank_labels, n_classes, weights, temperature=0.07):
    """-> (pred int64 [Nq], scores float64 [Nq, n_classes], status [refused neighbours, queries without one]).
    dist holds the STORED distances (float32 values); the weight arithmetic is float64 and the scores are added in
    neighbour order j = 0 .. k-1.  The first argmax wins."""
    idx, dist = np.asarray(idx), np.asarray(dist)
    Nq, k = idx.shape
    n_bank = len(bank_labels)
    pred = np.full(Nq, -1, dtype=np.int64)
    scores = np.zeros((Nq, n_classes), dtype=np.float64)
    status = [0, 0]
    T = np.float64(np.float32(temperature))
    for i in range(Nq):
        counted = []
        for j in range(k):
            n = int(idx[i, j])
            if n < 0:
                continue
            if n >= n_bank or not 0 <= int(bank_labels[n]) < n_classes:
                status[0] += 1
                continue
            counted.append((int(bank_labels[n]), np.float64(np.float32(dist[i, j]))))
        if not counted:
            status[1] += 1
            continue
        any_zero = any(d == 0.0 for _, d in counted)
        d_min = min(d for _, d in counted)               # softmax: the weights up to the common factor exp(d_min / T)
        for c, d in counted:
            if weights == UNIFORM:
                w = np.float64(1.0)
            elif weights == DISTANCE:
                w = np.float64(1.0 if d == 0.0 else 0.0) if any_zero else np.float64(1.0) / d
            else:
                w = np.exp(-(d - d_min) / T)
            scores[i, c] = scores[i, c] + w
        pred[i] = int(np.argmax(scores[i]))
    return pred, scores, status
