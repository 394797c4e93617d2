"""Trustworthiness and continuity of an embedding (Venna & Kaski; sklearn.manifold.trustworthiness), on the device.  No
counterpart in the reference.

For N points in two spaces -- the data X [N, D] and a picture of it E [N, d] (a UMAP embedding, or the prototypes of a map
against their grid) -- and a neighbourhood size k:

    trustworthiness = 1 - 2 / (N k (2N - 3k - 1)) * sum_i sum_{j in kNN_E(i)} max(r_X(i, j) - k, 0)
    continuity      = the same with the two spaces exchanged

where kNN_E(i) are the k nearest other rows of i in E and r_X(i, j) is the rank of j among the other N - 1 rows by
distance from i in X (1 = nearest).  Trustworthiness falls when the picture shows neighbours the data does not have,
continuity when neighbours in the data were torn apart.

Nothing of size N x N is built: the neighbour lists are the exact search of `vsom_umap_knn` (k + 1 with the row itself
dropped: ties go to the lower index, as in UMAP's graph), and the ranks come from `vsom_knn_ranks`, which re-runs the same
contraction and counts, for every listed neighbour, how many other rows lie closer (`less`) and how many exactly as far
(`tied`).  The rest is integer arithmetic on the [N, k] counts on the host.

Ties.  With distinct distances the rank is 1 + less.  Where distances in the ranking space tie the rank of a neighbour is
a convention: ties="min" (the default) gives every tied row the lowest rank of the group, 1 + less, "max" the highest,
1 + less + tied, "average" their mean.  sklearn ranks by argsort of an fp64 distance matrix, which gives tied rows
consecutive ranks in index order: a value between "min" and "max"; on tie-free data all agree.  The distances compared
here are fp32 (the library's contraction), so rows closer together than its rounding may swap ranks against fp64.
"""
from dataclasses import dataclass

import numpy as np
import torch

from . import ops
from .umap import METRICS

TIES = ("min", "max", "average")
MAX_NEIGHBORS = ops.KNN_MAX_K - 1                       # the search returns the row itself first


@dataclass
class RankPenalties:
    """One direction of the measure: neighbours taken in B, ranked in A.  Arrays are host arrays of shape [N, k]."""
    total: object                        # sum of per_row: a Python int for ties "min" / "max", a float exact in halves for "average"
    per_row: np.ndarray                  # int64 [N] ("average": float64, exact in halves)
    neighbours: np.ndarray               # int64: the k nearest other rows in B, ascending by (distance, index)
    less: np.ndarray                     # int64: rows closer in A than the neighbour
    tied: np.ndarray                     # int64: other rows exactly as far in A as the neighbour


@dataclass
class EmbeddingQuality:
    """Host values of one embedding_quality call."""
    trustworthiness: float
    continuity: float
    n_neighbors: int
    n_samples: int
    trust_penalty: int                   # sum of max(rank in X - k, 0) over the neighbours in E
    cont_penalty: int                    # sum of max(rank in E - k, 0) over the neighbours in X
    trust_per_row: np.ndarray            # int64 [N]: a row's share of trust_penalty (points the picture puts among strangers)
    cont_per_row: np.ndarray             # int64 [N]: a row's share of cont_penalty (points torn from their neighbours)


def _metric(metric, who):
    if not isinstance(metric, str) or metric not in METRICS:
        raise ValueError(f"{who}: metric must be one of {sorted(METRICS)}, got {metric!r}")
    return METRICS[metric]


def _points(t, name, who):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2:
        raise ValueError(f"{who}: {name} must be a float32 [N, D] tensor on the GPU")
    return t if t.stride(1) == 1 else t.contiguous()


def _check_k(k, N, who):
    if int(k) != k or k < 1:
        raise ValueError(f"{who}: n_neighbors must be a positive integer, got {k!r}")
    if k >= N / 2:
        raise ValueError(f"n_neighbors ({k}) should be less than n_samples / 2 ({N / 2})")
    if k > MAX_NEIGHBORS:
        raise ValueError(f"{who}: n_neighbors={k} exceeds the kernel's limit of {MAX_NEIGHBORS}")


def penalties_from_counts(less, tied, k, ties="min"):
    """per-row sum over the slots of max(rank - k, 0) from the [N, k] counts (negative counts: an empty slot, no penalty).
    int64 for "min" / "max"; for "average" float64 holding exact halves."""
    less, tied = np.asarray(less, dtype=np.int64), np.asarray(tied, dtype=np.int64)
    valid = less >= 0
    if ties == "min":
        over = 1 + less - k
    elif ties == "max":
        over = 1 + less + tied - k
    elif ties == "average":
        over = 2 * (1 + less - k) + tied                     # in halves
    else:
        raise ValueError(f"ties must be one of {TIES}, got {ties!r}")
    per_row = np.where(valid, np.maximum(over, 0), 0).sum(axis=1)
    return per_row / 2.0 if ties == "average" else per_row


def score_from_penalty(total, N, k):
    """sklearn's expression, term for term."""
    return 1.0 - total * (2.0 / (N * k * (2.0 * N - 3.0 * k - 1.0)))


def rank_penalties(A, B, k, metric_a="euclidean", metric_b="euclidean", ties="min"):
    """Neighbours of every row in B [N, Db] (its k nearest other rows), ranked in A [N, Da] -> RankPenalties.  A and B are
    float32 device tensors over the same N points; k <= 63."""
    who = "rank_penalties"
    A, B = _points(A, "A", who), _points(B, "B", who)
    ma, mb = _metric(metric_a, who), _metric(metric_b, who)
    if ties not in TIES:
        raise ValueError(f"ties must be one of {TIES}, got {ties!r}")
    N = A.shape[0]
    if B.shape[0] != N:
        raise ValueError(f"{who}: A has {N} rows and B {B.shape[0]}")
    _check_k(k, N, who)
    k = int(k)
    idx = torch.empty(N, k + 1, dtype=torch.int64, device=B.device)
    dist = torch.empty(N, k + 1, dtype=torch.float32, device=B.device)
    ops.umap_knn(B, k + 1, mb, idx, dist)                    # row i first in its own list, whatever duplicates it has
    nbr = idx[:, 1:].contiguous()
    n_empty = int((nbr < 0).sum())                           # N > 2 k: a slot is empty only where a pair has no distance
    if n_empty:
        raise ValueError(f"{who}: {n_empty} neighbour slots are empty although N={N} exceeds n_neighbors={k}: B holds NaN or "
                         f"infinity, or a row's squared norm overflows float32")
    less = torch.empty(N, k, dtype=torch.int32, device=A.device)
    tied = torch.empty(N, k, dtype=torch.int32, device=A.device)
    ops.knn_ranks(A, nbr, ma, less, tied)
    n_unranked = int((less < 0).sum())                       # every slot names another row: -1 only where A has no distance
    if n_unranked:
        raise ValueError(f"{who}: {n_unranked} neighbours could not be ranked: A holds NaN or infinity, or a row's squared "
                         f"norm overflows float32")
    less_h, tied_h = less.cpu().numpy().astype(np.int64), tied.cpu().numpy().astype(np.int64)
    per_row = penalties_from_counts(less_h, tied_h, k, ties)
    total = sum(int(v) for v in (2 * per_row).astype(np.int64)) / 2 if ties == "average" else sum(int(v) for v in per_row)
    return RankPenalties(total=total, per_row=per_row, neighbours=nbr.cpu().numpy(), less=less_h, tied=tied_h)


def trustworthiness(X, E, n_neighbors=5, metric="euclidean", ties="min"):
    """sklearn.manifold.trustworthiness(X, E, n_neighbors=, metric=) for device tensors: neighbours in E (euclidean), ranks
    in X (`metric`).  Raises sklearn's ValueError when n_neighbors >= N / 2."""
    pen = rank_penalties(X, E, n_neighbors, metric, "euclidean", ties)
    return score_from_penalty(pen.total, X.shape[0], int(n_neighbors))


def continuity(X, E, n_neighbors=5, metric="euclidean", ties="min"):
    """The same with the roles exchanged: neighbours in X (`metric`), ranks in E (euclidean)."""
    pen = rank_penalties(E, X, n_neighbors, "euclidean", metric, ties)
    return score_from_penalty(pen.total, X.shape[0], int(n_neighbors))


def embedding_quality(X, E, n_neighbors=15, metric="cosine"):
    """Both measures of the embedding E [N, d] of the data X [N, D] (float32 device tensors) -> EmbeddingQuality; ties "min".
    Defaults are those of the project's UMAP plots (n_neighbors=15, metric='cosine')."""
    N, k = X.shape[0], int(n_neighbors)
    t = rank_penalties(X, E, k, metric, "euclidean")
    c = rank_penalties(E, X, k, "euclidean", metric)
    return EmbeddingQuality(trustworthiness=score_from_penalty(t.total, N, k), continuity=score_from_penalty(c.total, N, k),
                            n_neighbors=k, n_samples=N, trust_penalty=t.total, cont_penalty=c.total,
                            trust_per_row=t.per_row, cont_per_row=c.per_row)


def subset_scores(q: EmbeddingQuality, rows):
    """(trustworthiness, continuity) restricted to `rows` (a boolean mask or indices): the penalties of those rows alone,
    their neighbour lists still taken over all N points, normalised by their count in place of N."""
    rows = np.asarray(rows)
    n = int(rows.sum()) if rows.dtype == bool else len(rows)
    if n == 0:
        return float("nan"), float("nan")
    scale = 2.0 / (n * q.n_neighbors * (2.0 * q.n_samples - 3.0 * q.n_neighbors - 1.0))
    return (1.0 - sum(int(v) for v in q.trust_per_row[rows]) * scale, 1.0 - sum(int(v) for v in q.cont_per_row[rows]) * scale)
