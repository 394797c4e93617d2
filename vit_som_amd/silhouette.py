"""Silhouette coefficient (Rousseeuw 1987; sklearn.metrics.silhouette_samples / silhouette_score) on the device: how
compact and how well separated the clusters of a labelling are in the space of X, without ground-truth labels.  No
counterpart in the reference.

For sample i in cluster A:

    a(i) = mean distance from i to the other members of A
    b(i) = the smallest mean distance from i to the members of any other cluster
    s(i) = (b - a) / max(a, b)            in [-1, 1]; 0 for a cluster of one, 0 where a = b = 0

Nothing of size N x N is built and X never leaves the device: `vsom_silhouette` re-runs the all-pairs contraction of the
neighbour search (csrc/knn.hip), dot products and norms summed in segments of 128 values (shorter fp32 chains than the
search's: more accurate for D > 128), and adds every distance, in fixed point, into a per-(row, cluster) integer sum.  Integer
sums do not depend on their order: every value is bitwise reproducible and does not depend on the order of the rows.
The distances are fp32 (the library's contraction), so values differ from sklearn's fp64 ones by the rounding of those
distances, a few 2^-24 relative; `score` and `per_cluster` are means taken from integer sums of s rounded to 2^-40.

Metrics: "euclidean" and "cosine" (the cosine distance of vsom_umap_knn: 0 between two zero rows, 1 between a zero row
and any other).
"""
from dataclasses import dataclass

import numpy as np
import torch

from . import ops
from .umap import METRICS

MAX_SAMPLES = ops.SILHOUETTE_MAX_N
SORT_ROWS = True                         # the default of every entry point here; see cluster_silhouette


@dataclass
class SilhouetteReport:
    """cluster_silhouette's result.  Cluster c of the arrays is the c-th distinct label in ascending order (`labels_`), or
    label c itself when n_clusters was given."""
    score: float                         # mean of per_sample
    per_sample: torch.Tensor             # float64 [N], device
    per_cluster: np.ndarray              # float64 [C], host: mean of per_sample over the cluster, NaN for an empty one
    counts: np.ndarray                   # int64 [C], host
    nearest_cluster: torch.Tensor        # int64 [N], device: the cluster that gives b(i)
    n_clusters: int                      # C
    n_samples: int
    metric: str
    labels_: np.ndarray = None           # int64 [C], host: the label each cluster stands for
    inference_time: float = 0.0


def _check(X, labels, metric, who):
    if not isinstance(metric, str) or metric not in METRICS:
        raise ValueError(f"{who}: metric must be one of {sorted(METRICS)}, got {metric!r}")
    if not isinstance(X, torch.Tensor) or not X.is_cuda or X.dtype != torch.float32 or X.dim() != 2:
        raise ValueError(f"{who}: X must be a float32 [N, D] tensor on the GPU")
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64 or labels.dim() != 1 or labels.device != X.device:
        raise ValueError(f"{who}: labels must be an int64 [N] tensor on the device of X")
    if labels.shape[0] != X.shape[0]:
        raise ValueError(f"Found input variables with inconsistent numbers of samples: [{X.shape[0]}, {labels.shape[0]}]")
    return X if X.stride(1) == 1 else X.contiguous()


def check_number_of_labels(n_labels, n_samples):
    """sklearn.metrics.cluster._unsupervised.check_number_of_labels, word for word."""
    if not 1 < n_labels < n_samples:
        raise ValueError("Number of labels is %d. Valid values are 2 to n_samples - 1 (inclusive)" % n_labels)


def _run(X, labels, metric, n_clusters, sort_rows, who):
    """-> (ops.Silhouette in the caller's row order, the label of every cluster).  n_clusters None: the distinct labels are
    mapped to 0 .. C - 1 on the device; otherwise labels are cluster ids in [0, n_clusters) and some may have no member."""
    X = _check(X, labels, metric, who)
    N = X.shape[0]
    if N > MAX_SAMPLES:
        raise ValueError(f"{who}: {N} samples exceed the kernel's limit of {MAX_SAMPLES} (silhouette_score: pass sample_size=)")
    if n_clusters is None:
        names, dense = torch.unique(labels, return_inverse=True)
        C = int(names.numel())
        check_number_of_labels(C, N)
        names = names.cpu().numpy()
    else:
        C, dense = int(n_clusters), labels.contiguous()
        if C < 1:
            raise ValueError(f"{who}: n_clusters must be positive, got {n_clusters!r}")
        names = np.arange(C, dtype=np.int64)
    if sort_rows:
        order = torch.argsort(dense, stable=True)
        res = ops.silhouette(X[order], dense[order].contiguous(), METRICS[metric], C)
        for name in ("sil", "a", "b", "nearest"):
            back = torch.empty_like(getattr(res, name))
            back[order] = getattr(res, name)
            setattr(res, name, back)
    else:
        res = ops.silhouette(X, dense.contiguous(), METRICS[metric], C)
    if res.status[0]:
        raise ValueError(f"{who}: {res.status[0]} labels fall outside [0, {C})")
    if n_clusters is not None:
        check_number_of_labels(res.status[2], N)           # the labels present, as sklearn counts them
    return res, names


def _report(res, names, metric, N):
    return SilhouetteReport(score=float(res.score.item()), per_sample=res.sil, per_cluster=res.cluster_mean.cpu().numpy(),
                            counts=res.counts.cpu().numpy(), nearest_cluster=res.nearest, n_clusters=len(names), n_samples=N,
                            metric=metric, labels_=names)


def cluster_silhouette(X, labels, metric="euclidean", n_clusters=None, sort_rows=SORT_ROWS):
    """-> SilhouetteReport of the float32 device tensor X [N, D] under the int64 device labels [N].  Labels need not be
    dense: the distinct values become clusters 0 .. C - 1 in ascending order (`labels_`).  With n_clusters the labels are
    taken as cluster ids in [0, n_clusters) as they are -- a SOM's units, say -- and an id without a member is an empty
    cluster: skipped for b, NaN in per_cluster, not counted where sklearn counts labels.
    Raises sklearn's ValueError unless 2 <= distinct labels <= N - 1, and ValueError for NaN or infinite input.
    sort_rows: hand the kernel the rows sorted by label (a stable argsort, a gathered copy of X, results scattered back).
    The result is bit for bit the same either way; the copy costs another N * D * 4 bytes of device memory while the
    call runs (469 MiB at 10 000 x 12 288), and turns the kernel's one atomic per (row, label change) into about one per
    (row, 64 columns).  Measured on shuffled labels (profiles/r14_silhouette.txt, N = 10 000): the kernel alone takes 1.29
    ms on sorted against 2.53 ms on shuffled rows at D = 192; at D = 12 288 the whole call with the sort takes 1.004 of the
    call without at 10 clusters (inside the spread) and 0.982 at 1 600.  Hence the default."""
    res, names = _run(X, labels, metric, n_clusters, sort_rows, "cluster_silhouette")
    return _report(res, names, metric, X.shape[0])


def silhouette_samples(X, labels, metric="euclidean", sort_rows=SORT_ROWS):
    """sklearn.metrics.silhouette_samples(X, labels, metric=) for device tensors -> float64 device tensor [N]."""
    return _run(X, labels, metric, None, sort_rows, "silhouette_samples")[0].sil


def silhouette_score(X, labels, metric="euclidean", sample_size=None, random_state=None, sort_rows=SORT_ROWS):
    """sklearn.metrics.silhouette_score for device tensors -> float.  sample_size: the score of the subset
    numpy.random.RandomState(random_state).permutation(N)[:sample_size] -- sklearn's draw -- gathered on the device."""
    _check(X, labels, metric, "silhouette_score")
    if sample_size is not None:
        idx = np.random.RandomState(random_state).permutation(X.shape[0])[:sample_size]
        idx = torch.from_numpy(idx).to(X.device)
        X, labels = X[idx], labels[idx]
    return float(_run(X, labels, metric, None, sort_rows, "silhouette_score")[0].score.item())
