"""sklearn.cluster.DBSCAN (sklearn/cluster/_dbscan.py; Ester, Kriegel, Sander and Xu 1996) on the device: density clusters
and, first class, the samples that belong to none.  With it k_distances (the curve one reads eps from), evaluate_dbscan and
visualize_dbscan for the latents the SOM layer sees.  No counterpart in the reference.

The expensive part is the eps-neighbourhood graph: `vsom_dbscan_neighbours` (csrc/knn.hip) re-runs the all-pairs
contraction of the neighbour search on the f32 matrix cores and keeps one BIT per pair -- bit j & 63 of word [i, j >> 6] is
set iff rows i and j have a distance <= eps, the diagonal set (a row is in its own neighbourhood, as in sklearn), N^2 / 8
bytes in all.  The rest walks those bits: the connected components of the core rows (count >= min_samples) by hooking and
pointer jumping, `vsom_dbscan_round`, repeated until a call moves nothing -- the host reads one int32 per call of
ROUNDS_PER_CALL rounds -- and `vsom_dbscan_finish`, which numbers the clusters by their smallest core row and gives a
border row the smallest number among its core neighbours.  Both rules are what sklearn's index-ordered expansion
produces, so labels_ equals sklearn's label for label, not just partition for partition.  No floating-point atomics, one
summation order, a unique fixed point: two fits are bitwise equal, whatever the chunking and the races.

Departures from sklearn, all stated here and in INTEGRATION.md:
* sample_weight is refused: the core test counts set bits (an integer popcount of the row), there is no weighted sum.
* algorithm, leaf_size, p and n_jobs are validated as sklearn validates them and then ignored: the search is exact and
  brute force, there is no tree to tune.  metric_params must be None or empty.
* metric is one of "euclidean", "l2", "cosine", "precomputed"; no callable, and none of sklearn's other names.
* N <= 131 072 (the bit matrix is then 2 GiB).
* The neighbourhood test is (double)d <= eps on the fp32 distance of vsom_umap_knn: a pair whose true distance is within
  fp32 rounding of eps may fall on either side.  For data whose column means are large against its spread use
  metric="precomputed" with ops.agglo_distances (the fp64 direct form; manhattan too).
* A row with a NaN, an infinity or an overflowing norm raises ValueError ("... not finite"), as silhouette.py does.
"""
import numbers
import time
from dataclasses import dataclass

import numpy as np
import torch

from . import ops
from .umap import METRICS

MAX_SAMPLES = ops.DBSCAN_MAX_N
ROUNDS_PER_CALL = 4                      # hook + jump pairs enqueued per host read of `changed` (DBSCAN)
MAX_K = 63                               # k_distances: umap_knn lists at most 64 rows, the row itself among them
_METRICS = {"euclidean": ops.DIST_EUCLIDEAN, "l2": ops.DIST_EUCLIDEAN, "cosine": ops.DIST_COSINE, "precomputed": None}
_ALGORITHMS = ("auto", "ball_tree", "kd_tree", "brute")
# the names sklearn 1.7.2 lists for DBSCAN's metric (its message prints them as a set, in no fixed order)
SKLEARN_METRICS = ("braycurtis", "canberra", "chebyshev", "cityblock", "correlation", "cosine", "dice", "euclidean", "hamming",
                   "haversine", "jaccard", "l1", "l2", "mahalanobis", "manhattan", "matching", "minkowski", "nan_euclidean",
                   "precomputed", "rogerstanimoto", "russellrao", "seuclidean", "sokalmichener", "sokalsneath", "sqeuclidean",
                   "wminkowski", "yule")
SAMPLE_WEIGHT = ("DBSCAN: sample_weight is not supported: a row is core when the popcount of its row of the bit matrix "
                 "reaches min_samples, and that count has no weights")


def _options(values):
    return "{" + ", ".join(repr(v) for v in values) + "}"


class DBSCAN:
    """sklearn.cluster.DBSCAN for float32 [N, D] device tensors (a row stride is fine; metric "precomputed": a float32 or
    float64 [N, N] device tensor of distances, symmetric), N <= 131 072.  Names, defaults and parameter error sentences are
    sklearn's.  fit / fit_predict.  Fitted: labels_ int64 [N] on the device, sklearn's numbering, -1 for noise;
    core_sample_indices_ int64 on the device, ascending; components_ (the core rows of X); n_features_in_.

    NOT in sklearn: n_clusters_, n_noise_, n_core_, n_border_ (host ints), n_round_calls_ (the vsom_dbscan_round calls
    the components took) and, with fit(..., keep_graph=True), neighbourhoods_: the bit matrix, int64 [N, ceil(N / 64)]
    on the device (None otherwise).

    Departures: sample_weight is refused (the core test is a popcount); algorithm, leaf_size, p and n_jobs are validated
    and ignored (the search is exact); no callable metric, "euclidean" / "l2" / "cosine" / "precomputed" only; the
    neighbourhood test is on the fp32 distance of vsom_umap_knn, so a pair within fp32 rounding of eps may fall on either
    side (offset-heavy data: metric="precomputed" with ops.agglo_distances); rows that are not finite raise ValueError."""

    def __init__(self, eps=0.5, *, min_samples=5, metric="euclidean", metric_params=None, algorithm="auto", leaf_size=30, p=None,
                 n_jobs=None):
        self.eps, self.min_samples, self.metric, self.metric_params = eps, min_samples, metric, metric_params
        self.algorithm, self.leaf_size, self.p, self.n_jobs = algorithm, leaf_size, p, n_jobs

    def _check_params(self):
        e = self.eps
        if not isinstance(e, numbers.Real) or not 0 < e < float("inf"):
            raise ValueError(f"The 'eps' parameter of DBSCAN must be a float in the range (0.0, inf). Got {e!r} instead.")
        if callable(self.metric):                                    # a departure: sklearn takes one
            raise ValueError("DBSCAN: a callable metric is not supported: the distances come from one contraction on the matrix "
                             "cores; pass the callable's distance matrix with metric='precomputed'")
        m = self.min_samples
        if not isinstance(m, numbers.Integral) or m < 1:
            raise ValueError(f"The 'min_samples' parameter of DBSCAN must be an int in the range [1, inf). Got {m!r} instead.")
        if not (isinstance(self.metric, str) and self.metric in SKLEARN_METRICS):
            raise ValueError(f"The 'metric' parameter of DBSCAN must be a str among {_options(SKLEARN_METRICS)} or a callable. "
                             f"Got {self.metric!r} instead.")
        if self.metric_params is not None and not isinstance(self.metric_params, dict):
            raise ValueError(f"The 'metric_params' parameter of DBSCAN must be an instance of 'dict' or None. "
                             f"Got {self.metric_params!r} instead.")
        if not (isinstance(self.algorithm, str) and self.algorithm in _ALGORITHMS):
            raise ValueError(f"The 'algorithm' parameter of DBSCAN must be a str among {_options(_ALGORITHMS)}. "
                             f"Got {self.algorithm!r} instead.")
        if not isinstance(self.leaf_size, numbers.Integral) or self.leaf_size < 1:
            raise ValueError(f"The 'leaf_size' parameter of DBSCAN must be an int in the range [1, inf). "
                             f"Got {self.leaf_size!r} instead.")
        if self.p is not None and (not isinstance(self.p, numbers.Real) or not self.p >= 0):
            raise ValueError(f"The 'p' parameter of DBSCAN must be a float in the range [0.0, inf) or None. Got {self.p!r} instead.")
        if self.n_jobs is not None and not isinstance(self.n_jobs, numbers.Integral):
            raise ValueError(f"The 'n_jobs' parameter of DBSCAN must be an instance of 'int' or None. Got {self.n_jobs!r} instead.")
        # the departures: what sklearn takes and this class does not
        if self.metric not in _METRICS:
            raise ValueError(f"DBSCAN: metric {self.metric!r} is not supported: the contraction computes {sorted(_METRICS)[:3]}; "
                             f"for any other metric pass its distance matrix with metric='precomputed' (ops.agglo_distances "
                             f"has manhattan)")
        if self.metric_params:
            raise ValueError(f"DBSCAN: metric_params {self.metric_params!r} is not supported: none of the metrics takes a parameter")

    def _check_x(self, X):
        if not (isinstance(X, torch.Tensor) and X.is_cuda):
            raise ValueError("DBSCAN: X must be a tensor on the GPU")
        if X.dim() != 2:
            raise ValueError(f"Expected 2D array, got {X.dim()}D tensor instead.")
        N, D = X.shape
        if self.metric == "precomputed":
            if X.dtype not in (torch.float32, torch.float64):
                raise ValueError("DBSCAN: a precomputed X must be float32 or float64")
            if N != D:
                raise ValueError(f"Precomputed matrix must be square. Input is a {N}x{D} matrix.")
        elif X.dtype != torch.float32:
            raise ValueError("DBSCAN: X must be a float32 [N, D] tensor on the GPU")
        if N < 1:
            raise ValueError(f"Found array with {N} sample(s) (shape=({N}, {D})) while a minimum of 1 is required by DBSCAN.")
        if D < 1:
            raise ValueError(f"Found array with {D} feature(s) (shape=({N}, {D})) while a minimum of 1 is required by DBSCAN.")
        if N > MAX_SAMPLES:
            raise ValueError(f"DBSCAN: {N} rows > {MAX_SAMPLES}, the most the kernels take (the bit matrix would pass 2 GiB)")
        if X.stride(1) != 1 or (X.dtype == torch.float64 and not X.is_contiguous()):
            X = X.contiguous()
        return X

    def _single_row(self, X, keep_graph):
        """N = 1 (the kernels start at two rows): the row is its own neighbourhood."""
        dev, core = X.device, int(self.min_samples) <= 1
        if not bool(torch.isfinite(X).all()):
            raise ValueError("DBSCAN: 1 row of X is not finite")
        self.labels_ = torch.full((1,), 0 if core else -1, dtype=torch.int64, device=dev)
        self.core_sample_indices_ = torch.arange(1 if core else 0, dtype=torch.int64, device=dev)
        self.n_clusters_, self.n_core_, self.n_border_, self.n_noise_ = int(core), int(core), 0, int(not core)
        self.n_round_calls_ = 0
        self.neighbourhoods_ = torch.ones(1, 1, dtype=torch.int64, device=dev) if keep_graph else None

    def fit(self, X, y=None, sample_weight=None, keep_graph=False):
        self._check_params()
        if sample_weight is not None:
            raise ValueError(SAMPLE_WEIGHT)
        X = self._check_x(X)
        N, dev = X.shape[0], X.device
        self.n_features_in_ = int(X.shape[1])
        if N == 1:
            self._single_row(X, keep_graph)
            self.components_ = X[self.core_sample_indices_]
            return self
        new = lambda dtype, *shape: torch.empty(*shape, dtype=dtype, device=dev)      # noqa: E731
        adj, count, status = new(torch.int64, N, ops.dbscan_words(N)), new(torch.int32, N), new(torch.int64, 2)
        if self.metric == "precomputed":
            if bool((X < 0).any()):
                raise ValueError("Negative values in data passed to X.")
            ops.dbscan_threshold(X, float(self.eps), adj, count, status)
            bad = int(status[0].item())
            if bad:
                raise ValueError(f"DBSCAN: the precomputed matrix is not finite: {bad} of its entries are NaN")
        else:
            ops.dbscan_neighbours(X, _METRICS[self.metric], float(self.eps), new(torch.float32, N), adj, count, status)
            bad = int(status[0].item())
            if bad:
                raise ValueError(f"DBSCAN: {bad} rows of X are not finite: they hold NaN or infinity, or their squared norm "
                                 f"overflows float32")
        core, root, changed = new(torch.uint8, N), new(torch.int32, N), new(torch.int32, 1)
        ops.dbscan_init(count, int(self.min_samples), core, root)
        calls = 0
        while True:
            ops.dbscan_round(adj, core, root, ROUNDS_PER_CALL, changed)
            calls += 1
            if not int(changed.item()):                              # THE host read of a call
                break
            if calls > N:                                            # every moving round lowers a root; N rounds cannot all move
                raise RuntimeError(f"DBSCAN: the components did not reach their fixed point in {calls} round calls")
        labels, record = new(torch.int64, N), new(torch.int32, 4)
        ops.dbscan_finish(adj, core, root, labels, record)
        rec = record.tolist()
        self.labels_ = labels
        self.core_sample_indices_ = torch.nonzero(core).view(-1)
        self.components_ = X[self.core_sample_indices_]
        self.n_clusters_, self.n_core_ = rec[ops.DBSCAN_CLUSTERS], rec[ops.DBSCAN_CORE]
        self.n_border_, self.n_noise_ = rec[ops.DBSCAN_BORDER], rec[ops.DBSCAN_NOISE]
        self.n_round_calls_ = calls
        self.neighbourhoods_ = adj if keep_graph else None
        return self

    def fit_predict(self, X, y=None, sample_weight=None):
        return self.fit(X, sample_weight=sample_weight).labels_


def k_distances(X, k, metric="euclidean"):
    """The distance of every row of X (float32 [N, D] on the device) to its k-th OTHER neighbour, sorted ascending ->
    float32 [N] on the device: the curve one reads eps from (Ester et al., section 4.2: min_samples = k + 1 and eps at the
    knee).  Through ops.umap_knn, whose lists begin with the row itself: 1 <= k <= 63, k + 1 < N.  A row that is not finite
    has no neighbours: its value is +inf, at the end."""
    if not isinstance(metric, str) or metric not in METRICS:
        raise ValueError(f"k_distances: metric must be one of {sorted(METRICS)}, got {metric!r}")
    if not isinstance(X, torch.Tensor) or not X.is_cuda or X.dtype != torch.float32 or X.dim() != 2:
        raise ValueError("k_distances: X must be a float32 [N, D] tensor on the GPU")
    if isinstance(k, bool) or not isinstance(k, numbers.Integral) or not 1 <= k <= MAX_K:
        raise ValueError(f"k_distances: k must be an int in [1, {MAX_K}], got {k!r}")
    N = X.shape[0]
    if k + 1 >= N:
        raise ValueError(f"k_distances: k + 1 = {k + 1} must be below the number of rows, {N}")
    X = X if X.stride(1) == 1 else X.contiguous()
    idx = torch.empty(N, k + 1, dtype=torch.int64, device=X.device)
    dist = torch.empty(N, k + 1, dtype=torch.float32, device=X.device)
    ops.umap_knn(X, k + 1, METRICS[metric], idx, dist)
    return torch.sort(dist[:, k]).values


# ------------------------------------------------------------------------------------ the latents' density clusters
@dataclass
class DBSCANReport:
    """Host values of one evaluate_dbscan pass (labels and k_distances stay on the device)."""
    eps: float
    min_samples: int
    metric: str
    n_clusters: int
    n_core: int
    n_border: int
    n_noise: int
    coverage: float                      # the share of the samples that are in a cluster
    cluster_sizes: np.ndarray            # int64 [n_clusters]
    purity: float                        # over the clustered samples only; NaN when nothing is clustered
    nmi: float                           # likewise
    noise_per_class: np.ndarray          # int64 [classes]: the noise rows of every ground-truth label
    k_distances: torch.Tensor            # float32 [N] on the device, ascending: k_distances(X, min_samples - 1)
    labels: torch.Tensor                 # int64 [N] on the device, loader order (all ranks' rows, rank 0's first); -1 noise
    n_samples: int
    inference_time: float


def eps_from_k_distances(curve, eps_quantile):
    """The stated rule for eps=None: the element of the ascending k-distance curve [N] at index
    min(floor(eps_quantile N), N - 1) -- a value the curve attains, so at least that share of the rows has its k-th
    neighbour within eps and is core."""
    if not 0.0 <= float(eps_quantile) <= 1.0:
        raise ValueError(f"evaluate_dbscan: eps_quantile must lie in [0, 1], got {eps_quantile!r}")
    n = curve.shape[0]
    return float(curve[min(int(float(eps_quantile) * n), n - 1)].item())


def _latents_and_labels(model, config, dataloader, who):
    """(the rows evaluation._som_latents returns, the loader's labels): one pass, the whole set on every rank."""
    from . import evaluation as E                         # its loader pass and model adapter; evaluation imports this module
    arch = E._Arch(model, config, who).require("som_input")
    return E._whole_set(arch, dataloader, lambda x: arch.som_input(x)[0], labels=True)


@torch.no_grad()
def evaluate_dbscan(model, config, dataloader, eps=None, min_samples=5, metric=None, eps_quantile=0.5):
    """DBSCAN of the latents the SOM layer sees (the rows of evaluate_silhouette) -> DBSCANReport: how many density clusters
    they form, which samples belong to none, and purity / NMI against the loader's labels over the CLUSTERED samples only
    (the noise rows are reported per class instead of being counted against a cluster).
    metric: "cosine" or "euclidean"; None takes the SOM's distance_fcn when it is one of the two and "euclidean" otherwise.
    eps None: the eps_quantile quantile of k_distances(X, min_samples - 1) (eps_from_k_distances) -- a stated rule, not a
        tuned one: with 0.5 half the rows are core by construction.  The report's curve is that of k = min_samples - 1
        held within [1, 63] and below N - 1 (min_samples 1: the curve of k = 1).
    With model.world_size > 1 every rank gathers the rows (as evaluate_kmeans does) and computes the same report."""
    from . import evaluation as E
    who = "evaluate_dbscan"
    som = model.som_layer
    if metric is None:
        metric = som.distance_fcn if som.distance_fcn in ("cosine", "euclidean") else "euclidean"
    if metric not in METRICS:
        raise ValueError(f"{who}: metric must be one of {sorted(METRICS)}, got {metric!r}")
    start = time.time()
    X, y = _latents_and_labels(model, config, dataloader, who)
    k = int(min_samples) - 1
    if eps is None and k > MAX_K:
        raise ValueError(f"{who}: eps=None reads the curve of k = min_samples - 1 = {k}, and k_distances takes k <= {MAX_K}; pass eps")
    curve = k_distances(X, min(max(k, 1), MAX_K, X.shape[0] - 2), metric)
    if eps is None:
        eps = eps_from_k_distances(curve, eps_quantile)
    db = DBSCAN(eps=float(eps), min_samples=int(min_samples), metric=metric).fit(X)
    labels, dev, N = db.labels_, X.device, X.shape[0]
    wide = E._label_count(config, None, True)
    inside = labels >= 0
    sizes = np.zeros(0, dtype=np.int64)
    purity = nmi = float("nan")
    if db.n_clusters_:
        table = E._Table(db.n_clusters_, wide, dev)
        table.add(labels[inside], y[inside])
        w = table.numpy()
        sizes, purity, nmi = w.sum(axis=1).astype(np.int64), E.purity_from_table(w), E.nmi_from_table(w)
    noise = E._Table(1, wide, dev)
    if db.n_noise_:
        noise.add(torch.zeros_like(y[~inside]), y[~inside])
    per_class = noise.numpy()[0].astype(np.int64)
    classes = int(config["data"].get("num_classes", 0))
    seen = int(np.flatnonzero(per_class).max()) + 1 if per_class.any() else 0
    inference_time = time.time() - start
    report = DBSCANReport(eps=float(eps), min_samples=int(min_samples), metric=metric, n_clusters=db.n_clusters_, n_core=db.n_core_,
                          n_border=db.n_border_, n_noise=db.n_noise_, coverage=float(N - db.n_noise_) / N, cluster_sizes=sizes,
                          purity=purity, nmi=nmi, noise_per_class=per_class[:max(classes, seen)], k_distances=curve, labels=labels,
                          n_samples=N, inference_time=float(inference_time))
    print(f"DBSCAN ({metric}, eps {report.eps:.6g}, min_samples {report.min_samples}): {report.n_clusters} clusters, "
          f"{report.n_noise} noise rows of {N}, Purity (DBSCAN): {purity:.3f}, NMI (DBSCAN): {nmi:.3f}, "
          f"Inference Time: {inference_time:.3f}")
    return report


@torch.no_grad()
def visualize_dbscan(model, config, dataloader, eps=None, min_samples=5, metric=None, eps_quantile=0.5, epoch=0,
                     output_dir="experiments/plots/vit_som/dbscan", fit_rows=None):
    """visualize_umap_progression's scatter of the rows evaluate_dbscan clusters (same UMAP, same fit_rows), coloured by
    density cluster with the noise rows in grey -> output_dir/som_dbscan_epoch_{epoch}.png (rank 0 only; skipped with a
    warning when matplotlib is missing).  Returns (embedding [N, 2] float32, cluster labels [N] int64) as host arrays."""
    import os
    from . import evaluation as E
    who = "visualize_dbscan"
    report = evaluate_dbscan(model, config, dataloader, eps=eps, min_samples=min_samples, metric=metric, eps_quantile=eps_quantile)
    X, _ = _latents_and_labels(model, config, dataloader, who)
    embedding = E._umap_embed(X, fit_rows)[1].cpu().numpy()
    labels = report.labels.cpu().numpy()
    if E._rank(model) == 0:
        plt = E._pyplot(who)
        if plt is not None:
            os.makedirs(output_dir, exist_ok=True)
            plt.figure(figsize=(10, 8), dpi=300)
            plt.axis("off")
            out = labels < 0
            plt.scatter(embedding[out, 0], embedding[out, 1], c="0.7", s=3, alpha=0.5, edgecolor="none", rasterized=True)
            plt.scatter(embedding[~out, 0], embedding[~out, 1], c=labels[~out] % 10, cmap="tab10", vmin=0, vmax=9, s=3, alpha=0.7,
                        edgecolor="none", rasterized=True)
            plt.savefig(os.path.join(output_dir, f"som_dbscan_epoch_{epoch}.png"), **E._UMAP_SAVEFIG)
            plt.close()
    return embedding, labels
