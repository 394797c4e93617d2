"""sklearn.cluster.AgglomerativeClustering (sklearn/cluster/_agglomerative.py) on the device, and evaluate_map_clusters /
visualize_map_clusters, the second-level clustering of the SOM's units built on it (Vesanto and Alhoniemi, "Clustering of
the self-organizing map"; no counterpart in the reference).

The two parts that cost time are HIP kernels (csrc/agglomerative.hip): the [N, N] fp64 distance matrix in the DIRECT form,
and the merge loop -- the generic greedy algorithm with a nearest-neighbour array, all N - 1 steps enqueued by one call, the
least pair taken under the total order (distance, smaller slot, larger slot).  The host reads children_, distances_ and the
status words in ONE copy at the end and cuts the tree with an O(N) union-find; the labels go back to the device.  Two fits
on the same input are bitwise equal.

Departures from sklearn, all stated here and in INTEGRATION.md:
* Clusters are numbered by their smallest row index, ascending.  sklearn's numbering (an artefact of its heap walk) is NOT
  promised; partitions agree.
* With a connectivity, only adjacent clusters merge, and the distance between two clusters is the FULL linkage distance over
  all their members, adjacent or not (Murtagh's contiguity constraint).  sklearn's average, complete and single linkages
  take distances over connected pairs only and build other trees; Ward agrees with sklearn.
* A connectivity with more than one component raises ValueError naming the count (sklearn completes the graph and warns).
* distances_ is always computed (compute_distances is accepted and ignored: the loop has the heights anyway).
* metric is one of "euclidean", "l2", "manhattan", "l1", "cosine", "precomputed"; no callable.  N <= 16 384.
"""
import numbers
import time
from dataclasses import dataclass

import numpy as np
import torch

from . import ops

_METRICS = {"euclidean": ops.AGGLO_EUCLIDEAN, "l2": ops.AGGLO_EUCLIDEAN, "manhattan": ops.AGGLO_MANHATTAN,
            "l1": ops.AGGLO_MANHATTAN, "cosine": ops.AGGLO_COSINE, "precomputed": None}
_LINKAGES = {"ward": ops.AGGLO_WARD, "average": ops.AGGLO_AVERAGE, "complete": ops.AGGLO_COMPLETE, "single": ops.AGGLO_SINGLE}
ONE_OF = "Exactly one of n_clusters and distance_threshold has to be set, and the other needs to be None."
FULL_TREE = "compute_full_tree must be True if distance_threshold is set."
_NP_BOOL = f"{np.bool_.__module__}.{np.bool_.__qualname__}"      # as sklearn names the type: numpy.bool_ or, numpy 2, numpy.bool
ZERO_VECTORS = "Cosine affinity cannot be used when X contains zero vectors"


def _options(values):
    return "{" + ", ".join(repr(v) for v in values) + "}"


def cut_tree(children, n_leaves, n_clusters):
    """Labels int64 [n_leaves] (numpy) of the tree `children` ([n_leaves - 1, 2], scipy's numbering) cut at n_clusters: the
    first n_leaves - n_clusters merges applied by a union-find, the clusters numbered by their smallest row, ascending."""
    N = int(n_leaves)
    if n_clusters > N:
        raise ValueError("Cannot extract more clusters than samples: %s clusters where given for a tree with %s leaves."
                         % (n_clusters, N))
    parent = list(range(2 * N - 1))

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root
    rows = np.asarray(children).tolist()
    for s in range(N - int(n_clusters)):
        a, b = rows[s]
        parent[find(a)] = N + s
        parent[find(b)] = N + s
    number, labels = {}, np.empty(N, dtype=np.int64)
    for i in range(N):
        labels[i] = number.setdefault(find(i), len(number))
    return labels


class AgglomerativeClustering:
    """sklearn.cluster.AgglomerativeClustering for float32 [N, D] device tensors (a row stride is fine; metric
    "precomputed": a float32 or float64 [N, N] device tensor), N <= 16 384.  Names, defaults and error sentences are
    sklearn's.  fit / fit_predict.  Fitted: labels_ int64 [N] on the device; children_ int64 [N - 1, 2] and distances_
    float64 [N - 1] as numpy arrays in scipy's `linkage` convention (row s creates cluster N + s, the smaller id first;
    distances_ is always there); n_clusters_, n_leaves_, n_connected_components_, n_features_in_.

    NOT sklearn's: clusters are numbered by their smallest row index, ascending (sklearn's numbering is not promised); a
    connectivity restricts WHICH clusters merge, the linkage distance stays the full one over all members; a connectivity
    with more than one component raises ValueError.  connectivity: a symmetric bool or 0 / 1 [N, N] device tensor, a
    numpy array, or a scipy sparse matrix (densified on the way in)."""

    def __init__(self, n_clusters=2, *, metric="euclidean", connectivity=None, compute_full_tree="auto", linkage="ward",
                 distance_threshold=None, compute_distances=False):
        self.n_clusters, self.metric, self.connectivity, self.compute_full_tree = n_clusters, metric, connectivity, compute_full_tree
        self.linkage, self.distance_threshold, self.compute_distances = linkage, distance_threshold, compute_distances

    def _check_params(self):
        n = self.n_clusters
        if n is not None and (isinstance(n, bool) or not isinstance(n, numbers.Integral) or n < 1):
            raise ValueError(f"The 'n_clusters' parameter of AgglomerativeClustering must be an int in the range [1, inf) or None. "
                             f"Got {n!r} instead.")
        if not isinstance(self.metric, str) or self.metric not in _METRICS:
            raise ValueError(f"The 'metric' parameter of AgglomerativeClustering must be a str among {_options(sorted(_METRICS))}. "
                             f"Got {self.metric!r} instead.")
        if not (isinstance(self.compute_full_tree, (bool, np.bool_)) or
                (isinstance(self.compute_full_tree, str) and self.compute_full_tree == "auto")):
            raise ValueError(f"The 'compute_full_tree' parameter of AgglomerativeClustering must be a str among {{'auto'}} or an "
                             f"instance of 'bool' or an instance of '{_NP_BOOL}'. Got {self.compute_full_tree!r} instead.")
        if not isinstance(self.linkage, str) or self.linkage not in _LINKAGES:
            raise ValueError(f"The 'linkage' parameter of AgglomerativeClustering must be a str among {_options(_LINKAGES)}. "
                             f"Got {self.linkage!r} instead.")
        t = self.distance_threshold
        if t is not None and (isinstance(t, bool) or not isinstance(t, numbers.Real) or not t >= 0):
            raise ValueError(f"The 'distance_threshold' parameter of AgglomerativeClustering must be a float in the range "
                             f"[0.0, inf) or None. Got {t!r} instead.")
        if not isinstance(self.compute_distances, (bool, np.bool_)):
            raise ValueError(f"The 'compute_distances' parameter of AgglomerativeClustering must be an instance of 'bool' or an "
                             f"instance of '{_NP_BOOL}'. Got {self.compute_distances!r} instead.")

    def _check_rules(self):
        """The rules of sklearn's _fit, in its order."""
        if not ((self.n_clusters is None) ^ (self.distance_threshold is None)):
            raise ValueError(ONE_OF)
        if self.distance_threshold is not None and not self.compute_full_tree:
            raise ValueError(FULL_TREE)
        if self.linkage == "ward" and self.metric != "euclidean":
            raise ValueError(f"{self.metric} was provided as metric. Ward can only work with euclidean distances.")

    def _check_x(self, X):
        if not (isinstance(X, torch.Tensor) and X.is_cuda):
            raise ValueError("AgglomerativeClustering: X must be a tensor on the GPU")
        if X.dim() != 2:
            raise ValueError(f"Expected 2D array, got {X.dim()}D tensor instead.")
        N, D = X.shape
        if self.metric == "precomputed":
            if X.dtype not in (torch.float32, torch.float64):
                raise ValueError("AgglomerativeClustering: a precomputed X must be float32 or float64")
            if N != D:
                raise ValueError(f"Distance matrix should be square, got matrix of shape {(N, D)}. Check that you are passing a "
                                 f"distance matrix to fit, not the data matrix.")
        elif X.dtype != torch.float32:
            raise ValueError("AgglomerativeClustering: X must be a float32 [N, D] tensor on the GPU")
        if N < 2:
            raise ValueError(f"Found array with {N} sample(s) (shape=({N}, {D})) while a minimum of 2 is required by "
                             f"AgglomerativeClustering.")
        if D < 1:
            raise ValueError(f"Found array with {D} feature(s) (shape=({N}, {D})) while a minimum of 1 is required by "
                             f"AgglomerativeClustering.")
        if N > ops.AGGLO_MAX_N:
            raise ValueError(f"AgglomerativeClustering: {N} rows > {ops.AGGLO_MAX_N}, the most the kernels take (the fp64 distance "
                             f"matrix would pass 2 GiB)")
        if self.metric != "precomputed" and X.stride(1) != 1:
            X = X.contiguous()
        return X

    @staticmethod
    def _adjacency(connectivity, N, device):
        c = connectivity
        if hasattr(c, "toarray"):                                    # a scipy sparse matrix
            c = c.toarray()
        if not isinstance(c, torch.Tensor):
            c = torch.from_numpy(np.ascontiguousarray(np.asarray(c) != 0))
        if c.dim() != 2 or tuple(c.shape) != (N, N):
            raise ValueError(f"AgglomerativeClustering: connectivity must be [{N}, {N}], got {tuple(c.shape)}")
        c = (c.to(device) != 0)
        return (c | c.t()).to(torch.uint8)

    def fit(self, X, y=None):
        self._check_params()
        X = self._check_x(X)
        self._check_rules()
        N, dev = X.shape[0], X.device
        connected = self.connectivity is not None
        ws = torch.empty(ops.agglo_workspace_bytes(N, connected), dtype=torch.uint8, device=dev)
        M = ops.agglo_matrix(ws, N)
        # one buffer for everything the host reads: distances fp64 [N - 1], children int32 [N - 1, 2], status int32 [8]
        out = torch.zeros(16 * (N - 1) + 32, dtype=torch.uint8, device=dev)
        distances = out[:8 * (N - 1)].view(torch.float64)
        children = out[8 * (N - 1):16 * (N - 1)].view(torch.int32).view(N - 1, 2)
        status = out[16 * (N - 1):].view(torch.int32)
        if self.metric == "precomputed":
            M.copy_(X)
            status[4:5].copy_((~torch.isfinite(M)).sum().to(torch.int32).view(1))
        else:
            ops.agglo_distances(X, _METRICS[self.metric], self.linkage == "ward", M, status[4:6])
        if connected:
            ops.agglo_adjacency(ws, N).copy_(self._adjacency(self.connectivity, N, dev))
        ops.agglo_merge(ws, N, _LINKAGES[self.linkage], connected, children, distances, status[:ops.AGGLO_STATUS])
        host = out.cpu().numpy()                                     # THE host read of a fit
        st = host[16 * (N - 1):].view(np.int32)
        if st[4]:
            if self.metric != "precomputed" and bool(torch.isnan(X).any()):
                raise ValueError("Input X contains NaN.\nAgglomerativeClustering does not accept missing values encoded as NaN.")
            raise ValueError(f"Input X contains infinity or a value too large for dtype('{str(X.dtype)[6:]}').")
        if st[5]:
            raise ValueError(ZERO_VECTORS)
        self.n_connected_components_ = int(st[ops.AGGLO_MISSING]) + 1
        if self.n_connected_components_ > 1:
            raise ValueError(f"AgglomerativeClustering: the connectivity has {self.n_connected_components_} connected components; "
                             f"it must have one (sklearn would complete the graph; here the tree of a disconnected graph is "
                             f"refused)")
        self.children_ = host[8 * (N - 1):16 * (N - 1)].view(np.int32).reshape(N - 1, 2).astype(np.int64)
        self.distances_ = host[:8 * (N - 1)].view(np.float64).copy()
        self.rescans_ = (int(st[ops.AGGLO_RESCANNED]), int(st[ops.AGGLO_RESCAN_STEPS]))   # slots searched again, steps with one
        self.n_leaves_ = N
        self.n_features_in_ = int(X.shape[1])
        if self.distance_threshold is not None:
            self.n_clusters_ = int(np.count_nonzero(self.distances_ >= self.distance_threshold)) + 1
        else:
            self.n_clusters_ = int(self.n_clusters)
        self.labels_ = torch.from_numpy(cut_tree(self.children_, N, self.n_clusters_)).to(dev)
        return self

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_


# ------------------------------------------------------------------------------------ the map's clusters
@dataclass
class MapClustersReport:
    """Host values of one evaluate_map_clusters pass (unit_labels and sample_labels stay on the device)."""
    purity: float
    nmi: float
    n_clusters: int
    metric: str
    linkage: str
    connectivity: str                    # "grid" or None
    unit_labels: torch.Tensor            # int64 [K] on the device: the cluster of every unit
    sample_labels: torch.Tensor          # int64 [this rank's samples], loader order: unit_labels[bmu]
    children: np.ndarray                 # int64 [K - 1, 2], scipy's numbering
    distances: np.ndarray                # float64 [K - 1]
    units_per_cluster: np.ndarray        # int64 [n_clusters]
    samples_per_cluster: np.ndarray      # int64 [n_clusters], over all ranks
    n_samples: int
    inference_time: float


def cluster_map_units(som, n_clusters, linkage=None, connectivity="grid", metric=None):
    """The fitted AgglomerativeClustering of a SOMLayer's prototypes and the (metric, linkage) it ran with.  metric None:
    the layer's distance_fcn; linkage None: "ward" for euclidean and cosine maps, "average" for manhattan maps.  Ward on a
    cosine map is Ward on the prototypes scaled to unit length, where d^2 = 2 (1 - cos)."""
    metric = som.distance_fcn if metric is None else metric
    if metric not in ("euclidean", "cosine", "manhattan"):
        raise ValueError(f"evaluate_map_clusters: metric must be 'euclidean', 'cosine' or 'manhattan', got {metric!r}")
    linkage = ("average" if metric == "manhattan" else "ward") if linkage is None else linkage
    if connectivity not in ("grid", None):
        raise ValueError(f"evaluate_map_clusters: connectivity must be 'grid' or None, got {connectivity!r}")
    rows = som.prototypes.detach().float().contiguous()
    fit_metric = metric
    if metric == "cosine" and linkage == "ward":
        rows, fit_metric = torch.nn.functional.normalize(rows, p=2, dim=1), "euclidean"
    ac = AgglomerativeClustering(n_clusters=int(n_clusters), metric=fit_metric, linkage=linkage,
                                 connectivity=som.grid_connectivity() if connectivity == "grid" else None)
    return ac.fit(rows), metric, linkage


@torch.no_grad()
def evaluate_map_clusters(model, config, dataloader, n_clusters=None, linkage=None, connectivity="grid", metric=None, num_labels=None):
    """The second-level clustering of the SOM -> MapClustersReport: the prototypes are merged hierarchically
    (cluster_map_units; connectivity="grid": only between units that touch on the grid, so every cluster is a connected
    region of the map; None: freely), the tree is cut at n_clusters (None: data.num_classes) and every sample takes the
    cluster of its BMU.  purity and nmi are those of the samples so labelled against the loader's labels, through the same
    table and rank sum as evaluate_clustering: they can be set against evaluate_kmeans and evaluate_gmm at the same k,
    which the per-unit figures of evaluate_clustering cannot.  No host synchronisation inside the loader loop.  The map is
    replicated, so with model.world_size > 1 every rank clusters it identically."""
    from . import evaluation as E                         # its loader pass and model adapter; evaluation imports this module
    arch = E._Arch(model, config, "evaluate_map_clusters").require()
    som = model.som_layer
    labels_wide = E._label_count(config, num_labels, True)
    k = int(config["data"].get("num_classes", 0)) if n_clusters is None else int(n_clusters)
    training = model.training
    start = time.time()
    if k < 1:                                             # a clustering config: the distinct labels, as evaluate_kmeans counts them
        hist = E._Table(1, labels_wide, arch.device)
        try:
            for _, y in arch.batches(dataloader, arch.images):
                hist.add(torch.zeros_like(y), y)
        finally:
            model.train(training)
        k = int((hist.numpy(E._world(model)) > 0).sum())
    ac, metric, linkage = cluster_map_units(som, k, linkage, connectivity, metric)
    unit_labels = ac.labels_
    table = E._Table(k, labels_wide, arch.device)
    seen = []
    try:
        for x, y in arch.batches(dataloader, arch.images):
            bmu, _ = model.predict(x)
            lab = unit_labels[bmu.reshape(-1).long()]
            table.add(lab, y)
            seen.append(lab)
    finally:
        model.train(training)
    w = table.numpy(E._world(model))
    inference_time = time.time() - start
    report = MapClustersReport(
        purity=E.purity_from_table(w), nmi=E.nmi_from_table(w), n_clusters=k, metric=metric, linkage=linkage,
        connectivity=connectivity, unit_labels=unit_labels,
        sample_labels=torch.cat(seen) if seen else torch.empty(0, dtype=torch.int64, device=arch.device),
        children=ac.children_, distances=ac.distances_,
        units_per_cluster=np.bincount(unit_labels.cpu().numpy(), minlength=k).astype(np.int64),
        samples_per_cluster=w.sum(axis=1).astype(np.int64), n_samples=int(w.sum()), inference_time=float(inference_time))
    print(f"Purity (map clusters, {k} of {linkage}/{metric}): {report.purity:.3f}, NMI (map clusters): {report.nmi:.3f}, "
          f"Inference Time: {inference_time:.3f}")
    return report


def visualize_map_clusters(model, config, n_clusters=None, linkage=None, connectivity="grid", metric=None,
                           output_dir="experiments/plots"):
    """The map's clusters as regions of the grid -> {output_dir}/{model_arch}_epoch_{epoch}_map_clusters.png (rank 0;
    skipped with a warning when matplotlib is missing), to put next to the U-matrix and the label heat map.  Needs no data.
    Returns the cluster of every unit, int64 [rows, cols]."""
    from . import evaluation as E
    som = model.som_layer
    k = int(config["data"].get("num_classes", 0)) if n_clusters is None else int(n_clusters)
    ac, _, _ = cluster_map_units(som, k, linkage, connectivity, metric)
    rows, cols = som.map_size
    regions = ac.labels_.cpu().numpy().reshape(rows, cols)
    E._save_cell_map(model, config, output_dir, "visualize_map_clusters", "map_clusters", "map clusters", regions, "cluster",
                     annotate=True)
    return regions
