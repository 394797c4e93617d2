"""sklearn.cluster.HDBSCAN (sklearn/cluster/_hdbscan; Campello, Moulavi and Sander 2013) on the device: density clusters
over all radii at once, chosen by their stability, noise first class, no eps.  With it evaluate_hdbscan and
visualize_hdbscan for the latents the SOM layer sees.  No counterpart in the reference.

The expensive part is the minimum spanning tree of the mutual-reachability graph d_mr(i, j) = max(core_i, core_j, d(i, j)),
core_i the distance of row i to its min_samples-th nearest row, the row itself counted (sklearn's rule): column
min_samples - 1 of ops.umap_knn's list.  The graph is never held.  Boruvka rounds (csrc/knn.hip, HDBSCAN section): one
round re-runs the all-pairs contraction of the neighbour search on the f32 matrix cores and keeps, per row, the least edge
that leaves the row's component (`vsom_hdbscan_nearest`); `vsom_hdbscan_merge` takes every component's least edge, hooks
the components and relabels.  The host reads one int32 [4] record per round and stops at one component: at most
ceil(log2 N) rounds.  Everything after the tree -- the single-linkage tree, the condensed tree, the stabilities, the
selection, labels and probabilities -- is numpy on the host, from the N - 1 edges read once.

The order.  Undirected edges are ordered by (w, min(i, j), max(i, j)), w the fp32 mutual-reachability distance.  The order
is strict, so the tree is unique and two fits are bitwise equal.  Mutual reachability is full of exact ties -- every edge
from a row to a neighbour nearer than its core distance has the same weight -- and the hierarchy is the one this order
fixes.  On tied or near-tied data a point between two clusters may land on the other side than in sklearn, whose result
depends on its own traversal order: a property of the method, not of the port.

Departures from sklearn, all stated here and in INTEGRATION.md:
* Distances are fp32 (the distance of vsom_umap_knn); metric "precomputed" takes float32 or float64 and rounds
  max(core_i, core_j, M[i, j]) to float32.
* metric is one of "euclidean", "l2", "cosine", "precomputed"; no callable.  metric_params must be None or empty.
* min_samples <= 64 (the neighbour lists hold at most 64 rows) and min_samples < N.
* alpha must be 1.0, max_cluster_size None, store_centers None: not built.
* algorithm, leaf_size, n_jobs and copy are validated as sklearn validates them and then ignored: the search is exact.
* N <= 131 072.  A row with a NaN, an infinity or an overflowing norm raises ValueError (sklearn labels it -2 / -3).
* Clusters are numbered by their smallest row, as AgglomerativeClustering here; sklearn numbers by tree node.
"""
import math
import numbers
import time
from dataclasses import dataclass

import numpy as np
import torch

from . import ops
from .dbscan import SKLEARN_METRICS, _latents_and_labels, _options
from .umap import METRICS

MAX_SAMPLES = ops.HDBSCAN_MAX_N
MAX_MIN_SAMPLES = 64                     # ops.umap_knn lists at most 64 rows, the row itself among them
_METRICS = {"euclidean": ops.DIST_EUCLIDEAN, "l2": ops.DIST_EUCLIDEAN, "cosine": ops.DIST_COSINE, "precomputed": None}
_ALGORITHMS = ("auto", "ball_tree", "brute", "kd_tree")
_METHODS = ("eom", "leaf")
_CENTERS = ("both", "centroid", "medoid")
# sklearn 1.7.2's names for HDBSCAN's metric: DBSCAN's and the fast trees' (its message prints them as a set)
HDBSCAN_METRICS = tuple(sorted(set(SKLEARN_METRICS) | {"infinity", "p", "pyfunc"}))
_BOOLEAN = f"an instance of 'bool' or an instance of '{np.bool_.__module__}.{np.bool_.__name__}'"      # sklearn prints numpy's own name
CONDENSED_DTYPE = np.dtype([("parent", np.intp), ("child", np.intp), ("value", np.float64), ("cluster_size", np.intp)])


# ------------------------------------------------------------------------------------ the tree, on the host
def sort_edges(lo, hi, w):
    """The edges in the total order (w, lo, hi) -> (lo, hi, w), lo < hi."""
    lo, hi, w = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64), np.asarray(w, dtype=np.float64)
    lo, hi = np.minimum(lo, hi), np.maximum(lo, hi)
    order = np.lexsort((hi, lo, w))
    return lo[order], hi[order], w[order]


def single_linkage(lo, hi, w):
    """The single-linkage tree of N - 1 tree edges sorted by sort_edges, in scipy's `linkage` convention: float64 [N - 1, 4],
    row k = (left, right, w, size) forms node N + k.  One union-find pass over the edges (path halving)."""
    n = len(w) + 1
    parent = list(range(2 * n - 1))
    size = [1] * n + [0] * (n - 1)
    Z = np.empty((n - 1, 4), dtype=np.float64)
    for k, (a, b) in enumerate(zip(lo.tolist(), hi.tolist())):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        while parent[b] != b:
            parent[b] = parent[parent[b]]
            b = parent[b]
        if a == b:
            raise ValueError("single_linkage: the edges close a cycle")
        node = n + k
        parent[a] = parent[b] = node
        size[node] = size[a] + size[b]
        Z[k, 0], Z[k, 1], Z[k, 3] = a, b, size[node]
    Z[:, 2] = w
    return Z


def leaf_layout(Z):
    """The leaves in tree order, laid out once -> (order int64 [N], start int64 [2 N - 1]): the leaves of node v are
    order[start[v] : start[v] + size(v)].  Top down over the rows of Z, no recursion."""
    n = Z.shape[0] + 1
    left, right = Z[:, 0].astype(np.int64), Z[:, 1].astype(np.int64)
    sizes = np.concatenate([np.ones(n, dtype=np.int64), Z[:, 3].astype(np.int64)])
    start = [0] * (2 * n - 1)
    sz = sizes.tolist()
    for k in range(n - 2, -1, -1):
        a, b, s = int(left[k]), int(right[k]), start[n + k]
        start[a] = s
        start[b] = s + sz[a]
    start = np.asarray(start, dtype=np.int64)
    order = np.empty(n, dtype=np.int64)
    order[start[:n]] = np.arange(n)
    return order, start


def condense_tree(Z, min_cluster_size):
    """sklearn's condensed tree (runt pruning at min_cluster_size) of a single-linkage tree -> structured array
    (parent, child, value = lambda = 1 / distance, cluster_size); samples are 0 .. N - 1, the root cluster is N and a
    child cluster's number is larger than its parent's.  A subtree that falls out of a cluster contributes its leaves
    as one slice of leaf_layout's order."""
    n = Z.shape[0] + 1
    order, start = leaf_layout(Z)
    left, right = Z[:, 0].astype(np.int64).tolist(), Z[:, 1].astype(np.int64).tolist()
    dist = Z[:, 2].tolist()
    sizes = [1] * n + Z[:, 3].astype(np.int64).tolist()
    begin = start.tolist()
    label = [-1] * (2 * n - 1)                   # the cluster a node carries; -1 inside a subtree that fell out
    label[2 * n - 2] = n
    next_label = n + 1
    c_parent, c_child, c_value, c_size = [], [], [], []       # rows whose child is a cluster
    f_parent, f_begin, f_size, f_value = [], [], [], []       # slices of leaves that fall out of a cluster
    for k in range(n - 2, -1, -1):
        c = label[n + k]
        if c < 0:
            continue
        a, b = left[k], right[k]
        lam = 1.0 / dist[k] if dist[k] > 0.0 else math.inf
        big_a, big_b = sizes[a] >= min_cluster_size, sizes[b] >= min_cluster_size
        if big_a and big_b:
            for child in (a, b):
                label[child] = next_label
                c_parent.append(c); c_child.append(next_label); c_value.append(lam); c_size.append(sizes[child])
                next_label += 1
            continue
        for child, big in ((a, big_a), (b, big_b)):
            if big:
                label[child] = c
            else:
                f_parent.append(c); f_begin.append(begin[child]); f_size.append(sizes[child]); f_value.append(lam)
    f_size = np.asarray(f_size, dtype=np.int64)
    total = int(f_size.sum())
    tree = np.empty(len(c_parent) + total, dtype=CONDENSED_DTYPE)
    m = len(c_parent)
    tree["parent"][:m], tree["child"][:m], tree["value"][:m], tree["cluster_size"][:m] = c_parent, c_child, c_value, c_size
    if total:
        ends = np.cumsum(f_size)
        within = np.arange(total) - np.repeat(ends - f_size, f_size)
        tree["parent"][m:] = np.repeat(np.asarray(f_parent, dtype=np.int64), f_size)
        tree["child"][m:] = order[np.repeat(np.asarray(f_begin, dtype=np.int64), f_size) + within]
        tree["value"][m:] = np.repeat(np.asarray(f_value, dtype=np.float64), f_size)
        tree["cluster_size"][m:] = 1
    return tree


def _cluster_tables(tree, n):
    """Per cluster id - n (the root is 0): parent cluster, birth lambda, size, stability, the largest lambda among its rows."""
    count = int(tree["parent"].max()) - n + 1 if len(tree) else 1
    rows = tree[tree["cluster_size"] > 1]
    parent = np.full(count, -1, dtype=np.int64)
    birth = np.zeros(count)
    size = np.zeros(count, dtype=np.int64)
    parent[rows["child"] - n], birth[rows["child"] - n], size[rows["child"] - n] = rows["parent"] - n, rows["value"], rows["cluster_size"]
    size[0] = n
    p = tree["parent"] - n
    with np.errstate(invalid="ignore"):
        stability = np.bincount(p, weights=(tree["value"] - birth[p]) * tree["cluster_size"], minlength=count)
    death = np.zeros(count)
    np.maximum.at(death, p, tree["value"])
    return parent, birth, size, stability, death


def select_clusters(tree, n, method="eom", allow_single_cluster=False, epsilon=0.0):
    """sklearn's _get_clusters up to the labels: which clusters of the condensed tree are chosen -> (selected bool
    [clusters], the tables of _cluster_tables).  Excess of mass bottom up over the cluster numbers (a child's is larger
    than its parent's), or the leaves; then cluster_selection_epsilon's walk towards the root."""
    parent, birth, size, stability, death = _cluster_tables(tree, n)
    count = len(parent)
    children = [[] for _ in range(count)]
    for c in range(1, count):
        children[parent[c]].append(c)
    first = 0 if allow_single_cluster else 1
    selected = np.zeros(count, dtype=bool)
    if method == "eom":
        stab = stability.copy()
        kept = np.zeros(count, dtype=bool)
        for c in range(count - 1, first - 1, -1):
            below = float(np.sum([stab[k] for k in children[c]])) if children[c] else 0.0
            if below > stab[c]:
                stab[c] = below
            else:
                kept[c] = True
        under = np.zeros(count, dtype=bool)          # below a kept cluster: sklearn clears those
        for c in range(1, count):
            under[c] = under[parent[c]] or kept[parent[c]]
        selected = kept & ~under
        if epsilon != 0.0 and count > 1:
            chosen = np.flatnonzero(selected).tolist()
            if chosen == [0]:
                selected[:] = False
                selected[0] = bool(allow_single_cluster)
            else:
                selected = _epsilon_search(chosen, parent, birth, children, epsilon, allow_single_cluster, count)
    else:
        leaves = [c for c in range(1, count) if not children[c]] if count > 1 else []
        if epsilon != 0.0 and leaves:
            selected = _epsilon_search(leaves, parent, birth, children, epsilon, allow_single_cluster, count)
        else:
            selected[leaves] = True
    return selected, (parent, birth, size, stability, death)


def _epsilon_search(candidates, parent, birth, children, epsilon, allow_single_cluster, count):
    """sklearn's epsilon_search: a candidate born at a distance below epsilon is replaced by its first ancestor born at a
    distance above it (the child of the root at the latest, the root itself with allow_single_cluster)."""
    selected = np.zeros(count, dtype=bool)
    done = set()
    for leaf in candidates:
        if 1.0 / birth[leaf] >= epsilon:
            selected[leaf] = True
            continue
        if leaf in done:
            continue
        node = leaf
        while True:
            up = parent[node]
            if up == 0:
                node = 0 if allow_single_cluster else node
                break
            node = up
            if 1.0 / birth[node] > epsilon:
                break
        selected[node] = True
        stack = list(children[node])
        while stack:
            c = stack.pop()
            done.add(c)
            stack.extend(children[c])
    return selected


def label_points(tree, n, selected, tables, allow_single_cluster=False, epsilon=0.0):
    """sklearn's _do_labelling and get_probabilities -> (labels int64 [n] numbered by the clusters' smallest row, -1 noise;
    probabilities float64 [n]; the chosen clusters' numbers in label order)."""
    parent, _, _, _, death = tables
    count = len(parent)
    top = np.full(count, -1, dtype=np.int64)         # the nearest chosen cluster at or above
    for c in range(count):
        top[c] = c if selected[c] else (top[parent[c]] if c else -1)
    points = tree[tree["cluster_size"] == 1]
    labels = np.full(n, -1, dtype=np.int64)
    prob = np.zeros(n)
    if not len(points):
        return labels, prob, np.zeros(0, dtype=np.int64)
    rows, lam = points["child"], points["value"]
    cluster = top[points["parent"] - n]
    inside = cluster >= 0
    if selected[0]:                                  # the root alone: a point stays only above the threshold
        if int(selected.sum()) == 1 and allow_single_cluster:
            threshold = 1.0 / epsilon if epsilon != 0.0 else float(tree["value"][tree["parent"] == n].max())
            inside &= (cluster != 0) | (lam >= threshold)
        else:
            inside &= cluster != 0
    chosen = np.flatnonzero(selected)
    smallest = np.full(count, n, dtype=np.int64)
    np.minimum.at(smallest, cluster[inside], rows[inside])
    chosen = chosen[np.argsort(smallest[chosen], kind="stable")]
    chosen = chosen[smallest[chosen] < n]
    number = np.full(count, -1, dtype=np.int64)
    number[chosen] = np.arange(len(chosen))
    labels[rows[inside]] = number[cluster[inside]]
    top_lambda = death[cluster[inside]]
    with np.errstate(invalid="ignore", divide="ignore"):
        p = np.where((top_lambda == 0.0) | np.isinf(lam[inside]), 1.0, np.minimum(lam[inside], top_lambda) / top_lambda)
    prob[rows[inside]] = p
    return labels, prob, chosen + n


def labels_at_cut(lo, hi, w, n, cut, min_cluster_size):
    """sklearn's labelling_at_cut on the sorted tree edges: the components of the edges with w < cut; those of at least
    min_cluster_size rows are clusters, numbered by their smallest row, the other rows noise."""
    parent = list(range(n))
    for a, b, d in zip(lo.tolist(), hi.tolist(), w.tolist()):
        if not d < cut:
            break
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        while parent[b] != b:
            parent[b] = parent[parent[b]]
            b = parent[b]
        parent[max(a, b)] = min(a, b)
    root = np.asarray(parent, dtype=np.int64)
    for _ in range(n):                               # roots are minima: every pass at least halves the depth
        up = root[root]
        if np.array_equal(up, root):
            break
        root = up
    sizes = np.bincount(root, minlength=n)
    keep = sizes[root] >= min_cluster_size
    number = np.full(n, -1, dtype=np.int64)
    roots = np.unique(root[keep])                    # a root is its component's smallest row
    number[roots] = np.arange(len(roots))
    return np.where(keep, number[root], -1)


def linkage_to_labels(Z, min_cluster_size=5, method="eom", allow_single_cluster=False, epsilon=0.0):
    """Everything after the single-linkage tree Z (scipy's convention, merges in ascending distance) -> dict(condensed_tree,
    labels, probabilities, clusters, persistence)."""
    n = Z.shape[0] + 1
    tree = condense_tree(Z, int(min_cluster_size))
    selected, tables = select_clusters(tree, n, method, bool(allow_single_cluster), float(epsilon))
    labels, prob, clusters = label_points(tree, n, selected, tables, bool(allow_single_cluster), float(epsilon))
    return dict(single_linkage_tree=Z, condensed_tree=tree, labels=labels, probabilities=prob, clusters=clusters,
                persistence=tables[3][clusters - n])


def tree_to_labels(lo, hi, w, n, min_cluster_size=5, method="eom", allow_single_cluster=False, epsilon=0.0):
    """Everything after the spanning tree -> linkage_to_labels' dict and edges = (lo, hi, w) in the order (w, lo, hi): the
    host side of HDBSCAN.fit, also what the tests feed sklearn's own distances."""
    lo, hi, w = sort_edges(lo, hi, w)
    if len(w) != n - 1:
        raise ValueError(f"tree_to_labels: {len(w)} edges for {n} rows")
    out = linkage_to_labels(single_linkage(lo, hi, w), min_cluster_size, method, allow_single_cluster, epsilon)
    out["edges"] = (lo, hi, w)
    return out


# ------------------------------------------------------------------------------------ the estimator
def round_limit(N):
    """The rounds a spanning tree of N rows may take: every Boruvka round at least halves the components, so
    ceil(log2 N) suffice; one more is allowed before the fit gives up."""
    return max(1, math.ceil(math.log2(N))) + 1


def spanning_tree(X, core, metric):
    """The minimum spanning tree of max(core_i, core_j, d(i, j)) under (w, lo, hi) by Boruvka rounds on the device ->
    (edges int32 [N - 1, 3] on the host: lo, hi and the fp32 bits of w, in no particular order; the rounds taken).
    X float32 [N, D] with metric DIST_EUCLIDEAN / DIST_COSINE, or with metric None a float32 / float64 [N, N] matrix of
    distances; core float32 [N].  One host read per round; ValueError for rows (entries) that are not finite,
    RuntimeError when round_limit(N) rounds leave more than one component."""
    N, dev = X.shape[0], X.device
    new = lambda dtype, *shape: torch.empty(*shape, dtype=dtype, device=dev)      # noqa: E731
    comp, edges, record = new(torch.int32, N), new(torch.int32, N, 3), new(torch.int32, 4)
    best, work, sq = new(torch.int64, N), new(torch.int64, ops.hdbscan_work(N)), new(torch.float32, N)
    ops.hdbscan_init(comp, edges, record)
    left = N
    for rounds in range(1, round_limit(N) + 1):
        if metric is None:
            ops.hdbscan_nearest_matrix(X, core, comp, best, record)
        else:
            ops.hdbscan_nearest(X, metric, core, comp, sq, best, record)
        ops.hdbscan_merge(best, comp, edges, work, record)
        left, _, bad, _ = record.tolist()                            # THE host read of a round
        if bad:
            if metric is None:
                raise ValueError(f"HDBSCAN: the precomputed matrix is not finite: {bad} of its entries are NaN or infinite")
            raise ValueError(f"HDBSCAN: {bad} rows of X are not finite: they hold NaN or infinity, or their squared norm "
                             f"overflows float32")
        if left == 1:
            break
    else:
        raise RuntimeError(f"HDBSCAN: the spanning tree is not complete after {rounds} rounds ({left} components left)")
    e = edges.cpu().numpy()
    e = e[e[:, 0] >= 0]
    if e.shape[0] != N - 1:
        raise RuntimeError(f"HDBSCAN: {e.shape[0]} edges for {N} rows")
    return e, rounds


class HDBSCAN:
    """sklearn.cluster.HDBSCAN for float32 [N, D] device tensors (a row stride is fine; metric "precomputed": a float32 or
    float64 [N, N] device tensor of distances, symmetric), 2 <= N <= 131 072.  Names, defaults and parameter error sentences
    are sklearn 1.7.2's.  fit / fit_predict / dbscan_clustering(cut_distance, min_cluster_size=5).  Fitted: labels_ int64 [N]
    on the device, -1 for noise; probabilities_ float32 [N] on the device; n_features_in_.

    NOT in sklearn: core_distances_ (float32 [N], device), minimum_spanning_tree_ (float64 [N - 1, 3] host: lo, hi, w in the
    order (w, lo, hi)), single_linkage_tree_ (host, scipy's convention), condensed_tree_ (host structured array: parent,
    child, value, cluster_size), cluster_persistence_ (the chosen clusters' stabilities), n_clusters_, n_noise_, n_rounds_.

    Departures: distances are fp32 and the tree is the one the strict order (w, min(i, j), max(i, j)) fixes -- mutual
    reachability is full of exact ties, and on tied or near-tied data a point between two clusters may land on the other
    side than in sklearn, whose result depends on its traversal order; clusters are numbered by their smallest row;
    metric "euclidean" / "l2" / "cosine" / "precomputed" only (precomputed: w is the float32 rounding of
    max(core_i, core_j, M[i, j])); min_samples <= 64 and < N; alpha 1.0, max_cluster_size None and store_centers None only;
    algorithm, leaf_size, n_jobs and copy are validated and ignored; rows that are not finite raise ValueError."""

    def __init__(self, min_cluster_size=5, min_samples=None, cluster_selection_epsilon=0.0, max_cluster_size=None, metric="euclidean",
                 metric_params=None, alpha=1.0, algorithm="auto", leaf_size=40, n_jobs=None, cluster_selection_method="eom",
                 allow_single_cluster=False, store_centers=None, copy=False):
        self.min_cluster_size, self.min_samples, self.cluster_selection_epsilon = min_cluster_size, min_samples, cluster_selection_epsilon
        self.max_cluster_size, self.metric, self.metric_params, self.alpha = max_cluster_size, metric, metric_params, alpha
        self.algorithm, self.leaf_size, self.n_jobs = algorithm, leaf_size, n_jobs
        self.cluster_selection_method, self.allow_single_cluster = cluster_selection_method, allow_single_cluster
        self.store_centers, self.copy = store_centers, copy

    def _check_params(self):
        def integral(v):
            return isinstance(v, numbers.Integral) and not isinstance(v, bool)

        def real(v):
            return isinstance(v, numbers.Real) and not isinstance(v, bool)

        def boolean(v):
            return isinstance(v, (bool, np.bool_))
        who = "HDBSCAN"
        v = self.min_cluster_size
        if not integral(v) or v < 2:
            raise ValueError(f"The 'min_cluster_size' parameter of {who} must be an int in the range [2, inf). Got {v!r} instead.")
        v = self.min_samples
        if v is not None and (not integral(v) or v < 1):
            raise ValueError(f"The 'min_samples' parameter of {who} must be an int in the range [1, inf) or None. Got {v!r} instead.")
        v = self.cluster_selection_epsilon
        if not real(v) or not v >= 0:
            raise ValueError(f"The 'cluster_selection_epsilon' parameter of {who} must be a float in the range [0.0, inf). "
                             f"Got {v!r} instead.")
        v = self.max_cluster_size
        if v is not None and (not integral(v) or v < 1):
            raise ValueError(f"The 'max_cluster_size' parameter of {who} must be None or an int in the range [1, inf). "
                             f"Got {v!r} instead.")
        if callable(self.metric):                                    # a departure: sklearn takes one
            raise ValueError("HDBSCAN: a callable metric is not supported: the distances come from one contraction on the matrix "
                             "cores; pass the callable's distance matrix with metric='precomputed'")
        if not (isinstance(self.metric, str) and self.metric in HDBSCAN_METRICS):
            raise ValueError(f"The 'metric' parameter of {who} must be a str among {_options(HDBSCAN_METRICS)} or a callable. "
                             f"Got {self.metric!r} instead.")
        v = self.metric_params
        if v is not None and not isinstance(v, dict):
            raise ValueError(f"The 'metric_params' parameter of {who} must be an instance of 'dict' or None. Got {v!r} instead.")
        v = self.alpha
        if not real(v) or not 0 < v < math.inf:
            raise ValueError(f"The 'alpha' parameter of {who} must be a float in the range (0.0, inf). Got {v!r} instead.")
        v = self.algorithm
        if not (isinstance(v, str) and v in _ALGORITHMS):
            raise ValueError(f"The 'algorithm' parameter of {who} must be a str among {_options(_ALGORITHMS)}. Got {v!r} instead.")
        v = self.leaf_size
        if not integral(v) or v < 1:
            raise ValueError(f"The 'leaf_size' parameter of {who} must be an int in the range [1, inf). Got {v!r} instead.")
        v = self.n_jobs
        if v is not None and not isinstance(v, numbers.Integral):
            raise ValueError(f"The 'n_jobs' parameter of {who} must be an instance of 'int' or None. Got {v!r} instead.")
        v = self.cluster_selection_method
        if not (isinstance(v, str) and v in _METHODS):
            raise ValueError(f"The 'cluster_selection_method' parameter of {who} must be a str among {_options(_METHODS)}. "
                             f"Got {v!r} instead.")
        v = self.allow_single_cluster
        if not boolean(v):
            raise ValueError(f"The 'allow_single_cluster' parameter of {who} must be {_BOOLEAN}. Got {v!r} instead.")
        v = self.store_centers
        if v is not None and not (isinstance(v, str) and v in _CENTERS):
            raise ValueError(f"The 'store_centers' parameter of {who} must be None or a str among {_options(_CENTERS)}. "
                             f"Got {v!r} instead.")
        v = self.copy
        if not boolean(v):
            raise ValueError(f"The 'copy' parameter of {who} must be {_BOOLEAN}. Got {v!r} instead.")
        # the departures: what sklearn takes and this class does not
        if self.metric not in _METRICS:
            raise ValueError(f"HDBSCAN: metric {self.metric!r} is not supported: the contraction computes {sorted(_METRICS)[:3]}; "
                             f"for any other metric pass its distance matrix with metric='precomputed' (ops.agglo_distances "
                             f"has manhattan)")
        if self.metric_params:
            raise ValueError(f"HDBSCAN: metric_params {self.metric_params!r} is not supported: none of the metrics takes a parameter")
        if self.min_samples is not None and self.min_samples > MAX_MIN_SAMPLES:
            raise ValueError(f"HDBSCAN: min_samples {self.min_samples} > {MAX_MIN_SAMPLES} is not supported: the core distance is "
                             f"read from the neighbour search's list, which holds at most {MAX_MIN_SAMPLES} rows")
        if float(self.alpha) != 1.0:
            raise ValueError(f"HDBSCAN: alpha {self.alpha!r} is not supported: the distances are not rescaled (robust single linkage "
                             f"is not built); only 1.0")
        if self.max_cluster_size is not None:
            raise ValueError("HDBSCAN: max_cluster_size is not supported: the excess-of-mass selection has no size limit; only None")
        if self.store_centers is not None:
            raise ValueError("HDBSCAN: store_centers is not supported: centroids and medoids are not computed; only None")

    def _check_x(self, X):
        if not (isinstance(X, torch.Tensor) and X.is_cuda):
            raise ValueError("HDBSCAN: X must be a tensor on the GPU")
        if X.dim() != 2:
            raise ValueError(f"Expected 2D array, got {X.dim()}D tensor instead.")
        N, D = X.shape
        if self.metric == "precomputed":
            if X.dtype not in (torch.float32, torch.float64):
                raise ValueError("HDBSCAN: a precomputed X must be float32 or float64")
            if N != D:
                raise ValueError(f"Precomputed matrix must be square. Input is a {N}x{D} matrix.")
        elif X.dtype != torch.float32:
            raise ValueError("HDBSCAN: X must be a float32 [N, D] tensor on the GPU")
        if N < 1:
            raise ValueError(f"Found array with {N} sample(s) (shape=({N}, {D})) while a minimum of 1 is required by HDBSCAN.")
        if D < 1:
            raise ValueError(f"Found array with {D} feature(s) (shape=({N}, {D})) while a minimum of 1 is required by HDBSCAN.")
        if N == 1:
            raise ValueError("n_samples=1 while HDBSCAN requires more than one sample")
        if N > MAX_SAMPLES:
            raise ValueError(f"HDBSCAN: {N} rows > {MAX_SAMPLES}, the most the kernels take")
        if X.stride(1) != 1 or (X.dtype == torch.float64 and not X.is_contiguous()):
            X = X.contiguous()
        return X

    def fit(self, X, y=None):
        self._check_params()
        X = self._check_x(X)
        N, dev = X.shape[0], X.device
        k = int(self.min_cluster_size if self.min_samples is None else self.min_samples)
        if k > N:
            raise ValueError(f"min_samples ({k}) must be at most the number of samples in X ({N})")
        if k > MAX_MIN_SAMPLES:
            raise ValueError(f"HDBSCAN: min_samples {k} (from min_cluster_size) > {MAX_MIN_SAMPLES} is not supported: the core "
                             f"distance is read from the neighbour search's list, which holds at most {MAX_MIN_SAMPLES} rows")
        if k == N:
            raise ValueError(f"HDBSCAN: min_samples {k} = the number of rows is not supported: the neighbour search lists fewer "
                             f"rows than the set has")
        new = lambda dtype, *shape: torch.empty(*shape, dtype=dtype, device=dev)      # noqa: E731
        pre = self.metric == "precomputed"
        if pre:
            if bool((X < 0).any()):
                raise ValueError("Negative values in data passed to X.")
            core = torch.kthvalue(X, k, dim=1).values.to(torch.float32).contiguous()
        else:
            idx, dist = new(torch.int64, N, k), new(torch.float32, N, k)
            ops.umap_knn(X, k, _METRICS[self.metric], idx, dist)
            core = dist[:, k - 1].contiguous()
        e, rounds = spanning_tree(X, core, None if pre else _METRICS[self.metric])
        out = tree_to_labels(e[:, 0], e[:, 1], np.ascontiguousarray(e[:, 2]).view(np.float32), N, self.min_cluster_size,
                             self.cluster_selection_method, self.allow_single_cluster, self.cluster_selection_epsilon)
        lo, hi, w = out["edges"]                                     # nothing is set before this line: a refused fit leaves no attribute
        self.n_features_in_ = int(X.shape[1])
        self._edges = (lo, hi, w)
        self.minimum_spanning_tree_ = np.stack([lo.astype(np.float64), hi.astype(np.float64), w], axis=1)
        self.single_linkage_tree_, self.condensed_tree_ = out["single_linkage_tree"], out["condensed_tree"]
        self.cluster_persistence_ = out["persistence"]
        self.labels_ = torch.from_numpy(out["labels"]).to(dev)
        self.probabilities_ = torch.from_numpy(out["probabilities"].astype(np.float32)).to(dev)
        self.core_distances_ = core
        self.n_clusters_, self.n_noise_, self.n_rounds_ = int(len(out["clusters"])), int((out["labels"] < 0).sum()), rounds
        return self

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_

    def dbscan_clustering(self, cut_distance, min_cluster_size=5):
        """sklearn's dbscan_clustering: DBSCAN* at eps = cut_distance from the fitted tree (the components of the tree edges
        below the cut; smaller ones than min_cluster_size are noise) -> int64 [N] on the device, numbered by smallest row."""
        lo, hi, w = self._edges
        labels = labels_at_cut(lo, hi, w, len(w) + 1, float(cut_distance), int(min_cluster_size))
        return torch.from_numpy(labels).to(self.labels_.device)


# ------------------------------------------------------------------------------------ the latents' density clusters
@dataclass
class HDBSCANReport:
    """Host values of one evaluate_hdbscan pass (labels stay on the device)."""
    min_cluster_size: int
    min_samples: int
    metric: str
    space: str
    n_clusters: int
    n_noise: int
    coverage: float                      # the share of the samples that are in a cluster
    cluster_sizes: np.ndarray            # int64 [n_clusters]
    cluster_persistence: np.ndarray      # float64 [n_clusters]: the chosen clusters' stabilities
    mean_probability: float              # of the clustered rows; NaN when nothing is clustered
    purity: float                        # over the clustered samples only; NaN when nothing is clustered
    nmi: float                           # likewise
    noise_per_class: np.ndarray          # int64 [classes]: the noise rows of every ground-truth label
    n_rounds: int
    labels: torch.Tensor                 # int64 [N] on the device, loader order (all ranks' rows, rank 0's first); -1 noise
    probabilities: torch.Tensor          # float32 [N] on the device
    n_samples: int
    fit_time: float
    inference_time: float


def default_min_cluster_size(n_samples, classes):
    """The stated rule for min_cluster_size=None, not a tuned one: max(5, N // (20 classes)) -- a twentieth of a class of
    average size."""
    return max(5, int(n_samples) // (20 * max(1, int(classes))))


@torch.no_grad()
def evaluate_hdbscan(model, config, dataloader, min_cluster_size=None, min_samples=None, metric=None, space="latent"):
    """HDBSCAN of the latents the SOM layer sees (the rows of evaluate_dbscan) -> HDBSCANReport: how many density clusters
    they form without an eps, which samples belong to none, and purity / NMI against the loader's labels over the CLUSTERED
    samples only (the noise rows are reported per class).
    min_cluster_size None: default_min_cluster_size(N, data.num_classes), a stated rule.  min_samples None: min_cluster_size
        held at 64, the most the class takes.
    metric: "cosine" or "euclidean"; None takes the SOM's distance_fcn when it is one of the two and "euclidean" otherwise.
    space: "latent" clusters the rows themselves; "umap" clusters the 2-D embedding of evaluation._umap_embed (euclidean
        there, whatever `metric` says: the embedding's own geometry) -- the canonical pairing.
    With model.world_size > 1 every rank gathers the rows (as evaluate_dbscan does) and computes the same report."""
    return _evaluate(model, config, dataloader, min_cluster_size, min_samples, metric, space, "evaluate_hdbscan")[0]


def _evaluate(model, config, dataloader, min_cluster_size, min_samples, metric, space, who, picture=False, fit_rows=None):
    """evaluate_hdbscan's one loader pass -> (the report, the rows' 2-D UMAP embedding on the device or None).  The embedding is
    computed once, when it is clustered (space "umap") or drawn (picture)."""
    from . import evaluation as E
    som = model.som_layer
    if metric is None:
        metric = som.distance_fcn if som.distance_fcn in ("cosine", "euclidean") else "euclidean"
    if metric not in METRICS:
        raise ValueError(f"{who}: metric must be one of {sorted(METRICS)}, got {metric!r}")
    if space not in ("latent", "umap"):
        raise ValueError(f"{who}: space must be 'latent' or 'umap', got {space!r}")
    start = time.time()
    X, y = _latents_and_labels(model, config, dataloader, who)
    N, dev = X.shape[0], X.device
    embedding = E._umap_embed(X, fit_rows)[1].contiguous() if space == "umap" or picture else None
    if space == "umap":
        X, metric = embedding, "euclidean"
    classes = int(config["data"].get("num_classes", 0))
    mcs = default_min_cluster_size(N, classes) if min_cluster_size is None else int(min_cluster_size)
    ms = min(mcs, MAX_MIN_SAMPLES, N - 1) if min_samples is None else int(min_samples)
    fit_start = time.time()
    hd = HDBSCAN(min_cluster_size=mcs, min_samples=ms, metric=metric).fit(X)
    fit_time = time.time() - fit_start
    labels = hd.labels_
    wide = E._label_count(config, None, True)
    inside = labels >= 0
    sizes = np.zeros(0, dtype=np.int64)
    purity = nmi = mean_p = float("nan")
    if hd.n_clusters_:
        table = E._Table(hd.n_clusters_, wide, dev)
        table.add(labels[inside], y[inside])
        w = table.numpy()
        sizes, purity, nmi = w.sum(axis=1).astype(np.int64), E.purity_from_table(w), E.nmi_from_table(w)
        mean_p = float(hd.probabilities_[inside].double().mean().item())
    noise = E._Table(1, wide, dev)
    if hd.n_noise_:
        noise.add(torch.zeros_like(y[~inside]), y[~inside])
    per_class = noise.numpy()[0].astype(np.int64)
    seen = int(np.flatnonzero(per_class).max()) + 1 if per_class.any() else 0
    inference_time = time.time() - start
    report = HDBSCANReport(min_cluster_size=mcs, min_samples=ms, metric=metric, space=space, n_clusters=hd.n_clusters_,
                           n_noise=hd.n_noise_, coverage=float(N - hd.n_noise_) / N, cluster_sizes=sizes,
                           cluster_persistence=np.asarray(hd.cluster_persistence_, dtype=np.float64), mean_probability=mean_p,
                           purity=purity, nmi=nmi, noise_per_class=per_class[:max(classes, seen)], n_rounds=hd.n_rounds_, labels=labels,
                           probabilities=hd.probabilities_, n_samples=N, fit_time=float(fit_time), inference_time=float(inference_time))
    print(f"HDBSCAN ({metric}, {space}, min_cluster_size {mcs}, min_samples {ms}): {report.n_clusters} clusters, "
          f"{report.n_noise} noise rows of {N}, Purity (HDBSCAN): {purity:.3f}, NMI (HDBSCAN): {nmi:.3f}, "
          f"Inference Time: {inference_time:.3f}")
    return report, embedding


@torch.no_grad()
def visualize_hdbscan(model, config, dataloader, min_cluster_size=None, min_samples=None, metric=None, space="latent", epoch=0,
                      output_dir="experiments/plots/vit_som/hdbscan", fit_rows=None):
    """visualize_dbscan's scatter of the rows evaluate_hdbscan clusters (same UMAP, same fit_rows), coloured by cluster with
    the noise rows in grey and every point's alpha from probabilities_ -> output_dir/som_hdbscan_epoch_{epoch}.png (rank 0
    only; skipped with a warning when matplotlib is missing).  One loader pass and one UMAP fit: with space="umap" the
    embedding that is drawn is the one that is clustered.  Returns (embedding [N, 2] float32, cluster labels [N] int64) as
    host arrays."""
    import os
    from . import evaluation as E
    who = "visualize_hdbscan"
    report, embedding = _evaluate(model, config, dataloader, min_cluster_size, min_samples, metric, space, who, picture=True,
                                  fit_rows=fit_rows)
    embedding = embedding.cpu().numpy()
    labels, prob = report.labels.cpu().numpy(), report.probabilities.cpu().numpy()
    if E._rank(model) == 0:
        plt = E._pyplot(who)
        if plt is not None:
            os.makedirs(output_dir, exist_ok=True)
            plt.figure(figsize=(10, 8), dpi=300)
            plt.axis("off")
            out = labels < 0
            plt.scatter(embedding[out, 0], embedding[out, 1], c="0.7", s=3, alpha=0.5, edgecolor="none", rasterized=True)
            colours = plt.get_cmap("tab10")(labels[~out] % 10)
            colours[:, 3] = 0.15 + 0.7 * prob[~out]
            plt.scatter(embedding[~out, 0], embedding[~out, 1], c=colours, s=3, edgecolor="none", rasterized=True)
            plt.savefig(os.path.join(output_dir, f"som_hdbscan_epoch_{epoch}.png"), **E._UMAP_SAVEFIG)
            plt.close()
    return embedding, labels
