"""numpy restatement of the on-device HDBSCAN (csrc/knn.hip's HDBSCAN section, vit_som_amd/hdbscan.py), in fp64 and
deliberately naive: (1) mutual reachability from a distance matrix and its minimum spanning tree under the strict total
order (w, lo, hi) -- Kruskal over all pairs, and Prim for the sizes at which sorting all pairs is slow (the tree is unique,
so both give the same edges; test_hdbscan_cpu.py checks that); (2) the single-linkage hierarchy, the condensed tree, the
stabilities, the selection and the labels with explicit member lists and dictionaries, written independently of the
product's array code; (3) the fixtures of the issue and the comparisons of two labelings."""
import math

import numpy as np

COSINE, EUCLIDEAN = 0, 1                       # VSOM_DIST_*


# ------------------------------------------------------------------ (1) mutual reachability and its spanning tree
def core_distances(D, min_samples):
    """The distance of every row to its min_samples-th nearest row, the row itself counted (sklearn's rule): column
    min_samples - 1 of the sorted row."""
    return np.partition(np.asarray(D), int(min_samples) - 1, axis=1)[:, int(min_samples) - 1]


def mutual_reachability(D, min_samples, core=None):
    D = np.asarray(D)
    core = core_distances(D, min_samples) if core is None else np.asarray(core, dtype=D.dtype)
    return np.maximum(np.maximum(core[:, None], core[None, :]), D), core


def kruskal(W):
    """The N - 1 edges of the minimum spanning tree of the complete graph W (symmetric; the diagonal is not read) under
    (w, lo, hi) -> (lo, hi, w) in that order.  All pairs are sorted."""
    n = W.shape[0]
    lo, hi = np.triu_indices(n, 1)
    w = W[lo, hi]
    order = np.lexsort((hi, lo, w))
    parent = list(range(n))
    out = []
    for e in order.tolist():
        a, b = int(lo[e]), int(hi[e])
        while parent[a] != a:
            a = parent[a]
        while parent[b] != b:
            b = parent[b]
        if a != b:
            parent[max(a, b)] = min(a, b)
            out.append(e)
            if len(out) == n - 1:
                break
    out = np.asarray(out, dtype=np.int64)
    return lo[out].astype(np.int64), hi[out].astype(np.int64), w[out]


def prim(W):
    """The same tree by Prim's algorithm, O(N^2): every row outside the tree keeps its least edge into the tree under
    (w, lo, hi), and the least of those joins.  Returned in the order (w, lo, hi)."""
    n = W.shape[0]
    idx = np.arange(n)
    inside = np.zeros(n, dtype=bool)
    inside[0] = True
    bw = W[0].copy()
    blo, bhi = np.minimum(idx, 0), np.maximum(idx, 0)
    edges = []
    big = np.asarray(np.inf, dtype=W.dtype)
    for _ in range(n - 1):
        open_w = np.where(inside, big, bw)
        cand = np.flatnonzero(open_w == open_w.min())                # the rows outside the tree at the least weight
        k = cand[np.lexsort((bhi[cand], blo[cand]))[0]] if len(cand) > 1 else cand[0]
        edges.append((int(blo[k]), int(bhi[k]), bw[k]))
        inside[k] = True
        w, lo, hi = W[k], np.minimum(idx, k), np.maximum(idx, k)
        better = (w < bw) | ((w == bw) & ((lo < blo) | ((lo == blo) & (hi < bhi))))
        better &= ~inside
        bw[better], blo[better], bhi[better] = w[better], lo[better], hi[better]
    lo, hi = np.asarray([e[0] for e in edges], dtype=np.int64), np.asarray([e[1] for e in edges], dtype=np.int64)
    w = np.asarray([e[2] for e in edges], dtype=W.dtype)
    order = np.lexsort((hi, lo, w))
    return lo[order], hi[order], w[order]


def is_spanning_tree(lo, hi, n):
    """N - 1 edges that join all N rows."""
    if len(lo) != n - 1:
        return False
    parent = list(range(n))
    for a, b in zip(np.asarray(lo).tolist(), np.asarray(hi).tolist()):
        while parent[a] != a:
            a = parent[a]
        while parent[b] != b:
            b = parent[b]
        if a == b:
            return False
        parent[a] = b
    return True


# ------------------------------------------------------------------ (2) the hierarchy, naively
def naive_hdbscan(lo, hi, w, n, min_cluster_size=5, method="eom", allow_single_cluster=False, epsilon=0.0):
    """Labels (numbered by smallest row, -1 noise) and probabilities from tree edges sorted by (w, lo, hi), following
    sklearn's _tree.pyx step by step with member lists and dictionaries."""
    # the dendrogram: node n + k joins the two nodes edge k connects
    members = {i: [i] for i in range(n)}
    top = list(range(n))                       # the current node of every row's component, by representative
    rep = list(range(n))

    def find(a):
        while rep[a] != a:
            a = rep[a]
        return a
    kids, height = {}, {}
    for k, (a, b, d) in enumerate(zip(np.asarray(lo).tolist(), np.asarray(hi).tolist(), np.asarray(w, dtype=np.float64).tolist())):
        ra, rb = find(a), find(b)
        assert ra != rb
        node = n + k
        kids[node], height[node] = (top[ra], top[rb]), d
        members[node] = members[top[ra]] + members[top[rb]]
        rep[rb] = ra
        top[ra] = node
    root = 2 * n - 2
    # the condensed tree
    rows = []                                  # (parent, child, lambda, size)
    next_id = n + 1
    stack = [(root, n)]
    while stack:
        node, c = stack.pop()
        if node < n:
            continue
        a, b = kids[node]
        lam = 1.0 / height[node] if height[node] > 0.0 else math.inf
        na, nb = len(members[a]), len(members[b])
        if na >= min_cluster_size and nb >= min_cluster_size:
            for child, size in ((a, na), (b, nb)):
                rows.append((c, next_id, lam, size))
                stack.append((child, next_id))
                next_id += 1
        else:
            for child, size in ((a, na), (b, nb)):
                if size >= min_cluster_size:
                    stack.append((child, c))
                else:
                    rows.extend((c, p, lam, 1) for p in members[child])
    clusters = sorted({r[0] for r in rows} | {r[1] for r in rows if r[3] > 1})
    up = {r[1]: r[0] for r in rows if r[3] > 1}
    birth = {r[1]: r[2] for r in rows if r[3] > 1}
    birth[n] = 0.0
    below = {c: [r[1] for r in rows if r[0] == c and r[3] > 1] for c in clusters}
    stability = {c: 0.0 for c in clusters}
    for p, _, lam, size in rows:
        stability[p] += (lam - birth[p]) * size
    persistence = dict(stability)

    def descendants(c):
        out, todo = [], list(below[c])
        while todo:
            x = todo.pop()
            out.append(x)
            todo.extend(below[x])
        return out

    def epsilon_search(cands):
        chosen, done = set(), set()
        for leaf in cands:
            if 1.0 / birth[leaf] >= epsilon if birth[leaf] > 0 else True:
                chosen.add(leaf)
                continue
            if leaf in done:
                continue
            node = leaf
            while True:
                if up[node] == n:
                    node = n if allow_single_cluster else node
                    break
                node = up[node]
                if 1.0 / birth[node] > epsilon:
                    break
            chosen.add(node)
            done.update(descendants(node))
        return chosen

    order = sorted(clusters, reverse=True)
    if not allow_single_cluster:
        order = order[:-1]
    is_cluster = {c: True for c in order}
    if method == "eom":
        for c in order:
            sub = sum(stability[k] for k in below[c])
            if sub > stability[c]:
                is_cluster[c] = False
                stability[c] = sub
            else:
                for k in descendants(c):
                    is_cluster[k] = False
        chosen = {c for c in is_cluster if is_cluster[c]}
        if epsilon != 0.0 and len(clusters) > 1:
            if chosen == {n}:
                chosen = chosen if allow_single_cluster else set()
            else:
                chosen = epsilon_search(sorted(chosen))
    else:
        leaves = [c for c in clusters if c != n and not below[c]]
        chosen = epsilon_search(leaves) if epsilon != 0.0 and leaves else set(leaves)
    # labels and probabilities
    death = {c: max(r[2] for r in rows if r[0] == c) for c in clusters}
    owner, lam_of = {}, {}
    for p, child, lam, size in rows:
        if size > 1:
            continue
        c = p
        while c not in chosen and c != n:
            c = up[c]
        if c not in chosen:
            c = None
        elif c == n:
            if len(chosen) == 1 and allow_single_cluster:
                threshold = 1.0 / epsilon if epsilon != 0.0 else max(r[2] for r in rows if r[0] == n)
                c = n if lam >= threshold else None
            else:
                c = None
        owner[child], lam_of[child] = c, lam
    smallest = {}
    for p in range(n):
        if owner[p] is not None:
            smallest[owner[p]] = min(smallest.get(owner[p], n), p)
    number = {c: k for k, c in enumerate(sorted(smallest, key=smallest.get))}
    labels, prob = np.full(n, -1, dtype=np.int64), np.zeros(n)
    for p in range(n):
        c = owner[p]
        if c is None:
            continue
        labels[p] = number[c]
        prob[p] = 1.0 if death[c] == 0.0 or math.isinf(lam_of[p]) else min(lam_of[p], death[c]) / death[c]
    return labels, prob, np.asarray([persistence[c] for c in sorted(number, key=number.get)])


def naive_cut(lo, hi, w, n, cut, min_cluster_size):
    """sklearn's labelling_at_cut: the components of the edges below the cut; the small ones are noise."""
    group = list(range(n))
    for a, b, d in zip(np.asarray(lo).tolist(), np.asarray(hi).tolist(), np.asarray(w).tolist()):
        if d < cut:
            ga, gb = group[a], group[b]
            group = [ga if g == gb else g for g in group]
    labels, number = np.full(n, -1, dtype=np.int64), {}
    for p in range(n):
        if group.count(group[p]) >= min_cluster_size:
            labels[p] = number.setdefault(group[p], len(number))
    return labels


# ------------------------------------------------------------------ (3) fixtures and comparisons
SHAPES = [(257, 12288), (333, 1003), (130, 3), (700, 64)]
PARAMS = [(5, None), (12, 4)]                  # (min_cluster_size, min_samples)
OFFSETS = [0.0, 50.0]


def blobs(N, D, offset=0.0, centers=3):
    """make_blobs(N - 12, D, centers, cluster_std=1.0, random_state=N + D) plus 12 uniform rows over the data's range
    (RandomState(N)), plus `offset` on every coordinate -> float32 [N, D]."""
    from sklearn.datasets import make_blobs
    X, _ = make_blobs(n_samples=N - 12, n_features=D, centers=centers, cluster_std=1.0, random_state=N + D)
    out = np.random.RandomState(N).uniform(X.min(), X.max(), (12, D))
    return (np.concatenate([X, out]) + offset).astype(np.float32)


def distances64(X, metric):
    """fp64 distances: euclidean in sklearn's own form (pairwise_distances), cosine from normalised rows; zero diagonal."""
    X = np.asarray(X, dtype=np.float64)
    if metric == EUCLIDEAN:
        from sklearn.metrics import pairwise_distances
        D = pairwise_distances(X)
    else:
        U = X / np.sqrt((X * X).sum(1))[:, None]
        D = np.maximum(1.0 - U @ U.T, 0.0)
        D = 0.5 * (D + D.T)
    np.fill_diagonal(D, 0.0)
    return D


def same_partition(a, b):
    """Two labelings with -1 for noise describe the same noise set and the same clusters up to their numbers."""
    a, b = np.asarray(a), np.asarray(b)
    if not np.array_equal(a < 0, b < 0):
        return False
    pairs = set(zip(a[a >= 0].tolist(), b[b >= 0].tolist()))
    return len(pairs) == len({p[0] for p in pairs}) == len({p[1] for p in pairs})


def labels_that_differ(a, b):
    """The fewest rows whose label must change to turn labeling a into b up to the clusters' numbers (-1, noise, is itself):
    N less the best one-to-one matching of the clusters."""
    from scipy.optimize import linear_sum_assignment
    a, b = np.asarray(a), np.asarray(b)
    both = (a >= 0) & (b >= 0)
    table = np.zeros((a.max() + 1 if both.any() else 1, b.max() + 1 if both.any() else 1), dtype=np.int64)
    np.add.at(table, (a[both], b[both]), 1)
    rows, cols = linear_sum_assignment(-table)
    return int(len(a) - ((a < 0) & (b < 0)).sum() - table[rows, cols].sum())


def rand_index_is_one(a, b):
    from sklearn.metrics import adjusted_rand_score
    return adjusted_rand_score(a, b) == 1.0
