"""sklearn.cluster.KMeans (sklearn/cluster/_kmeans.py, algorithm="lloyd") on the device, for evaluate_kmeans
(tools/evaluation.py:54-91).

Every step that touches the data is a HIP kernel (kmeans.hip): k-means++ distances and potentials, the tolerance's
column variances, the fused E-step / partial M-step (one launch per Lloyd iteration), the slab reduction and the
empty-cluster relocation.  The host keeps what sklearn decides with its random numbers and small arrays:
the draws of one ``np.random.RandomState`` shared by all ``n_init`` runs (``choice`` for the first centre,
``uniform * current_pot`` + ``searchsorted`` on the cumulative ``closest_dist_sq`` for the candidates), the
convergence tests on a four-number device status read once per iteration, and ``np.argpartition`` of the distances
when a cluster is empty (the only time they are copied to the host).  The features never leave the device.

Differences from sklearn, all below fp32 rounding on data with margins: distances are fp32 sums of squared
differences (sklearn: |x|^2 - 2 x.c + |c|^2 on mean-centred data), potentials and inertia are fp64 sums, and
``center_shift_tot`` is the fp64 sum of the squared shifts.  No sample weights, Elkan, sparse input or mini-batch.
"""
import math

import numpy as np
import torch

from . import ops


def _check_x(X):
    if not (isinstance(X, torch.Tensor) and X.is_cuda and X.dtype == torch.float32 and X.dim() == 2):
        raise ValueError("KMeans: X must be a float32 [N, D] tensor on the GPU")
    if X.shape[1] > 0 and X.stride(1) != 1:
        X = X.contiguous()
    return X


def _random_state(seed):
    if isinstance(seed, np.random.RandomState):
        return seed
    return np.random.RandomState(seed)                     # sklearn.utils.check_random_state


class _Work:
    """Device buffers of one fit (shape-dependent, reused by every run)."""

    def __init__(self, N, D, k, device):
        self.ws = torch.empty(max(ops.kmeans_workspace_bytes(N, D, k), 16), dtype=torch.uint8, device=device)
        self.labels = [torch.empty(N, dtype=torch.int64, device=device) for _ in range(2)]
        self.mind = torch.empty(N, dtype=torch.float32, device=device)
        self.counts = torch.empty(k, dtype=torch.int64, device=device)
        self.status = torch.empty(4, dtype=torch.float64, device=device)
        self.centers = [torch.empty(k, D, dtype=torch.float32, device=device) for _ in range(2)]


def _refuse_non_finite(X, what):
    """sklearn refuses such input up front; here the kernels have already said so (a row at no finite distance from any
    centre joins cluster 0 with mind = inf or keeps a NaN potential), and the rows are counted to name them."""
    sq = torch.empty(X.shape[0], dtype=torch.float32, device=X.device)
    ops.row_sqnorm(X, sq)
    n = int((~torch.isfinite(sq)).sum())
    raise ValueError(f"KMeans: the {what} is not finite: {n} rows of X hold NaN or infinity, or their squared norm "
                     f"overflows float32")


def _kmeans_plusplus(X, n_clusters, rs, n_local_trials=None):
    """_kmeans_plusplus (unit weights) -> (centers [k, D] device tensor, indices np.int64 [k])."""
    N, D = X.shape
    dev = X.device
    if n_local_trials is None:
        n_local_trials = 2 + int(np.log(n_clusters))
    sw = np.ones(N, dtype=np.float32)
    indices = np.full(n_clusters, -1, dtype=np.int64)
    indices[0] = rs.choice(N, p=sw / sw.sum())
    closest = torch.empty(1, N, dtype=torch.float32, device=dev)
    pots = torch.empty(max(n_local_trials, 1), dtype=torch.float64, device=dev)
    ops.kmeanspp_dist(X, torch.tensor(indices[:1], device=dev), None, closest, pots)
    current_pot = float(pots[0])
    if not math.isfinite(current_pot):
        _refuse_non_finite(X, "k-means++ potential")
    closest_h = closest[0].cpu().numpy()
    dist = torch.empty(n_local_trials, N, dtype=torch.float32, device=dev)
    for c in range(1, n_clusters):
        rand_vals = rs.uniform(size=n_local_trials) * current_pot
        cand = np.searchsorted(np.cumsum(closest_h, dtype=np.float64), rand_vals)
        np.clip(cand, None, N - 1, out=cand)
        ops.kmeanspp_dist(X, torch.from_numpy(cand.astype(np.int64)).to(dev), closest[0], dist, pots)
        pots_h = pots[:n_local_trials].cpu().numpy()
        best = int(np.argmin(pots_h))
        current_pot = float(pots_h[best])
        closest[0].copy_(dist[best])
        closest_h = closest[0].cpu().numpy()
        indices[c] = cand[best]
    centers = X[torch.from_numpy(indices).to(dev)].contiguous()
    return centers, indices


def kmeans_plusplus(X, n_clusters, random_state=None, n_local_trials=None):
    """sklearn.cluster.kmeans_plusplus(X, n_clusters, random_state=...) on the device: (centers, indices)."""
    X = _check_x(X)
    if not 1 <= n_clusters <= X.shape[0]:
        raise ValueError(f"n_samples={X.shape[0]} should be >= n_clusters={n_clusters}")
    return _kmeans_plusplus(X, n_clusters, _random_state(random_state), n_local_trials)


def _is_same_clustering(a, b, k, device):
    """sklearn.utils._is_same_clustering: every cluster of `a` maps onto one cluster of `b`."""
    table = torch.zeros(k, k, dtype=torch.int64, device=device)
    bad = torch.zeros(1, dtype=torch.int32, device=device)
    ops.contingency(a, b, table, bad)
    return bool(((table.cpu().numpy() > 0).sum(axis=1) <= 1).all())


def _lloyd(X, centers_init, max_iter, tol, w):
    """_kmeans_single_lloyd -> (labels, inertia, centers, n_iter); labels / centers are views of w's buffers."""
    N = X.shape[0]
    cur, new = w.centers
    cur.copy_(centers_init)
    lab, lab_next = w.labels
    lab.fill_(-1)                                         # labels_old starts at -1: the first pass changes every label
    strict, it, st = False, 0, None
    for it in range(max_iter):
        ops.kmeans_assign(X, cur, lab_next, lab, w.mind, w.ws)
        ops.kmeans_update(cur, new, N, w.mind, w.counts, w.status, w.ws)
        st = w.status.tolist()                            # the one host read of the iteration
        if not math.isfinite(st[3]):
            _refuse_non_finite(X, "inertia")
        if st[2] > 0:                                     # _relocate_empty_clusters_dense
            counts = w.counts.cpu().numpy()
            empty = np.where(counts == 0)[0]
            n_empty = empty.shape[0]
            far = np.argpartition(w.mind.cpu().numpy(), -n_empty)[:-n_empty - 1:-1]
            moves = torch.from_numpy(np.stack([empty, far], axis=1).astype(np.int64)).to(X.device)
            ops.kmeans_relocate(X, lab_next, moves, cur, new, w.counts, w.status, w.ws)
            st = w.status.tolist()
        cur, new = new, cur
        lab, lab_next = lab_next, lab
        if st[0] == 0:
            strict = True
            break
        if st[1] <= tol:
            break
    if not strict:
        # rerun the E-step so that the labels match the final centres; its update only serves the inertia
        ops.kmeans_assign(X, cur, lab_next, lab, w.mind, w.ws)
        ops.kmeans_update(cur, new, N, w.mind, w.counts, w.status, w.ws)
        lab = lab_next
        st = w.status.tolist()
    return lab, st[3], cur, it + 1


class KMeans:
    """sklearn.cluster.KMeans(n_clusters, init="k-means++", n_init, max_iter, tol, random_state, algorithm="lloyd")
    for a float32 [N, D] device tensor (a row stride is fine).  ``init`` may also be an array of initial centres
    (then a single run, as in sklearn).  After fit: ``cluster_centers_`` [k, D] and ``labels_`` (int64) on the device,
    ``inertia_`` and ``n_iter_`` with sklearn's meaning."""

    def __init__(self, n_clusters=8, n_init=10, max_iter=300, tol=1e-4, random_state=0, init="k-means++"):
        self.n_clusters, self.n_init, self.max_iter, self.tol = int(n_clusters), int(n_init), int(max_iter), float(tol)
        self.random_state, self.init = random_state, init

    def fit(self, X):
        X = _check_x(X)
        N, D = X.shape
        k = self.n_clusters
        if not 1 <= k <= N:
            raise ValueError(f"n_samples={N} should be >= n_clusters={k}")
        w = _Work(N, D, k, X.device)
        tol = 0.0
        if self.tol:                                      # _tolerance: mean(var(X, axis=0)) * tol
            var = torch.empty(1, dtype=torch.float64, device=X.device)
            ops.kmeans_colvar(X, k, var, w.ws)
            tol = float(var) * self.tol
        rs = _random_state(self.random_state)
        given = not (isinstance(self.init, str) and self.init == "k-means++")
        if given:
            init = torch.as_tensor(np.asarray(self.init) if not isinstance(self.init, torch.Tensor) else self.init)
            init = init.to(device=X.device, dtype=torch.float32).contiguous()
            if init.shape != (k, D):
                raise ValueError(f"init has shape {tuple(init.shape)}, expected {(k, D)}")
        best = None
        for _ in range(1 if given else self.n_init):
            c0 = init if given else _kmeans_plusplus(X, k, rs)[0]
            labels, inertia, centers, n_iter = _lloyd(X, c0, self.max_iter, tol, w)
            if best is None or (inertia < best[1] and not _is_same_clustering(labels, best[0], k, X.device)):
                best = (labels.clone(), inertia, centers.clone(), n_iter)
        self.labels_, self.inertia_, self.cluster_centers_, self.n_iter_ = best
        return self

    def fit_predict(self, X):
        return self.fit(X).labels_
