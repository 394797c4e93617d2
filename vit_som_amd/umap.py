"""umap-learn's ``umap.UMAP`` (0.5: umap_.py) on the device, for visualize_umap_progression
(tools/evaluation.py:267-323).

As in kmeans.py, the steps that touch the data are HIP kernels: the exact k-nearest-neighbour search on the f32 matrix
cores (knn.hip, the search of the kNN probe with the set as its own bank) and one launch per layout epoch (umap.hip).  The host keeps the O(N k) decisions, vectorised numpy / scipy as
umap-learn itself does them: sigma / rho, the membership strengths, the set operations, the pruning, the a / b curve
fit and the spectral initialisation.  The kNN table and the graph are copied to the host once; the input never leaves
the device.  Everything is bitwise reproducible for a given ``random_state``.

The algorithm (umap-learn 0.5, restated; the departures are marked):

1. kNN: k = n_neighbors nearest rows of every row, the row itself included, ascending by (distance, index), the row
   itself first at distance 0 (vsom_umap_knn).  cosine = 1 - <x,y> / (|x||y|) (0 for two zero rows, 1 when exactly one
   is zero); euclidean is the true distance.
2. sigma, rho per row (smooth_knn_dist).  d = the row's k distances, nz = its non-zero distances in order,
   lc = local_connectivity, idx = floor(lc), t = lc - idx.
   rho: if len(nz) >= lc: nz[idx-1] (+ t (nz[idx] - nz[idx-1]) when t > 1e-5) if idx > 0, else t nz[0];
   otherwise max(nz) if nz is non-empty, else 0.
   sigma: binary search for sum_{j=1..k-1} f(d_j) = log2(k), f(d) = exp(-(d - rho) / sigma) if d - rho > 0 else 1
   (j = 0 skipped): lo = 0, hi = inf, sigma = 1, at most 64 steps, stop when |sum - target| < 1e-5; sum > target:
   hi = sigma, sigma = (lo + hi) / 2; else lo = sigma and sigma = 2 sigma if hi = inf, else (lo + hi) / 2.  Finally
   sigma >= 1e-3 mean(d) if rho > 0, else >= 1e-3 mean(all kNN distances).
3. Membership: w_ij = 0 for j = i; 1 if d_ij - rho_i <= 0 or sigma_i = 0; exp(-(d_ij - rho_i) / sigma_i) otherwise.
4. Symmetrise: with A the directed graph and P = A o A^T, G = mix (A + A^T - P) + (1 - mix) P (mix =
   set_op_mix_ratio), zeros dropped.  Each term is symmetric in floating point, so G is exactly symmetric (step 8
   relies on it).  ``graph_`` is G in float32, unpruned, as umap-learn keeps it.
5. n_epochs = 500 if N <= 10000 else 200 unless given.  Edges with w < max(w) / n_epochs are dropped;
   epochs_per_sample_e = max(w) / w_e (fp64), epochs_per_negative_sample_e = epochs_per_sample_e /
   negative_sample_rate; the next-sample / next-negative state starts at these values.
6. a, b: scipy.optimize.curve_fit of 1 / (1 + a x^(2b)) on x = linspace(0, 3 spread, 300) against y = 1 for
   x < min_dist and exp(-(x - min_dist) / spread) otherwise (defaults: a = 1.57694346, b = 0.89506088).
7. Init.  'spectral', connected graph: L = I - D^-1/2 G D^-1/2, scipy.sparse.linalg.eigsh(L, k=dim+1, which='SM',
   ncv=max(2(dim+1)+1, int(sqrt(N))), tol=1e-4, v0=ones, maxiter=5N), the eigenvectors of eigenvalues 2..dim+1.
   Several components: each laid out the same way around a meta-position (+-e_i for <= 2 dim components; more: the
   PCA of the component centroids in input space, scaled to unit maximum -- a departure, umap-learn embeds the
   centroids spectrally) and scaled to half the smallest distance between meta-positions; a component with fewer
   than 2 dim points, or <= dim + 1, is uniform random in that box.  Then x 10 / max|.| plus normal(scale=1e-4)
   noise.  If ARPACK fails: a warning and the random init.  'random': uniform(-10, 10).  An array is taken as given.
   'spectral_device' (opt-in): on a connected graph the same eigenvectors from the device solver of spectral.py
   (Chebyshev-filtered subspace iteration in fp64, residual <= 1e-8, a fixed start); with several components the host
   path above.  'spectral' stays ARPACK and stays the default.
   Then every column is normalised to [0, 10]: 10 (e - min) / (max - min).
   The fit draws from its RandomState in this order: 8 bytes (``bytes(8)``, little-endian) = the 64-bit seed of
   step 8; then the init: the uniform boxes of small components (in component order) and the normal noise
   ('spectral'), or the uniform init ('random').
8. Layout (optimize_layout_euclidean, move_other=True), epochs n = 0 .. n_epochs-1 (epoch 0 samples nothing, as
   epochs_per_sample >= 1); alpha_0 = learning_rate, alpha_n = learning_rate (1 - (n-1) / n_epochs).  Edge e = (v, u)
   is sampled in epoch n when next_e <= n.  Attraction: d2 = |y_v - y_u|^2, coefficient -2ab d2^(b-1) / (a d2^b + 1)
   (0 if d2 = 0).  Repulsion from a negative sample s: 2 gamma b / ((0.001 + d2)(a d2^b + 1)) (gamma =
   repulsion_strength) if d2 > 0; s == v is skipped, any other coincident sample adds 0.  Each term is
   clip(coef (y_v - y_other), -4, 4) per component.  After the attraction n_neg = floor((n - next_neg_e) /
   eps_neg_e), then next_e += epochs_per_sample_e and next_neg_e += n_neg eps_neg_e.
   Departure -- synchronous updates: umap-learn moves the points one edge at a time; here every term reads the
   epoch-start embedding and y_v' = y_v + alpha_n sum(terms), summed in CSR order: each sampled out-edge's
   attraction, then its n_neg repulsions.  As G is symmetric the reverse edge (u, v) has the same schedule, so the
   "move other" update umap-learn applies to v from (u, v) equals v's own attraction term: v adds it twice and
   nothing is scattered.
   Departure -- negative samples: a counter-based hash of (seed, epoch, edge index, p) instead of umap-learn's
   sequential Tausworthe draws: two splitmix64 rounds (include/vitsom_hip.h, vsom_umap_neg_sample) mod N.

transform(X) of M new rows into a fitted map (umap-learn 0.5's ``transform``, restated from memory like the steps above:
umap-learn is not a dependency and the restatement has not been run against it):

9.  X is the very tensor the model was fitted on: ``embedding_`` is returned.
10. Search: the k = n_neighbors nearest training rows of every new row, ascending by (distance, ordinal), nothing
    excluded and nothing put first (vsom_knn_query against the kept training tensor ``_raw_data``).
11. Graph (transform_graph, host, fp64): sigma / rho of step 2 over the [M, k] table with local_connectivity
    max(0, lc - 1) -- the sum still skips j = 0, which umap-learn's transform inherits from the fit although column 0
    is no longer the row itself; w_ij = 1 if d_ij - rho_i <= 0 or sigma_i = 0, else exp(-(d_ij - rho_i) / sigma_i),
    with no "self" column; every row divided by its sum (added in the order j = 0 .. k-1).  Edges with
    w < max(w) / n_epochs (max over the whole table) are pruned, epochs_per_sample = +inf; the others max(w) / w.
12. n_epochs = 100 if M <= 10000 else 30 when ``n_epochs`` is None, else n_epochs // 3; 0 returns the init.
13. Init and layout (vsom_umap_transform_layout, one launch): y_i = sum_j w_ij Y_train[idx_ij] in fp64, rounded once;
    then optimize_layout_euclidean with move_other=False: alpha_0 = learning_rate / 4, alpha_n = alpha_0
    (1 - (n-1) / n_epochs), gamma = repulsion_strength, the fit's a and b, the schedule of step 8 per (i, j) with
    next = eps and next_neg = eps / negative_sample_rate at the start.  Only the new point moves, and new points meet
    training points only, so each is laid out on its own, all epochs in one thread, and every term is applied at once
    in the order (epoch, j, attraction, negative samples) as umap-learn's loop applies them: step 8's synchronous
    departure is not needed here.  The attraction counts once.  A negative sample that coincides with the point adds
    nothing (umap-learn adds 4 per component there unless it is the point itself).
    Departure -- negative samples: step 8's hash with edge index i k + j (the position in the [M, k] table, so pruning
    does not shift it), drawn among the N training rows.  The seed is the first 8 bytes of a fresh
    RandomState(random_state), as in fit: transform does not depend on how often it was called before.
Not covered: supervised / parametric / inverse transform, densMAP, sparse input, other metrics.
"""
import warnings

import numpy as np
import scipy.sparse
import scipy.sparse.csgraph
import scipy.sparse.linalg
import torch

from . import ops
from .kmeans import _random_state

SMOOTH_K_TOLERANCE = 1e-5
MIN_K_DIST_SCALE = 1e-3
METRICS = {"euclidean": ops.DIST_EUCLIDEAN, "cosine": ops.DIST_COSINE}
MAX_COMPONENTS = 4                                               # vsom_umap_epoch: 1 <= dim <= 4


def smooth_knn_dist(knn_dist, local_connectivity=1.0, n_iter=64):
    """Step 2 for every row at once -> (sigma, rho), float64 [N]."""
    d = np.asarray(knn_dist, dtype=np.float64)
    N, k = d.shape
    lc = float(local_connectivity)
    nz = d > 0.0
    count = nz.sum(axis=1)
    # non-zero distances first, each row in its own order
    nzd = np.take_along_axis(d, np.argsort(~nz, axis=1, kind="stable"), axis=1)
    idx = int(np.floor(lc))
    t = lc - idx
    if idx > 0:
        lo_i = min(idx - 1, k - 1)
        r = nzd[:, lo_i].copy()
        if t > SMOOTH_K_TOLERANCE:
            r += t * (nzd[:, min(idx, k - 1)] - nzd[:, lo_i])
    else:
        r = t * nzd[:, 0]
    rho = np.where(count >= lc, r, np.where(count > 0, d.max(axis=1), 0.0))

    target = np.log2(k)
    x = d[:, 1:] - rho[:, None]
    lo, hi, mid = np.zeros(N), np.full(N, np.inf), np.ones(N)
    act = np.arange(N)
    for _ in range(n_iter):
        if act.size == 0:
            break
        xa, m = x[act], mid[act]
        with np.errstate(over="ignore"):
            term = np.where(xa > 0.0, np.exp(-(xa / m[:, None])), 1.0)
        psum = np.zeros(act.size)
        for j in range(k - 1):                                   # the scalar loop's order
            psum += term[:, j]
        keep = np.abs(psum - target) >= SMOOTH_K_TOLERANCE        # the others stop here
        act, psum = act[keep], psum[keep]
        gt = psum > target
        a_gt, a_le = act[gt], act[~gt]
        hi[a_gt] = mid[a_gt]
        mid[a_gt] = (lo[a_gt] + hi[a_gt]) / 2.0
        lo[a_le] = mid[a_le]
        inf = np.isinf(hi[a_le])
        mid[a_le[inf]] = mid[a_le[inf]] * 2
        a2 = a_le[~inf]
        mid[a2] = (lo[a2] + hi[a2]) / 2.0
    floor_ = MIN_K_DIST_SCALE * np.where(rho > 0.0, d.mean(axis=1), d.mean())
    sigma = np.where(mid < floor_, floor_, mid)
    return sigma, rho


def membership_strengths(knn_idx, knn_dist, sigma, rho):
    """Step 3 -> (rows, cols, vals) of the directed graph A."""
    knn_idx = np.asarray(knn_idx, dtype=np.int64)
    d = np.asarray(knn_dist, dtype=np.float64)
    N, k = knn_idx.shape
    x = d - rho[:, None]
    s = sigma[:, None]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        val = np.where((x <= 0.0) | (s == 0.0), 1.0, np.exp(-(x / s)))
    val[knn_idx == np.arange(N)[:, None]] = 0.0
    return np.repeat(np.arange(N, dtype=np.int64), k), knn_idx.ravel(), val.ravel()


def fuzzy_simplicial_set(knn_idx, knn_dist, set_op_mix_ratio=1.0, local_connectivity=1.0):
    """Steps 2-4 -> (G float64 CSR, exactly symmetric, sorted indices, no zeros; sigma; rho)."""
    N = knn_idx.shape[0]
    sigma, rho = smooth_knn_dist(knn_dist, local_connectivity)
    rows, cols, vals = membership_strengths(knn_idx, knn_dist, sigma, rho)
    A = scipy.sparse.coo_matrix((vals, (rows, cols)), shape=(N, N)).tocsr()
    A.eliminate_zeros()
    At = A.transpose().tocsr()
    P = A.multiply(At).tocsr()
    mix = float(set_op_mix_ratio)
    G = (mix * (A + At - P) + (1.0 - mix) * P).tocsr()
    G.eliminate_zeros()
    G.sort_indices()
    return G, sigma, rho


def find_ab_params(spread=1.0, min_dist=0.1):
    """Step 6: (a, b) of the curve 1 / (1 + a x^(2b))."""
    from scipy.optimize import curve_fit

    def curve(x, a, b):
        return 1.0 / (1.0 + a * x ** (2 * b))

    xv = np.linspace(0, spread * 3, 300)
    yv = np.zeros(xv.shape)
    yv[xv < min_dist] = 1.0
    yv[xv >= min_dist] = np.exp(-(xv[xv >= min_dist] - min_dist) / spread)
    params, _ = curve_fit(curve, xv, yv)
    return float(params[0]), float(params[1])


def default_n_epochs(N):
    return 500 if N <= 10000 else 200


def make_schedule(graph, n_epochs, negative_sample_rate):
    """Step 5 -> (pruned CSR graph, epochs_per_sample, epochs_per_negative_sample), the last two fp64 per edge in
    CSR order."""
    G = scipy.sparse.csr_matrix(graph, copy=True)
    w = G.data.astype(np.float64)
    G.data[w < w.max() / float(n_epochs)] = 0
    G.eliminate_zeros()
    G.sort_indices()
    w = G.data.astype(np.float64)
    eps = w.max() / w
    return G, eps, eps / float(negative_sample_rate)


def transform_n_epochs(n_epochs, M):
    """Step 12: the layout epochs of a transform of M rows by a model made with ``n_epochs``."""
    if n_epochs is None:
        return 100 if M <= 10000 else 30
    return int(n_epochs) // 3


def transform_graph(knn_idx, knn_dist, local_connectivity=1.0, n_epochs=100):
    """Step 11 -> (weights, epochs_per_sample), float64 [M, k]: the row-normalised memberships of the new rows in their
    k nearest training rows, and max(w) / w with +inf on the edges pruned for an n_epochs layout (n_epochs = 0 prunes
    them all).  Entry (i, j) belongs to the edge from new row i to training row knn_idx[i, j]: the graph keeps the
    table's layout, so the ordinals are only checked for their shape."""
    d = np.asarray(knn_dist, dtype=np.float64)
    if np.shape(knn_idx) != d.shape or d.ndim != 2:
        raise ValueError(f"transform_graph: knn_idx {np.shape(knn_idx)} and knn_dist {d.shape} must be the same [M, k]")
    sigma, rho = smooth_knn_dist(d, max(0.0, float(local_connectivity) - 1.0))
    x = d - rho[:, None]
    s = sigma[:, None]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        w = np.where((x <= 0.0) | (s == 0.0), 1.0, np.exp(-(x / s)))
    total = np.zeros(d.shape[0])
    for j in range(d.shape[1]):                                  # the scalar loop's order
        total += w[:, j]
    w = w / total[:, None]
    top = w.max()
    with np.errstate(divide="ignore"):
        eps = np.where(w < top / np.float64(n_epochs), np.inf, top / w)
    return w, eps


def _eigenmap(G, dim):
    """The eigenvectors of eigenvalues 2..dim+1 of I - D^-1/2 G D^-1/2 (one connected graph)."""
    from scipy.sparse.linalg import eigsh
    n = G.shape[0]
    G = G.astype(np.float64)
    deg = np.asarray(G.sum(axis=0)).ravel()
    Dm = scipy.sparse.spdiags(1.0 / np.sqrt(deg), 0, n, n)
    L = scipy.sparse.identity(n, dtype=np.float64) - Dm @ G @ Dm
    k = dim + 1
    ncv = max(2 * k + 1, int(np.sqrt(n)))
    vals, vecs = eigsh(L, k, which="SM", ncv=ncv, tol=1e-4, v0=np.ones(n), maxiter=n * 5)
    return vecs[:, np.argsort(vals)[1:k]]


_ARPACK_FAILURES = (scipy.sparse.linalg.ArpackError, ValueError)


def _meta_positions(n_comp, labels, dim, centroids):
    if n_comp <= 2 * dim:
        kk = int(np.ceil(n_comp / 2.0))
        base = np.hstack([np.eye(kk), np.zeros((kk, dim - kk))])
        return np.vstack([base, -base])[:n_comp]
    C = centroids(labels, n_comp)
    U, S, _ = np.linalg.svd(C - C.mean(axis=0), full_matrices=False)
    meta = np.zeros((n_comp, dim))
    r = min(dim, S.size)
    meta[:, :r] = U[:, :r] * S[:r]
    big = np.abs(meta).max()
    return meta / big if big > 0 else meta


def spectral_init(G, dim, rs, centroids, device=None):
    """Step 7's 'spectral' layout before the x 10 / max scaling and the noise.  `centroids(labels, n)` -> [n, D]
    float64 mean input row of every component.  device (init='spectral_device'): a connected graph's eigenvectors come
    from the device solver of spectral.py instead of ARPACK; several components take the host path either way."""
    n_comp, labels = scipy.sparse.csgraph.connected_components(G, directed=False)
    if n_comp == 1:
        if device is not None:
            from .spectral import eigenmap_device
            return eigenmap_device(G, dim, device)
        return _eigenmap(G, dim)
    meta = _meta_positions(n_comp, labels, dim, centroids)
    out = np.empty((G.shape[0], dim))
    Gr = G.tocsr()
    for c in range(n_comp):
        members = labels == c
        m = int(members.sum())
        dist = np.sqrt(((meta - meta[c]) ** 2).sum(axis=1))
        pos = dist[dist > 0.0]
        half = pos.min() / 2.0 if pos.size else 1.0
        if m < 2 * dim or m <= dim + 1:
            out[members] = rs.uniform(low=-half, high=half, size=(m, dim)) + meta[c]
            continue
        try:
            emb = _eigenmap(Gr[members][:, members], dim)
            out[members] = emb * (half / np.abs(emb).max()) + meta[c]
        except _ARPACK_FAILURES as e:
            warnings.warn(f"UMAP: spectral layout of component {c} failed ({e}); random init for it")
            out[members] = rs.uniform(low=-half, high=half, size=(m, dim)) + meta[c]
    return out


def _check_x(X, n_neighbors):
    """n_neighbors None: the rows of a transform, of which one is enough."""
    if not isinstance(X, torch.Tensor) or X.dim() != 2:
        raise ValueError("UMAP: X must be a float32 [N, D] tensor on the GPU")
    if n_neighbors is None and X.shape[0] < 1:
        raise ValueError("UMAP: X has no rows")
    if n_neighbors is not None and X.shape[0] <= n_neighbors:
        raise ValueError(f"UMAP: N={X.shape[0]} rows must exceed n_neighbors={n_neighbors}")
    if X.shape[1] < 1:
        raise ValueError("UMAP: X has no columns")
    if X.dtype != torch.float32:
        raise ValueError(f"UMAP: X must be float32, got {X.dtype}")
    if not X.is_cuda:
        raise ValueError("UMAP: X must be on the GPU (there is no CPU path)")
    if not X.is_contiguous():
        raise ValueError("UMAP: X must be contiguous")
    return X


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


class UMAP:
    """umap.UMAP for a float32 [N, D] device tensor, with umap-learn's parameter names and defaults (the subset
    listed; module docstring for the algorithm and its departures).  After ``fit``: ``embedding_`` float32
    [N, n_components] on the device, ``graph_`` (scipy CSR, float32, the unpruned fuzzy graph), ``_a``, ``_b``, and
    ``_raw_data``: the training tensor itself, a reference and not a copy, which ``transform`` searches -- the caller
    must not overwrite it while the model is in use."""

    def __init__(self, n_neighbors=15, n_components=2, metric="euclidean", n_epochs=None, learning_rate=1.0,
                 init="spectral", min_dist=0.1, spread=1.0, set_op_mix_ratio=1.0, local_connectivity=1.0,
                 repulsion_strength=1.0, negative_sample_rate=5, random_state=None):
        self.n_neighbors, self.n_components, self.metric, self.n_epochs = n_neighbors, n_components, metric, n_epochs
        self.learning_rate, self.init, self.min_dist, self.spread = learning_rate, init, min_dist, spread
        self.set_op_mix_ratio, self.local_connectivity = set_op_mix_ratio, local_connectivity
        self.repulsion_strength, self.negative_sample_rate = repulsion_strength, negative_sample_rate
        self.random_state = random_state

    def _validate(self):
        if not _is_int(self.n_neighbors) or not 2 <= self.n_neighbors <= ops.UMAP_MAX_K:
            raise ValueError(f"UMAP: n_neighbors must be an integer in [2, {ops.UMAP_MAX_K}], got {self.n_neighbors!r}")
        if not _is_int(self.n_components) or not 1 <= self.n_components <= MAX_COMPONENTS:
            raise ValueError(f"UMAP: n_components must be an integer in [1, {MAX_COMPONENTS}], got {self.n_components!r}")
        if not isinstance(self.metric, str) or self.metric not in METRICS:
            raise ValueError(f"UMAP: metric must be one of {sorted(METRICS)}, got {self.metric!r}")
        if self.n_epochs is not None and (not _is_int(self.n_epochs) or self.n_epochs < 1):
            raise ValueError(f"UMAP: n_epochs must be None or a positive integer, got {self.n_epochs!r}")
        if isinstance(self.init, str) and self.init not in ("spectral", "spectral_device", "random"):
            raise ValueError(f"UMAP: init must be 'spectral', 'spectral_device', 'random' or an array, got {self.init!r}")
        if not self.learning_rate > 0:
            raise ValueError("UMAP: learning_rate must be positive")
        if not (self.min_dist >= 0 and self.spread > 0 and self.min_dist <= self.spread):
            raise ValueError("UMAP: need 0 <= min_dist <= spread and spread > 0")
        if not 0.0 <= self.set_op_mix_ratio <= 1.0:
            raise ValueError("UMAP: set_op_mix_ratio must lie in [0, 1]")
        if not self.local_connectivity >= 0:
            raise ValueError("UMAP: local_connectivity must not be negative")
        if not self.repulsion_strength >= 0:
            raise ValueError("UMAP: repulsion_strength must not be negative")
        if not _is_int(self.negative_sample_rate) or self.negative_sample_rate < 1:
            raise ValueError("UMAP: negative_sample_rate must be a positive integer")

    def _centroids(self, X):
        def centroids(labels, n):
            lab = torch.from_numpy(labels.astype(np.int64)).to(X.device)
            order = torch.argsort(lab, stable=True)
            counts = np.bincount(labels, minlength=n)
            rows, start = [], 0
            for c in range(n):
                rows.append(X.index_select(0, order[start:start + counts[c]]).double().mean(dim=0))
                start += counts[c]
            return torch.stack(rows).cpu().numpy()
        return centroids

    def _initial(self, X, G, rs):
        N, dim = X.shape[0], self.n_components
        if not isinstance(self.init, str):
            init = self.init.detach().cpu().numpy() if isinstance(self.init, torch.Tensor) else np.asarray(self.init)
            if init.shape != (N, dim):
                raise ValueError(f"UMAP: init has shape {init.shape}, expected {(N, dim)}")
            emb = init.astype(np.float64)
        elif self.init == "random":
            emb = rs.uniform(low=-10.0, high=10.0, size=(N, dim))
        else:
            try:
                emb = spectral_init(G, dim, rs, self._centroids(X), X.device if self.init == "spectral_device" else None)
            except _ARPACK_FAILURES as e:
                warnings.warn(f"UMAP: spectral initialisation failed ({e}); falling back to random init")
                emb = None
            if emb is None:
                emb = rs.uniform(low=-10.0, high=10.0, size=(N, dim))
            else:
                emb = emb * (10.0 / np.abs(emb).max()) + rs.normal(scale=0.0001, size=(N, dim))
        lo, hi = emb.min(axis=0), emb.max(axis=0)
        span = np.where(hi > lo, hi - lo, 1.0)
        return 10.0 * (emb - lo) / span

    def fit(self, X):
        self._validate()
        X = _check_x(X, self.n_neighbors)
        N, k, dim = X.shape[0], self.n_neighbors, self.n_components
        dev = X.device
        idx = torch.empty(N, k, dtype=torch.int64, device=dev)
        dist = torch.empty(N, k, dtype=torch.float32, device=dev)
        ops.umap_knn(X, k, METRICS[self.metric], idx, dist)
        n_empty = int((idx < 0).sum())               # N > k: a slot is empty only where a pair has no distance
        if n_empty:
            raise ValueError(f"UMAP: {n_empty} neighbour slots are empty although N={N} exceeds n_neighbors={k}: X holds NaN "
                             f"or infinity, or a row's squared norm overflows float32")
        self._knn_indices, self._knn_dists = idx.cpu().numpy(), dist.cpu().numpy()
        G, self._sigmas, self._rhos = fuzzy_simplicial_set(self._knn_indices, self._knn_dists, self.set_op_mix_ratio,
                                                           self.local_connectivity)
        self.graph_ = G.astype(np.float32)
        self._a, self._b = find_ab_params(self.spread, self.min_dist)
        n_epochs = self.n_epochs if self.n_epochs is not None else default_n_epochs(N)
        rs = _random_state(self.random_state)
        seed = int(np.frombuffer(rs.bytes(8), dtype="<u8")[0])
        emb = self._initial(X, self.graph_, rs)

        P, eps, eps_neg = make_schedule(self.graph_, n_epochs, self.negative_sample_rate)

        def dev_t(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        indptr, indices = dev_t(P.indptr.astype(np.int64)), dev_t(P.indices.astype(np.int64))
        eps_d, eps_neg_d = dev_t(eps), dev_t(eps_neg)
        nxt, nxt_neg = eps_d.clone(), eps_neg_d.clone()
        Y = [dev_t(emb.astype(np.float32)), torch.empty(N, dim, dtype=torch.float32, device=dev)]
        lr = float(self.learning_rate)
        for n in range(n_epochs):
            alpha = lr if n == 0 else lr * (1.0 - (n - 1) / float(n_epochs))
            ops.umap_epoch(indptr, indices, eps_d, nxt, eps_neg_d, nxt_neg, Y[0], Y[1], self._a, self._b,
                           self.repulsion_strength, alpha, n, seed)
            Y.reverse()
        self.embedding_ = Y[0]
        self._n_epochs, self._layout_seed = n_epochs, seed
        self._raw_data = X                                       # a reference: transform() searches it
        return self

    def fit_transform(self, X):
        return self.fit(X).embedding_

    def transform(self, X):
        """Steps 9-13: float32 [M, D] device tensor -> float32 [M, n_components] device tensor, the new rows placed in
        the fitted embedding, which does not move.  Reproducible: the result depends on X, the fit and ``random_state``
        only."""
        if not hasattr(self, "embedding_"):
            raise ValueError("UMAP: transform() needs a fitted model; call fit() first")
        self._validate()
        train = self._raw_data
        if X is train:
            return self.embedding_
        if isinstance(X, torch.Tensor) and X.dim() == 2 and X.shape[1] != train.shape[1]:
            raise ValueError(f"UMAP: X has {X.shape[1]} columns, the model was fitted on {train.shape[1]}")
        X = _check_x(X, None)
        if X.device != train.device:
            raise ValueError(f"UMAP: X is on {X.device}, the model was fitted on {train.device}")
        M, N, k, dim = X.shape[0], train.shape[0], self.n_neighbors, self.n_components
        if N < k:
            raise ValueError(f"UMAP: the {N} training rows are fewer than n_neighbors={k}")
        dev = X.device
        idx = torch.empty(M, k, dtype=torch.int64, device=dev)
        dist = torch.empty(M, k, dtype=torch.float32, device=dev)
        ops.knn_query(X, train, k, METRICS[self.metric], idx, dist)
        n_epochs = transform_n_epochs(self.n_epochs, M)
        weights, eps = transform_graph(idx.cpu().numpy(), dist.cpu().numpy(), self.local_connectivity, n_epochs)
        seed = int(np.frombuffer(_random_state(self.random_state).bytes(8), dtype="<u8")[0])
        Y = torch.empty(M, dim, dtype=torch.float32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        ops.umap_transform_layout(idx, torch.from_numpy(weights).to(dev), torch.from_numpy(eps).to(dev), self.embedding_, Y,
                                  self._a, self._b, self.repulsion_strength, float(self.learning_rate) / 4.0, n_epochs, 0,
                                  n_epochs, self.negative_sample_rate, seed, status,
                                  ops.umap_transform_workspace(M, k, dev))
        refused = int(status.item())
        if refused:
            raise ValueError(f"UMAP: the transform layout refused {refused} edges (a neighbour outside the training set, or "
                             f"a weight or schedule entry that is not a number)")
        return Y
