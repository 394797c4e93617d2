"""scikit-learn's ``sklearn.manifold.TSNE`` (1.7: manifold/_t_sne.py, _utils.pyx) on the device, next to UMAP: the other
standard non-linear picture of the latents.

As in umap.py, the steps that touch the data are HIP kernels: the exact k-nearest-neighbour search (knn.hip), the
perplexity search (vsom_tsne_affinities) and two launches per iteration (vsom_tsne_repulsion, vsom_tsne_step, tsne.hip).
The host keeps the O(N k) graph (scipy, fp64) and the schedule.  The repulsion is EXACT: all N (N - 1) pairs every
iteration, no tree and no grid, which is what makes a fit bitwise reproducible.  Two components only.

The algorithm (sklearn 1.7, restated; the departures are marked):

1. Neighbours: k = min(N - 1, 63, floor(3 perplexity)) nearest OTHER rows of every row (vsom_umap_knn with k + 1, the row
   itself first and skipped; where k = N - 1, which a set of at most 64 rows can reach, the same search leave-one-out,
   vsom_knn_query, as vsom_umap_knn wants k + 1 < N).  cosine = 1 - <x,y> / (|x||y|); euclidean is the true distance, squared in f32 before use
   as sklearn squares it.
   Departure -- truncation: sklearn's barnes_hut takes floor(3 perplexity) neighbours whatever their number; the search
   here holds 63 (tsne-cuda ships the same kind of truncation).  Where 3 perplexity > 63 the bisection of step 2 matches
   the perplexity over 63 neighbours.  perplexity must be below k.
2. Conditional P (_binary_search_perplexity, fp64, one thread per row): beta = 1; up to 100 steps of
   e_j = exp(-d_j beta), S = sum e_j (1e-8 if 0), H = log S + beta sum_j d_j e_j / S; stop at |H - log perplexity| <= 1e-5;
   beta doubles (halves) while the other bound is infinite, else moves to the midpoint.  P_j|i = e_j / S.
3. Joint P (_joint_probabilities_nn, host): P = (C + C^T) / sum(C + C^T) with C the [N, N] sparse matrix of step 2, as
   sorted CSR in fp64, exactly symmetric; uploaded once.
4. Init: 'pca' = vit_som_amd.PCA(2).fit_transform(X) / std(first column) * 1e-4 (f32, on the host; sklearn's default,
   random_state None counting as 0 so that the default fit is reproducible); 'random' = 1e-4 *
   RandomState(random_state).standard_normal((N, 2)).astype(float32); a float32 [N, 2] device tensor is taken as given.
5. Descent (_gradient_descent), Y f32, update = 0 and gains = 1 (f32) at the start of EACH stage as sklearn has them:
   stage 1 = iterations [0, min(250, max_iter)) with P * early_exaggeration, momentum 0.5, progress window 250;
   stage 2 = up to max_iter with P, momentum 0.8, window n_iter_without_progress.  learning_rate 'auto' =
   max(N / early_exaggeration / 4, 50).  One iteration, from the iteration-start Y:
     q_ij = 1 / (1 + |y_i - y_j|^2) over ALL pairs, Z = sum_i sum_{j != i} q_ij          (vsom_tsne_repulsion: f32 terms,
     grad_i = 4 (sum_e P_e q_e (y_i - y_j) - sum_j q_ij^2 (y_i - y_j) / Z)                 fp64 across chunks; the edges
     gains += 0.2 where update * grad < 0, else *= 0.8; gains >= 0.01                     and the rest in fp64)
     update = momentum update - learning_rate gains grad;  Y += update                  (vsom_tsne_step)
   sklearn clamps q / Z at 2^-52 inside the gradient as well; here only inside the KL's logarithm (a difference below
   2^-52 per term).
6. Checks: after iteration i with (i + 1) % 50 == 0, and after a stage's last one, the host reads the step's record --
   the only synchronisations of a fit: KL = sum_e P_e log(P_e / (q_e / Z)) over the edges with the stage's (exaggerated) P
   as sklearn reports it, and |grad|.  A KL that is not below the stage's best for more than the window ends the stage,
   |grad| <= min_grad_norm likewise.  kl_divergence_ is the last KL read, n_iter_ the last iteration run.
   max_iter may be any positive integer (sklearn wants >= 250).

What is exact against sklearn: steps 2 and 3 to rounding, and the gradient and KL of step 5 at a given Y to the error of
the f32 repulsion terms.  What is not: the trajectory -- step 1's truncation, sklearn's Barnes-Hut approximation of the
repulsion (exact here), its float64 update and gains (float32 here) and the PCA behind the init differ, and t-SNE's
descent amplifies any of them; final KL and trustworthiness agree, the coordinates do not.
Not covered: three components, method='barnes_hut' / angle, more than 63 neighbours, precomputed distances, transform().
"""
import time
from dataclasses import dataclass

import numpy as np
import scipy.sparse
import torch

from . import ops
from .embedding_quality import EmbeddingQuality, embedding_quality
from .kmeans import _random_state
from .pca import PCA

METRICS = {"euclidean": ops.DIST_EUCLIDEAN, "cosine": ops.DIST_COSINE}
MACHINE_EPSILON = np.finfo(np.double).eps
EXPLORATION_ITERS = 250                                          # sklearn: _EXPLORATION_MAX_ITER, also stage 1's window
N_ITER_CHECK = 50
_EXACT = ("the repulsion here is exact: every pair is summed on the device in every iteration, there is no Barnes-Hut tree "
          "to choose or to tune")


def neighbour_count(N, perplexity):
    """Step 1's k: the neighbours (the row itself not counted) the affinities are taken over."""
    return int(min(N - 1, ops.TSNE_MAX_K, np.floor(3.0 * perplexity)))


def joint_probabilities(knn_idx, cond_P):
    """Step 3 -> P float64 CSR [N, N]: exactly symmetric, sorted indices, sums to 1.  knn_idx int64 [N, k] (the row itself
    not among them), cond_P float64 [N, k]."""
    knn_idx = np.asarray(knn_idx, dtype=np.int64)
    cond_P = np.asarray(cond_P, dtype=np.float64)
    N, k = knn_idx.shape
    if cond_P.shape != (N, k):
        raise ValueError(f"joint_probabilities: knn_idx {knn_idx.shape} and cond_P {cond_P.shape} must be the same [N, k]")
    C = scipy.sparse.csr_matrix((cond_P.ravel(), knn_idx.ravel(), np.arange(0, N * k + 1, k, dtype=np.int64)), shape=(N, N))
    P = (C + C.T).tocsr()
    P.sum_duplicates()
    P.sort_indices()
    P.data /= max(P.data.sum(), MACHINE_EPSILON)
    return P


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


class _Graph:
    """The joint P on the device and the buffers an iteration writes."""

    def __init__(self, P, device):
        def dev_t(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(device)
        N = P.shape[0]
        self.N = N
        self.indptr, self.indices = dev_t(P.indptr.astype(np.int64)), dev_t(P.indices.astype(np.int64))
        self.data = dev_t(P.data.astype(np.float64))
        self.rep = torch.empty(N, 2, dtype=torch.float64, device=device)
        self.sumq = torch.empty(N, dtype=torch.float64, device=device)
        self.zpart = torch.empty(ops.tsne_repulsion_parts(N), dtype=torch.float64, device=device)
        self.part = torch.zeros(ops.tsne_step_parts(N), dtype=torch.float64, device=device)


def read_record(part):
    """The step's record -> (KL, |grad|): the per-block pairs added on the host (one copy: a synchronisation)."""
    rec = part.cpu().numpy().reshape(-1, 2)
    return float(rec[:, 0].sum()), float(np.sqrt(rec[:, 1].sum()))


def descend(graph, Y, update, gains, begin, end, stage_end, exaggeration, momentum, learning_rate, window=EXPLORATION_ITERS,
            min_grad_norm=1e-7, progress=None):
    """Iterations [begin, end) of a stage that ends at stage_end (step 5 and 6).  Y f32 [N, 2] is the state with update and
    gains (f32 [N, 2], changed in place); -> (Y after the last iteration run, that iteration's index, stopped early).
    progress: the dict a stage's calls share (best KL so far, its iteration, the last KL and |grad| read); cutting a
    stage into several calls changes no bit of Y, update or gains.  Y's storage is one of the two buffers the iterations
    alternate between: the tensor passed in is overwritten."""
    if progress is None:
        progress = {}
    progress.setdefault("best_error", np.finfo(float).max)
    progress.setdefault("best_iter", begin)
    cur, nxt = Y, torch.empty_like(Y)
    last = begin - 1
    for i in range(begin, end):
        check = (i + 1) % N_ITER_CHECK == 0
        record = check or i == stage_end - 1
        ops.tsne_repulsion(cur, graph.rep, graph.sumq, graph.zpart)
        ops.tsne_step(graph.indptr, graph.indices, graph.data, cur, nxt, update, gains, graph.rep, graph.zpart, exaggeration,
                      momentum, learning_rate, graph.part, record=record)
        cur, nxt = nxt, cur
        last = i
        if record:
            progress["kl"], progress["grad_norm"] = read_record(graph.part)
        if check:
            if progress["kl"] < progress["best_error"]:
                progress["best_error"], progress["best_iter"] = progress["kl"], i
            elif i - progress["best_iter"] > window:
                return cur, last, True
            if progress["grad_norm"] <= min_grad_norm:
                return cur, last, True
    return cur, last, False


class TSNE:
    """sklearn.manifold.TSNE for a float32 [N, D] device tensor, with sklearn's parameter names and defaults (the subset
    listed; module docstring for the algorithm and its departures).  After ``fit``: ``embedding_`` float32 [N, 2] on the
    device, ``kl_divergence_``, ``n_iter_``, ``n_features_in_``, ``learning_rate_``."""

    def __init__(self, n_components=2, perplexity=30.0, early_exaggeration=12.0, learning_rate="auto", max_iter=1000,
                 n_iter_without_progress=300, min_grad_norm=1e-7, metric="euclidean", init="pca", random_state=None,
                 **unsupported):
        method = unsupported.pop("method", "exact")
        if method != "exact":
            raise ValueError(f"TSNE: method={method!r} is not available; {_EXACT}")
        if "angle" in unsupported:
            raise ValueError(f"TSNE: angle is not available; {_EXACT}")
        if unsupported:
            raise TypeError(f"TSNE: unexpected keyword arguments {sorted(unsupported)}")
        self.n_components, self.perplexity, self.early_exaggeration = n_components, perplexity, early_exaggeration
        self.learning_rate, self.max_iter, self.n_iter_without_progress = learning_rate, max_iter, n_iter_without_progress
        self.min_grad_norm, self.metric, self.init, self.random_state = min_grad_norm, metric, init, random_state

    def _validate(self, N):
        """sklearn's parameter errors and this implementation's limits, for a set of N rows -> k of step 1."""
        if self.n_components != 2:
            raise ValueError(f"TSNE: n_components must be 2, got {self.n_components!r}: a third component changes the degrees "
                             f"of freedom and with them the kernel q = 1 / (1 + d^2) the device repulsion is written for")
        if not isinstance(self.metric, str) or self.metric not in METRICS:
            raise ValueError(f"TSNE: metric must be one of {sorted(METRICS)}, got {self.metric!r}")
        if not (isinstance(self.perplexity, (int, float, np.floating, np.integer)) and self.perplexity > 0):
            raise ValueError(f"TSNE: perplexity must be a positive number, got {self.perplexity!r}")
        if self.perplexity >= N:
            raise ValueError(f"TSNE: perplexity ({self.perplexity}) must be less than n_samples ({N})")
        k = neighbour_count(N, self.perplexity)
        if k < 1 or not self.perplexity < k:
            raise ValueError(f"TSNE: perplexity ({self.perplexity}) must be below the number of neighbours k = min(n_samples - 1, "
                             f"{ops.TSNE_MAX_K}, floor(3 perplexity)) = {k}: the search keeps at most {ops.TSNE_MAX_K} neighbours "
                             f"of a row")
        if not self.early_exaggeration >= 1.0:
            raise ValueError(f"TSNE: early_exaggeration must be at least 1, got {self.early_exaggeration!r}")
        if not (self.learning_rate == "auto" or (not isinstance(self.learning_rate, str) and self.learning_rate > 0)):
            raise ValueError(f"TSNE: learning_rate must be 'auto' or a positive number, got {self.learning_rate!r}")
        if not _is_int(self.max_iter) or self.max_iter < 1:
            raise ValueError(f"TSNE: max_iter must be a positive integer, got {self.max_iter!r}")
        if not _is_int(self.n_iter_without_progress) or self.n_iter_without_progress < 0:
            raise ValueError(f"TSNE: n_iter_without_progress must be a non-negative integer, got {self.n_iter_without_progress!r}")
        if not self.min_grad_norm >= 0:
            raise ValueError("TSNE: min_grad_norm must not be negative")
        if isinstance(self.init, str) and self.init not in ("pca", "random"):
            raise ValueError(f"TSNE: init must be 'pca', 'random' or a float32 [N, 2] device tensor, got {self.init!r}")
        return k

    @staticmethod
    def _check_x(X):
        if not isinstance(X, torch.Tensor) or X.dim() != 2:
            raise ValueError("TSNE: X must be a float32 [N, D] tensor on the GPU")
        if X.shape[0] < 2 or X.shape[1] < 1:
            raise ValueError(f"TSNE: X of shape {tuple(X.shape)} needs at least two rows and one column")
        return X

    @staticmethod
    def _check_device(X):
        if X.dtype != torch.float32:
            raise ValueError(f"TSNE: X must be float32, got {X.dtype}")
        if not X.is_cuda:
            raise ValueError("TSNE: X must be on the GPU (there is no CPU path)")
        if not X.is_contiguous():
            raise ValueError("TSNE: X must be contiguous")

    def _initial(self, X):
        N = X.shape[0]
        if not isinstance(self.init, str):
            init = self.init
            if not isinstance(init, torch.Tensor) or tuple(init.shape) != (N, 2) or init.dtype != torch.float32 or not init.is_cuda:
                raise ValueError(f"TSNE: init must be 'pca', 'random' or a float32 device tensor of shape {(N, 2)}")
            return init.detach().clone().contiguous()
        if self.init == "random":
            emb = 1e-4 * _random_state(self.random_state).standard_normal(size=(N, 2)).astype(np.float32)
        else:
            if X.shape[1] < 2:
                raise ValueError("TSNE: init='pca' needs at least two columns")
            seed = 0 if self.random_state is None else self.random_state
            emb = PCA(n_components=2, random_state=seed).fit_transform(X).cpu().numpy().astype(np.float32)
            emb = emb / np.std(emb[:, 0]) * 1e-4
        return torch.from_numpy(np.ascontiguousarray(emb.astype(np.float32))).to(X.device)

    def affinities(self, X, k):
        """Steps 1-3 -> the joint P (scipy CSR, fp64).  Keeps ``_knn_indices`` / ``_knn_dists`` (the k neighbours, the row
        itself left out) and ``_betas`` on the host."""
        N, dev = X.shape[0], X.device
        first = 1 if k + 1 < N else 0
        idx = torch.empty(N, k + first, dtype=torch.int64, device=dev)
        dist = torch.empty(N, k + first, dtype=torch.float32, device=dev)
        if first:
            ops.umap_knn(X, k + 1, METRICS[self.metric], idx, dist)
        else:
            # k = N - 1 (a set of at most 64 rows): every other row is a neighbour, and vsom_umap_knn wants k + 1 < N.
            # The same search, leave-one-out: no self slot to skip.
            ops.knn_query(X, X, k, METRICS[self.metric], idx, dist, exclude=torch.arange(N, dtype=torch.int64, device=dev))
        cond = torch.empty(N, k, dtype=torch.float64, device=dev)
        beta = torch.empty(N, dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        ops.tsne_affinities(dist, self.perplexity, cond, beta, status, knn_idx=idx, first=first, square=self.metric == "euclidean")
        refused = int(status.item())
        if refused:
            raise ValueError(f"TSNE: {refused} rows have no complete list of {k} neighbours at a finite distance: X holds NaN or "
                             f"infinity, or a row's squared norm overflows float32")
        self._knn_indices, self._knn_dists = idx[:, first:].cpu().numpy(), dist[:, first:].cpu().numpy()
        self._betas = beta.cpu().numpy()
        return joint_probabilities(self._knn_indices, cond.cpu().numpy())

    def fit(self, X):
        X = self._check_x(X)
        k = self._validate(X.shape[0])
        self._check_device(X)
        N = X.shape[0]
        P = self.affinities(X, k)
        Y = self._initial(X)
        graph = _Graph(P, X.device)
        lr = max(N / float(self.early_exaggeration) / 4.0, 50.0) if self.learning_rate == "auto" else float(self.learning_rate)
        update, gains = torch.zeros_like(Y), torch.ones_like(Y)
        stage1 = min(EXPLORATION_ITERS, self.max_iter)
        progress = {}
        Y, last, _ = descend(graph, Y, update, gains, 0, stage1, stage1, float(self.early_exaggeration), 0.5, lr,
                             EXPLORATION_ITERS, self.min_grad_norm, progress)
        if self.max_iter > EXPLORATION_ITERS:
            update.zero_()
            gains.fill_(1.0)
            progress = {}                                    # last + 1 <= 250 < max_iter: stage 2 runs at least once
            Y, last, _ = descend(graph, Y, update, gains, last + 1, self.max_iter, self.max_iter, 1.0, 0.8, lr,
                                 self.n_iter_without_progress, self.min_grad_norm, progress)
        self.embedding_ = Y
        self.kl_divergence_ = progress["kl"]
        self.n_iter_ = last
        self.n_features_in_ = X.shape[1]
        self.learning_rate_ = lr
        return self

    def fit_transform(self, X):
        return self.fit(X).embedding_


# ------------------------------------------------------------------------------------ evaluation entries
_TSNE_SAVEFIG = dict(bbox_inches="tight", pad_inches=0, transparent=False, dpi=400)


def _tsne_embed(X, perplexity):
    """-> the fitted TSNE(perplexity, metric='cosine', random_state=42) and its embedding (a device tensor)."""
    reducer = TSNE(perplexity=perplexity, metric="cosine", random_state=42)
    return reducer, reducer.fit_transform(X)


@torch.no_grad()
def visualize_tsne_progression(model, config, dataloader, epoch=0, output_dir="experiments/plots/vit_som/tsne", perplexity=30.0):
    """visualize_umap_progression with t-SNE (no counterpart in the reference): TSNE(perplexity, metric='cosine',
    random_state=42) of model.get_latent_representation(x) over the whole set, fitted on the device, drawn with the same
    scatter plot into output_dir/som_tsne_epoch_{epoch}.png (rank 0 only; skipped with a warning when matplotlib is
    missing).  With model.world_size > 1 every rank gathers all rows and runs the same deterministic fit.  Returns
    (embedding [N, 2] float32, labels [N]) as host arrays."""
    from . import evaluation as E                         # its loader pass and model adapter; evaluation imports this module
    who = "visualize_tsne_progression"
    arch = E._Arch(model, config, who)
    X, y = E._whole_set(arch, dataloader, model.get_latent_representation, labels=True, shape=arch.images)
    embedding = _tsne_embed(X, perplexity)[1].cpu().numpy()
    all_labels = y.cpu().numpy()
    if E._rank(model) == 0:
        E._save_scatter(who, output_dir, f"som_tsne_epoch_{epoch}.png", embedding, all_labels, **_TSNE_SAVEFIG)
    return embedding, all_labels


@dataclass
class TSNEQualityReport(EmbeddingQuality):
    """evaluate_tsne_quality's result: EmbeddingQuality of the t-SNE embedding against the latents, the embedding itself
    and how the fit ended."""
    embedding: np.ndarray = None         # float32 [N, 2], host
    kl_divergence: float = float("nan")  # TSNE.kl_divergence_
    n_iter: int = 0                      # TSNE.n_iter_
    inference_time: float = 0.0


@torch.no_grad()
def evaluate_tsne_quality(model, config, dataloader, n_neighbors=15, perplexity=30.0):
    """Trustworthiness and continuity (embedding_quality.py) of the picture visualize_tsne_progression draws ->
    TSNEQualityReport.  Latents as evaluate_embedding_quality takes them (get_latent_representation for vit_som, x_encoded
    for desom), TSNE(perplexity, metric='cosine', random_state=42); the latents are compared by cosine distance, the
    embedding by euclidean, ties take the lowest rank.  With model.world_size > 1 every rank gathers the rows and computes
    the same numbers."""
    from . import evaluation as E
    arch = E._Arch(model, config, "evaluate_tsne_quality").require("latent")
    start = time.time()
    X, _ = E._whole_set(arch, dataloader, arch.latent, labels=True)
    reducer, embedding = _tsne_embed(X, perplexity)
    q = embedding_quality(X, embedding.contiguous(), n_neighbors=n_neighbors, metric="cosine")
    report = TSNEQualityReport(**vars(q), embedding=embedding.cpu().numpy(), kl_divergence=float(reducer.kl_divergence_),
                               n_iter=int(reducer.n_iter_))
    report.inference_time = time.time() - start
    print(f"t-SNE Trustworthiness: {report.trustworthiness:.4f}, Continuity: {report.continuity:.4f} (k={report.n_neighbors}, "
          f"{report.n_samples} samples), KL: {report.kl_divergence:.4f} after {report.n_iter + 1} iterations, "
          f"Inference Time: {report.inference_time:.3f}")
    return report
