"""On-device evaluation behind the reference's tools/evaluation.py entry points, and what this project adds to them.
The model forward runs on the HIP kernels; what an entry folds or collects stays on the device, and the host sees a table
or a report at the end.  One rule holds for every entry: NO HOST SYNCHRONISATION INSIDE A LOADER LOOP.

Scaffolding, each written once:
  _Arch         what a vit_som or a desom model is fed and what is read from it; the one unsupported-model error
  _Arch.batches the loader loop: model.eval(), the batch moved to the model's device and shaped, labels flat int64
  _whole_set    a reader's rows of every batch (copied), concatenated, all-gathered over the ranks (rank 0's first)
  _rank_shift   where this rank's sample ordinals start among all ranks'
  plots.py      the drawing, from host arrays

Entries, by what they read from the model (every entry runs with grad mode off; with model.world_size > 1 every rank
returns the whole set's result; figures are drawn by rank 0):
  predict(), images for every arch     evaluate_clustering (BMUs -> `vsom_contingency`), evaluate_classification (logits),
                                       evaluate_map_clusters (the BMU's cluster of units; defined in agglomerative.py next
                                       to its estimator, reachable from here)
  predict(), the arch's own shape      visualize_label_heatmap (`vsom_last_label`), evaluate_map_quality / visualize_hit_map
                                       (the SOM layer's buffers -> `vsom_map_stats`)
  k-means feature, model(x)[1]         evaluate_kmeans (kmeans.py)
  get_latent_representation, images    visualize_umap_progression (umap.py), visualize_tsne_progression (defined in
                                       tsne.py next to its estimator, reachable from here)
  latent                               visualize_umap_map, evaluate_embedding_quality (embedding_quality.py),
                                       visualize_pca_map (pca.py), evaluate_knn (knn.py), evaluate_linear_probe
                                       (defined in linear_probe.py next to its estimator, reachable from here),
                                       evaluate_tsne_quality (tsne.py, likewise), evaluate_gmm (gmm.py, likewise)
  SOM input                            evaluate_dbscan / visualize_dbscan (defined in dbscan.py next to their estimator,
                                       reachable from here), evaluate_hdbscan / visualize_hdbscan (hdbscan.py, likewise)
  the encoder's saved qkv              evaluate_attention / visualize_attention_rollout / visualize_attention_map (defined in
                                       attention_rollout.py next to the chain, reachable from here)
  SOM input and BMU                    evaluate_silhouette / visualize_silhouette_map (silhouette.py),
                                       evaluate_latent_spectrum, init_som_from_data, fit_som_batch (SOMLayer.fit_batch)
  the prototypes only, no data         visualize_decoded_prototypes / decoded_prototype_canvas / decode_prototype
                                       (`vsom_proto_mosaic`), umatrix / visualize_umatrix (`vsom_umatrix`), map_neighbourhood,
                                       visualize_map_clusters (agglomerative.py)
Host arithmetic on a table: purity_from_table, nmi_from_table, classification_from_table, calculate_purity."""
import os
import time
from dataclasses import dataclass

import numpy as np
import torch

from . import ops
from .embedding_quality import EmbeddingQuality, embedding_quality, subset_scores
from .kmeans import KMeans
from .knn import KNNClassifier
from .linear_probe import LinearProbeReport, evaluate_linear_probe, linear_probe_report  # noqa: F401  (the entry lives with its estimator)
from .gmm import GMMReport, evaluate_gmm  # noqa: F401  (the entry lives with its estimator)
from .agglomerative import MapClustersReport, evaluate_map_clusters, visualize_map_clusters  # noqa: F401  (likewise)
from .dbscan import DBSCANReport, evaluate_dbscan, visualize_dbscan  # noqa: F401  (likewise)
from .hdbscan import HDBSCANReport, evaluate_hdbscan, visualize_hdbscan  # noqa: F401  (likewise)
from .spectral import SpectralReport, evaluate_spectral, visualize_spectral_map  # noqa: F401  (likewise)
from .attention_rollout import AttentionReport, evaluate_attention, visualize_attention_map, visualize_attention_rollout  # noqa: F401  (likewise)
from .tsne import TSNEQualityReport, evaluate_tsne_quality, visualize_tsne_progression  # noqa: F401  (the entries live with their estimator)
from .plots import _draw_grid, _draw_map, _pyplot, _save_scatter, _umap_scatter, draw_decoded_prototypes, draw_label_heatmap  # noqa: F401
from .silhouette import cluster_silhouette
from .umap import UMAP


class _Table:
    def __init__(self, na, nb, device):
        self.table = torch.zeros(na, nb, dtype=torch.int64, device=device)
        self.bad = torch.zeros(1, dtype=torch.int32, device=device)

    def add(self, a, b):
        ops.contingency(a.contiguous().view(-1), b.contiguous().view(-1).long(), self.table, self.bad)

    def grow_columns(self, nb):
        """Widen the table to `nb` columns (labels are not known in advance for the clustering configs)."""
        if nb > self.table.shape[1]:
            t = torch.zeros(self.table.shape[0], nb, dtype=torch.int64, device=self.table.device)
            t[:, :self.table.shape[1]] = self.table
            self.table = t

    def numpy(self, world_size=1):
        """The table on the host -- summed over the ranks first when every rank folded its own shard of the data
        (one all-reduce of the integer table: every rank then reports the metrics of the WHOLE set)."""
        if world_size > 1:
            import torch.distributed as dist
            both = torch.cat([self.table.view(-1), self.bad.view(-1).long()])
            dist.all_reduce(both)
            self.table, self.bad = both[:-1].view_as(self.table), both[-1:].int()
        nbad = int(self.bad.item())
        if nbad:
            raise ValueError(f"{nbad} label/prediction values fell outside the contingency table "
                             f"({self.table.shape[0]} x {self.table.shape[1]}); pass num_labels= for larger label sets")
        return self.table.cpu().numpy()


def purity_from_table(w: np.ndarray) -> float:
    """evaluation.py:142-151: majority-vote label per predicted cluster, then accuracy."""
    n = w.sum()
    return float(w.max(axis=1).sum() / n) if n else float("nan")


def nmi_from_table(w: np.ndarray) -> float:
    """sklearn.metrics.normalized_mutual_info_score(average_method='arithmetic') from a contingency table."""
    w = w.astype(np.float64)
    n = w.sum()
    a, b = w.sum(axis=1), w.sum(axis=0)
    na, nb = int((a > 0).sum()), int((b > 0).sum())
    if (na == 1 and nb == 1) or (na == 0 and nb == 0):
        return 1.0
    nz = w > 0
    outer = np.outer(a, b)
    mi = float((w[nz] / n * (np.log(w[nz]) - np.log(n) - (np.log(outer[nz]) - 2 * np.log(n)))).sum())
    mi = max(mi, 0.0)

    def ent(c):
        c = c[c > 0]
        return float(-(c / n * (np.log(c) - np.log(n))).sum())
    norm = max(0.5 * (ent(a) + ent(b)), np.finfo(np.float64).eps)
    return mi / norm


def classification_from_table(cm: np.ndarray):
    """accuracy + sklearn precision_recall_fscore_support(average='macro', zero_division=nan) from the
    confusion matrix cm[true, pred] over labels = union(y_true, y_pred)."""
    cm = cm.astype(np.float64)
    present = (cm.sum(axis=0) + cm.sum(axis=1)) > 0
    cm = cm[present][:, present]
    tp = np.diag(cm)
    pred_sum, true_sum = cm.sum(axis=0), cm.sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        precision = np.where(pred_sum > 0, tp / pred_sum, np.nan)      # zero_division=nan: excluded from the macro mean
        recall = np.where(true_sum > 0, tp / true_sum, np.nan)
        f1 = 2 * tp / (true_sum + pred_sum)                            # sklearn: (1+b^2) tp / (b^2 true + pred), never 0/0 here
    acc = float(tp.sum() / cm.sum()) if cm.sum() else float("nan")
    return acc, float(np.nanmean(precision)), float(np.nanmean(recall)), float(np.nanmean(f1))


def calculate_purity(y_trues, y_preds):
    """evaluation.py:130-151 (same signature); the contingency table is built on the device."""
    dev = y_preds.device if isinstance(y_preds, torch.Tensor) and y_preds.is_cuda else torch.device("cuda", torch.cuda.current_device())
    yt = torch.as_tensor(np.asarray(y_trues) if not isinstance(y_trues, torch.Tensor) else y_trues).to(dev).long().view(-1)
    yp = torch.as_tensor(np.asarray(y_preds) if not isinstance(y_preds, torch.Tensor) else y_preds).to(dev).long().view(-1)
    assert yp.numel() == yt.numel(), f"y_preds ({yp.numel()}) and y_trues ({yt.numel()}) must be the same size"
    D = int(max(int(yp.max()), int(yt.max())) + 1)
    t = _Table(D, D, dev)
    t.add(yp, yt)
    return purity_from_table(t.numpy())


def _world(model):
    return int(getattr(model, "world_size", 1))


def _rank(model):
    return int(getattr(model, "rank", 0))


def _label_count(config, num_labels, at_least_256):
    """num_labels when given.  Else data.num_classes: raised to 256 (at_least_256, the tables of the clustering
    entries), or 256 only when the config has none (the kNN probe, whose vote kernel takes at most 1024 classes)."""
    if num_labels:
        return int(num_labels)
    n = int(config["data"].get("num_classes", 0))
    return max(n, 256) if at_least_256 or n <= 0 else n


class _Arch:
    """What a vit_som or a desom model is fed and what is read from it, for the entry `who`.  The only place in this
    module that knows the architectures.  Shapes take a batch on the device; readers take the shaped batch and may return
    views of buffers that the model's next forward overwrites."""
    _PROBES = {("vit_som", "latent"): "get_latent_representation", ("vit_som", "som_input"): "_som_input",
               ("desom", "latent"): "autoencoder", ("desom", "som_input"): "autoencoder"}

    def __init__(self, model, config, who):
        d = config["data"]
        self.model, self.who = model, who
        self.C, self.S = d["num_channels"], d["input_size"]
        self.name = config.get("hyperparameters", {}).get("model_arch")

    @property
    def device(self):
        return self.model.arena.device

    def require(self, reader=None):
        """Refuse, before any batch is read, a model_arch that is neither vit_som nor desom and a model that lacks what
        `reader` ("latent", "som_input") reads.  Returns self."""
        probe = self._PROBES.get((self.name, reader))
        if self.name not in ("vit_som", "desom") or (probe is not None and not hasattr(self.model, probe)):
            raise ValueError(f"{self.who}: needs a vit_som or a desom model; got {type(self.model).__name__} with "
                             f"model_arch {self.name!r}")
        return self

    @staticmethod
    def is_vit_som(config):
        """For an entry the reference has for vit_som alone, asked before anything of the model is touched."""
        return config["hyperparameters"]["model_arch"] == "vit_som"

    # ---- shapes
    def images(self, x):
        return x.reshape(-1, self.C, self.S, self.S)

    @staticmethod
    def flat(x):
        return x.reshape(x.shape[0], -1)

    def own(self, x):
        """The shape the architecture's forward takes (after require())."""
        return self.images(x) if self.name == "vit_som" else self.flat(x)

    # ---- readers
    def latent(self, x):
        """[B, D] features: get_latent_representation for vit_som, x_encoded for desom (require("latent"))."""
        return self.model.get_latent_representation(x) if self.name == "vit_som" else self.model(x)[1]

    def som_input(self, x):
        """(the rows the SOM layer was given, the unit each of them won) (require("som_input")).  vit_som: predict()
        leaves the BMUs in the SOM layer's buffers and the encoder output in the ViT's.  desom: forward() returns both."""
        m = self.model
        if self.name == "vit_som":
            bmu, _ = m.predict(x)
            return m._som_input(m.vit._buffers_for(x.shape[0], x.device)), bmu
        _, z, _, bmu = m(x)
        return z, bmu

    def kmeans_feature(self, x):
        """The SECOND output of forward(): recon_img for vit_som (the reference calls it x_encoded, vit_som.py:67-78), the
        encoder latent for desom (desom.py:50-54)."""
        return self.model(x)[1]

    # ---- the loader loop
    def batches(self, loader, shape, labels=True):
        """THE loop over a data loader: the model in eval mode, every batch moved to its device; yields (shape(x), y) with
        y flat int64 on the device, or None -- the loader's labels untouched -- when labels is False.  Grad mode is the
        caller's business (a generator cannot hold a no_grad across its yields): every entry is @torch.no_grad()."""
        self.model.eval()
        dev = self.device
        for x, y in loader:
            x = shape(x.to(dev, non_blocking=True))
            yield x, (y.to(dev, non_blocking=True).reshape(-1).long().contiguous() if labels else None)


def _rows(arch, loader, read, labels, shape=None, what="loader"):
    """This rank's (X [N, D] float32, second [N] int64) over the loader, on the device.  labels True: read(x) gives the
    rows and second is the labels.  labels False: read(x) gives (rows, units) and the labels are not touched.  What a
    reader returns is copied: it may be a view of a buffer the next batch overwrites."""
    first, second = [], []
    batches = arch.batches(loader, shape or arch.own, labels)
    for x, y in batches:
        z, other = (read(x), None) if labels else read(x)
        first.append(z.reshape(z.shape[0], -1).float().clone())
        second.append(y if labels else other.reshape(-1).long().clone())
    if not first:
        raise ValueError(f"{arch.who}: the {what} is empty")
    return torch.cat(first).contiguous(), torch.cat(second).contiguous()


def _whole_set(arch, loader, read, labels, shape=None):
    """_rows over the whole set on every rank: with model.world_size > 1 every rank gathers all rows, rank 0's first."""
    X, second = _rows(arch, loader, read, labels, shape)
    world = _world(arch.model)
    if world > 1:
        X, second = _gather_rows(X, world).contiguous(), _gather_rows(second, world).contiguous()
    return X, second


def _rank_shift(model, seen, who):
    """-> (before, total): the samples the ranks before this one have seen, and all ranks' together; (0, seen) in a single
    process.  Ordinals travel in 31 bits of a packed word: 2^31 samples or more raise ValueError."""
    world = _world(model)
    if world == 1:
        return 0, seen
    import torch.distributed as dist
    dev = model.arena.device
    counts = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(world)]
    dist.all_gather(counts, torch.tensor([seen], dtype=torch.int64, device=dev))
    counts = [int(c) for c in counts]
    if sum(counts) >= 2 ** 31:
        raise ValueError(f"{who}: more than 2^31 - 1 samples")
    return sum(counts[:_rank(model)]), sum(counts)


@torch.no_grad()
def evaluate_clustering(model, config, dataloader, num_labels=None):
    """evaluation.py:18-52 -> (purity, nmi, inference_time) from the model's native BMU assignments.  No host
    synchronisation inside the loop: labels outside [0, num_labels) are counted on the device and reported once at the
    end (num_labels defaults to max(data.num_classes, 256)).  With model.world_size > 1 every rank folds its shard and
    the tables are summed, so all ranks return the metrics of the whole set."""
    arch = _Arch(model, config, "evaluate_clustering")
    table = _Table(model.som_layer.n_prototypes, _label_count(config, num_labels, True), arch.device)
    start = time.time()
    batches = arch.batches(dataloader, arch.images)
    for x, y in batches:
        bmu, _ = model.predict(x)
        table.add(bmu, y)
    w = table.numpy(_world(model))
    purity, nmi = purity_from_table(w), nmi_from_table(w)
    inference_time = time.time() - start
    print(f"Purity: {purity:.3f}, NMI: {nmi:.3f}, Inference Time: {inference_time:.3f}")
    return purity, nmi, inference_time


def _gather_rows(t, world_size):
    """Every rank's rows, concatenated in rank order (ranks may hold different row counts)."""
    import torch.distributed as dist
    n = torch.tensor([t.shape[0]], dtype=torch.int64, device=t.device)
    sizes = [torch.zeros_like(n) for _ in range(world_size)]
    dist.all_gather(sizes, n)
    sizes = [int(s) for s in sizes]
    pad = torch.zeros((max(sizes),) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    pad[:t.shape[0]] = t
    parts = [torch.empty_like(pad) for _ in range(world_size)]
    dist.all_gather(parts, pad)
    return torch.cat([p[:s] for p, s in zip(parts, sizes)])


@torch.no_grad()
def evaluate_kmeans(model, config, dataloader, num_labels=None):
    """evaluation.py:54-91 -> (purity, nmi, inference_time) of KMeans(n_clusters=len(unique(labels)), random_state=0,
    n_init=10) on the model's outputs.  The features are what the reference clusters: for vit_som the SECOND output of
    ViTSOM.forward, i.e. recon_img flattened to C*H*W (the reference calls it x_encoded, vit_som.py:67-78), for desom
    the encoder latent x_encoded (desom.py:50-54).  Features and labels stay on the device; the fit is the HIP k-means
    (kmeans.py).  Labels must lie in [0, num_labels) (default max(data.num_classes, 256)).  With model.world_size > 1
    every rank gathers the whole set and runs the same deterministic fit, so all ranks report the whole set's metrics."""
    arch = _Arch(model, config, "evaluate_kmeans").require()
    dev, L = arch.device, _label_count(config, num_labels, True)
    start = time.time()
    X, y = _whole_set(arch, dataloader, arch.kmeans_feature, labels=True)
    hist = _Table(1, L, dev)                               # len(np.unique(y_trues)), labels range-checked
    hist.add(torch.zeros_like(y), y)
    n_clusters = int((hist.numpy() > 0).sum())
    km = KMeans(n_clusters=n_clusters, random_state=0, n_init=10)
    table = _Table(n_clusters, L, dev)
    table.add(km.fit_predict(X), y)
    w = table.numpy()
    purity, nmi = purity_from_table(w), nmi_from_table(w)
    inference_time = time.time() - start
    print(f"Purity (KMeans): {purity:.3f}, NMI (KMeans): {nmi:.3f}, Inference Time: {inference_time:.3f}")
    return purity, nmi, inference_time


def _umap_fit_subset(N, fit_rows):
    """The rows _umap_embed fits on, as a boolean mask [N]; None when it fits all of them."""
    if fit_rows is None or N <= int(fit_rows):
        return None
    chosen = np.zeros(N, dtype=bool)
    chosen[np.random.RandomState(42).permutation(N)[:int(fit_rows)]] = True
    return chosen


def _umap_embed(X, fit_rows=None):
    """-> (the fitted UMAP(n_neighbors=15, min_dist=0.1, metric='cosine', random_state=42), the embedding of every row
    of X as a device tensor).  fit_rows None, or not below the row count: one fit of all rows.  Otherwise the fit sees a
    fixed subset -- the first fit_rows entries of RandomState(42).permutation(N), sorted -- and the other rows are
    placed into it by transform(); the rows come back in their original order."""
    reducer = UMAP(n_neighbors=15, min_dist=0.1, metric="cosine", random_state=42)
    N = X.shape[0]
    chosen = _umap_fit_subset(N, fit_rows)
    if chosen is None:
        return reducer, reducer.fit_transform(X)
    sub = torch.from_numpy(np.flatnonzero(chosen)).to(X.device)
    rest = torch.from_numpy(np.flatnonzero(~chosen)).to(X.device)
    fitted = reducer.fit_transform(X.index_select(0, sub))
    embedding = torch.empty(N, fitted.shape[1], dtype=torch.float32, device=X.device)
    embedding[sub] = fitted
    embedding[rest] = reducer.transform(X.index_select(0, rest))
    return reducer, embedding


_UMAP_SAVEFIG = dict(bbox_inches="tight", pad_inches=0, transparent=False, dpi=400)


@torch.no_grad()
def visualize_umap_progression(model, config, dataloader, epoch=0, output_dir="experiments/plots/vit_som/umap", fit_rows=None):
    """evaluation.py:267-323: UMAP(n_neighbors=15, min_dist=0.1, metric='cosine', random_state=42) of
    model.get_latent_representation(x) over the whole set, fitted on the device (umap.py), drawn as the reference's
    scatter plot into output_dir/som_umap_epoch_{epoch}.png (rank 0 only; skipped with a warning when matplotlib is
    missing).  With model.world_size > 1 every rank gathers all rows and runs the same deterministic fit.  fit_rows (not in
    the reference): fit on a fixed subset of that many rows and transform() the others into it (_umap_embed), for sets
    whose host-side graph and spectral initialisation would take too long.  Returns (embedding [N, 2] float32, labels [N])
    as host arrays (the reference returns None)."""
    who = "visualize_umap_progression"
    arch = _Arch(model, config, who)
    X, y = _whole_set(arch, dataloader, model.get_latent_representation, labels=True, shape=arch.images)
    embedding = _umap_embed(X, fit_rows)[1].cpu().numpy()
    all_labels = y.cpu().numpy()
    if _rank(model) == 0:
        _save_scatter(who, output_dir, f"som_umap_epoch_{epoch}.png", embedding, all_labels, **_UMAP_SAVEFIG)
    return embedding, all_labels


@torch.no_grad()
def visualize_umap_map(model, config, dataloader, epoch=0, output_dir="experiments/plots/vit_som/umap", fit_rows=None):
    """The map in data space (no counterpart in the reference): the embedding of visualize_umap_progression (same
    latents, same UMAP, same fit_rows) with the SOM's K prototypes placed INTO it by UMAP.transform -- they live in the
    space of the latents -- and the unit grid drawn over the scatter plot: a marker per unit and a line between units the
    layer's topology makes adjacent (umatrix's neighbour table, square and hexagonal) ->
    output_dir/som_umap_map_epoch_{epoch}.png (rank 0 only; skipped with a warning when matplotlib is missing).  Latents:
    model.get_latent_representation(x) for vit_som, x_encoded for desom, as evaluate_knn chooses them; any other model
    raises ValueError.  Returns (embedding [N, 2] float32, labels [N], prototype_embedding [K, 2] float32) as host arrays."""
    who = "visualize_umap_map"
    arch = _Arch(model, config, who).require("latent")
    X, y = _whole_set(arch, dataloader, arch.latent, labels=True)
    reducer, embedding = _umap_embed(X, fit_rows)
    protos = reducer.transform(model.som_layer.prototypes.detach().float().contiguous()).cpu().numpy()
    embedding, all_labels = embedding.cpu().numpy(), y.cpu().numpy()
    nbr_idx = umatrix(model)[1]
    if _rank(model) == 0:
        _save_scatter(who, output_dir, f"som_umap_map_epoch_{epoch}.png", embedding, all_labels, grid=(protos, nbr_idx),
                      **_UMAP_SAVEFIG)
    return embedding, all_labels, protos


@dataclass
class EmbeddingQualityReport(EmbeddingQuality):
    """evaluate_embedding_quality's result: EmbeddingQuality of the UMAP embedding against the latents, the embedding
    itself, and with fit_rows the two measures over the fitted and over the transformed rows alone."""
    embedding: np.ndarray = None         # float32 [N, 2], host
    fitted_rows: np.ndarray = None       # bool [N]: the rows the UMAP was fitted on; None when it was fitted on all
    fitted: tuple = None                 # (trustworthiness, continuity) over the fitted rows
    transformed: tuple = None            # ... over the rows placed by transform()
    inference_time: float = 0.0


@torch.no_grad()
def evaluate_embedding_quality(model, config, dataloader, n_neighbors=15, fit_rows=None):
    """Trustworthiness and continuity (embedding_quality.py) of the picture visualize_umap_map draws -> EmbeddingQualityReport.
    Same latents (_Arch.latent: get_latent_representation for vit_som, x_encoded for desom), same UMAP(n_neighbors=15,
    min_dist=0.1, metric='cosine', random_state=42) and same fit_rows subset; the latents are compared by cosine distance,
    the embedding by euclidean, ties take the lowest rank.  With fit_rows the measures are also given over the fitted rows
    and over the transformed rows alone -- what the shortcut costs; every neighbour list is still taken over all rows.
    With model.world_size > 1 every rank gathers the rows and computes the same numbers."""
    arch = _Arch(model, config, "evaluate_embedding_quality").require("latent")
    start = time.time()
    X, _ = _whole_set(arch, dataloader, arch.latent, labels=True)
    _, embedding = _umap_embed(X, fit_rows)
    q = embedding_quality(X, embedding.contiguous(), n_neighbors=n_neighbors, metric="cosine")
    chosen = _umap_fit_subset(X.shape[0], fit_rows)
    report = EmbeddingQualityReport(**vars(q), embedding=embedding.cpu().numpy(), fitted_rows=chosen,
                                    fitted=None if chosen is None else subset_scores(q, chosen),
                                    transformed=None if chosen is None else subset_scores(q, ~chosen))
    report.inference_time = time.time() - start
    line = f"Trustworthiness: {report.trustworthiness:.4f}, Continuity: {report.continuity:.4f} (k={report.n_neighbors}, {report.n_samples} samples)"
    if chosen is not None:
        line += (f"; fitted rows {report.fitted[0]:.4f} / {report.fitted[1]:.4f}, transformed rows "
                 f"{report.transformed[0]:.4f} / {report.transformed[1]:.4f}")
    print(line + f", Inference Time: {report.inference_time:.3f}")
    return report


def _epoch(model):
    return getattr(model, "current_epoch", 0)


def decode_prototype(vit, prototype, num_patches, embed_dim, device):
    """evaluation.py:209-222 (same signature) -> recon_img [1, C, S, S] on the device: the prototype behind a zero CLS row
    through the decoder, unpatchified.  Runs in the ViT's decoder-only buffers (ViTAutoencoder.decode_prototypes)."""
    proto = prototype.to(device).reshape(1, num_patches * embed_dim)
    images, _ = vit.decode_prototypes(proto, chunk=1, want_canvas=False)
    return images


def decoded_prototype_canvas(model, config, chunk=512, gap=1):
    """The computing half of visualize_decoded_prototypes: every prototype decoded, `chunk` per decoder pass, and laid
    out on the map grid on the device.  Returns (images [K, C, S, S] float32, canvas uint8 [H, W, 3]) as host arrays;
    prototype k sits at cell divmod(k, cols), cells `gap` white pixels apart.  Writes no file."""
    d, vit_hp = config["data"], config["hyperparameters"]["vit"]
    prototypes = model.som_layer.prototypes.detach()
    num_patches = (d["input_size"] // vit_hp["patch_size"]) ** 2
    if prototypes.shape[1] != num_patches * vit_hp["emb_dim"]:
        raise ValueError("Prototype dimensions mismatch for decoding.")
    images, canvas = model.vit.decode_prototypes(prototypes, model.som_layer.map_size, chunk=chunk, gap=gap)
    return images.cpu().numpy(), canvas.cpu().numpy()


def visualize_decoded_prototypes(model, config, output_dir="experiments/plots", return_decoded=False, chunk=512, gap=1):
    """evaluation.py:153-207: the SOM prototypes decoded into image space and drawn on the map grid.  The reference runs
    one decoder pass and one Axes per prototype; here the prototypes go through the decoder `chunk` at a time and the
    picture is ONE image assembled on the device (decoded_prototype_canvas), drawn by rank 0.  Returns the
    [K, C, S, S] array when return_decoded, else None."""
    model.eval()
    hp = config["hyperparameters"]
    if not _Arch.is_vit_som(config) or hp.get("som", {}).get("use_reduced", False):
        print("Visualization supported only for vit_som with use_reduced=False.")
        return None
    images, canvas = decoded_prototype_canvas(model, config, chunk=chunk, gap=gap)
    if _rank(model) == 0:
        if draw_decoded_prototypes(canvas, output_dir, hp["model_arch"], _epoch(model)) is not None:
            print(f"Saved decoded prototypes visualization to {output_dir}")
    return images if return_decoded else None


@torch.no_grad()
def visualize_label_heatmap(model, config, dataloader, output_dir="experiments/plots"):
    """evaluation.py:224-265: the ground-truth label that lands on each map cell, as an annotated heat-map.  Where several
    samples hit a cell the LAST one in loader order wins, as in the reference's loop; the fold runs on the device
    (`vsom_last_label`: an atomic max over (sample ordinal, label) words), one launch per batch and no host
    synchronisation in the loop.  With model.world_size > 1 every rank folds its shard, ordinals are shifted so that rank
    r's samples follow rank r - 1's, and one MAX all-reduce combines the tables.  Returns the int64 [rows, cols] array
    of the whole set (the reference returns None); a cell no sample hit holds 0."""
    who = "visualize_label_heatmap"
    arch = _Arch(model, config, who).require()
    rows, cols = model.som_layer.map_size
    cells = torch.zeros(rows * cols, dtype=torch.int64, device=arch.device)
    bad = torch.zeros(1, dtype=torch.int32, device=arch.device)
    seen = 0
    batches = arch.batches(dataloader, arch.own)
    for x, y in batches:
        bmu, _ = model.predict(x)
        ops.last_label(bmu.contiguous().view(-1), y, seen, cells, bad)
        seen += y.numel()
    before, _ = _rank_shift(model, seen, who)
    if _world(model) > 1:
        import torch.distributed as dist
        cells = torch.where(cells != 0, cells + (before << 32), cells)
        dist.all_reduce(cells, op=dist.ReduceOp.MAX)
        bad = bad.long()
        dist.all_reduce(bad)
    nbad = int(bad.item())
    if nbad:
        raise ValueError(f"{nbad} BMU indices fell outside the {rows} x {cols} map or labels outside [0, 2^31)")
    heatmap = (cells & 0xFFFFFFFF).view(rows, cols).cpu().numpy()
    if _rank(model) == 0:
        if draw_label_heatmap(heatmap, output_dir, arch.name, _epoch(model)) is not None:
            print(f"Saved label heatmap visualization to {output_dir}")
    return heatmap


# ------------------------------------------------------------------------------------ map quality
@dataclass
class MapQuality:
    """Host values of one evaluate_map_quality pass.  Arrays are [rows, cols], unit k at divmod(k, cols)."""
    quantization_error: float            # mean over the samples of dist[i, bmu[i]]
    topographic_error: float             # share of samples whose best and second-best units are not grid neighbours
    hits: np.ndarray                     # int64: samples per unit
    dead_units: int                      # units no sample hit
    cell_quantization_error: np.ndarray  # float64: mean dist of the samples a unit won, NaN where hits == 0
    nearest_sample: np.ndarray           # int64: loader ordinal of the sample closest to the unit (over ALL samples), -1 if none
    nearest_distance: np.ndarray         # float32: its distance, NaN if none
    n_samples: int
    inference_time: float


def _key_to_float(key):
    """Inverse of vsom_map_stats' ordered_key on a uint32 array -> float32."""
    key = np.asarray(key, dtype=np.uint32)
    bits = np.where(key & np.uint32(0x80000000), key ^ np.uint32(0x80000000), ~key).astype(np.uint32)
    return bits.view(np.float32)


_SIGN64 = -(1 << 63)


@torch.no_grad()
def evaluate_map_quality(model, config, dataloader):
    """Quantization error, topographic error, hit map and the nearest sample of every unit over the loader -> MapQuality.
    For vit_som and desom.  Every batch goes through predict(); the distances [B, K] and BMUs it leaves in the SOM layer's
    buffers are folded on the device by one `vsom_map_stats` launch (integer atomics only: the report is bitwise
    reproducible) -- no clone and no host synchronisation in the loop; rows the kernel refused (a NaN distance, a BMU off
    the map, a distance of 2^31 or more) are counted and raise ValueError at the end.  Neighbourhood on the grid is
    SOMLayer.adjacency_radius2() applied to the layer's own grid_positions, so both topologies take the same path.
    The second-best unit is the argmin, BMU excluded, of the distances the BMU pass wrote: the cosine pass re-ranks exactly
    only the prototypes within its window of the minimum, so a runner-up outside that window is chosen among distances
    that each carry the contraction's rounding error.  With model.world_size > 1 every rank folds its shard, ordinals are
    shifted so that rank r's samples follow rank r - 1's, and one SUM and one MIN all-reduce combine the tables: every
    rank returns the whole set's report."""
    who = "evaluate_map_quality"
    arch = _Arch(model, config, who).require()
    som = model.som_layer
    rows, cols = som.map_size
    K = rows * cols
    dev = arch.device
    adj_r2 = som.adjacency_radius2()
    sums = torch.zeros(2 * K + 1, dtype=torch.int64, device=dev)          # hits | qe_fix | te: one all-reduce
    hits, qe_fix, te = sums[:K], sums[K:2 * K], sums[2 * K:]
    nearest = torch.full((K,), -1, dtype=torch.int64, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    seen, start = 0, time.time()
    batches = arch.batches(dataloader, arch.own, labels=False)
    for x, _ in batches:
        bmu, _ = model.predict(x)
        s = som._buffers_for(bmu.shape[0], bmu.device)                  # the set predict() has just written
        if s.bmu.data_ptr() != bmu.data_ptr():
            raise RuntimeError("evaluate_map_quality: predict() did not leave its distances in the SOM layer's buffers")
        ops.map_stats(s.dist, s.bmu, som.grid_positions, adj_r2, seen, hits, qe_fix, te, nearest, bad)
        seen += bmu.shape[0]
    before, seen = _rank_shift(model, seen, who)
    if _world(model) > 1:
        import torch.distributed as dist
        both = torch.cat([sums, bad.long()])
        dist.all_reduce(both)
        sums, bad = both[:-1], both[-1:]
        hits, qe_fix, te = sums[:K], sums[K:2 * K], sums[2 * K:]
        # the words are unsigned: flipping the top bit makes int64 order their order (an empty cell, all-ones, stays largest)
        nearest = torch.where(nearest != -1, nearest + before, nearest) ^ _SIGN64
        dist.all_reduce(nearest, op=dist.ReduceOp.MIN)
        nearest = nearest ^ _SIGN64
    nbad = int(bad.item())
    if nbad:
        raise ValueError(f"{nbad} rows had a BMU outside the {rows} x {cols} map, a NaN distance or a distance of 2^31 or more")
    h = hits.cpu().numpy()
    q = qe_fix.cpu().numpy()
    near = nearest.cpu().numpy()
    n_te = int(te.item())
    inference_time = time.time() - start
    scale = float(2 ** 32)
    total = sum(int(v) for v in q)                         # Python integers: the sum over the cells cannot overflow
    empty = near == -1
    report = MapQuality(
        quantization_error=total / scale / seen if seen else float("nan"),
        topographic_error=n_te / seen if seen else float("nan"),
        hits=h.reshape(rows, cols),
        dead_units=int((h == 0).sum()),
        cell_quantization_error=np.where(h > 0, q / scale / np.maximum(h, 1), np.nan).reshape(rows, cols),
        nearest_sample=np.where(empty, -1, near & 0xFFFFFFFF).astype(np.int64).reshape(rows, cols),
        nearest_distance=np.where(empty, np.float32("nan"), _key_to_float((near >> 32) & 0xFFFFFFFF)).astype(np.float32).reshape(rows, cols),
        n_samples=int(seen),
        inference_time=inference_time)
    print(f"Quantization error: {report.quantization_error:.4f}, Topographic error: {report.topographic_error:.4f}, "
          f"Dead units: {report.dead_units}/{K}, Inference Time: {inference_time:.3f}")
    return report


def umatrix(model):
    """-> (u [rows, cols] float32, nbr_idx [K, 8] int32, nbr_dist [K, 8] float32) as host arrays: for every unit its grid
    neighbours (SOMLayer.adjacency_radius2() on the layer's grid_positions; ascending index order, -1 padding), the
    distance of their prototypes to the unit's in the layer's distance function, and the mean of those (`vsom_umatrix`:
    fp64 accumulation; the euclidean distance in its difference form).  Needs no data and touches no training buffer."""
    som = model.som_layer
    rows, cols = som.map_size
    u, nbr_idx, nbr_dist = ops.umatrix(som.prototypes.detach().contiguous(), som.grid_positions, som.adjacency_radius2(), som._dist_mode)
    return u.view(rows, cols).cpu().numpy(), nbr_idx.cpu().numpy(), nbr_dist.cpu().numpy()


@dataclass
class MapNeighbourhood:
    """Host values of map_neighbourhood.  Unit u is row u; its grid neighbours in umatrix's order, -1 padding."""
    neighbours: np.ndarray               # int32 [K, 8]: umatrix(model)[1]
    ranks: np.ndarray                    # int64 [K, 8]: rank of the grid neighbour among the other K - 1 prototypes (1 = nearest), -1 padding
    mean_rank: float                     # over all grid edges (each seen from both ends)
    within_degree: float                 # share of grid neighbours among the unit's deg(u) nearest prototypes


def map_neighbourhood(model):
    """Is the map folded?  For every unit, where its grid neighbours rank among all prototypes by prototype distance ->
    MapNeighbourhood.  Needs no data and no labels, like umatrix: the neighbour table is umatrix's (the layer's topology,
    square or hexagonal), the ranks are one `vsom_knn_ranks` call on the prototypes in the layer's distance function
    (cosine or euclidean; anything else raises ValueError); tied prototypes share the lowest rank.  On a well-ordered map
    a unit's deg(u) grid neighbours ARE its deg(u) nearest prototypes: mean_rank near (deg + 1) / 2 and within_degree near 1."""
    som = model.som_layer
    if som._dist_mode not in (ops.DIST_COSINE, ops.DIST_EUCLIDEAN):
        raise ValueError(f"map_neighbourhood: the layer's distance {som.distance_fcn!r} is not one the rank kernel has (cosine, euclidean)")
    protos = som.prototypes.detach().float().contiguous()
    nbr_idx = umatrix(model)[1]
    nbr = torch.from_numpy(nbr_idx.astype(np.int64)).to(protos.device)
    less = torch.empty(nbr.shape, dtype=torch.int32, device=protos.device)
    tied = torch.empty(nbr.shape, dtype=torch.int32, device=protos.device)
    ops.knn_ranks(protos, nbr, som._dist_mode, less, tied)
    less = less.cpu().numpy().astype(np.int64)
    valid = less >= 0
    ranks = np.where(valid, 1 + less, -1)
    deg = valid.sum(axis=1, keepdims=True)
    n = int(valid.sum())
    return MapNeighbourhood(neighbours=nbr_idx, ranks=ranks,
                            mean_rank=float(ranks[valid].sum() / n) if n else float("nan"),
                            within_degree=float((valid & (ranks <= deg)).sum() / n) if n else float("nan"))


def _save_cell_map(model, config, output_dir, who, suffix, kind, values, label, annotate=False):
    """Rank 0: one value per map cell as an image -> {output_dir}/{model_arch}_epoch_{epoch}_{suffix}.png."""
    if _rank(model) == 0:
        model_arch = config["hyperparameters"]["model_arch"]
        path = os.path.join(output_dir, f"{model_arch}_epoch_{_epoch(model)}_{suffix}.png")
        if _draw_map(who, values, label, annotate, path) is not None:
            print(f"Saved {kind} visualization to {output_dir}")


def visualize_umatrix(model, config, output_dir="experiments/plots"):
    """The U-matrix as one image -> {output_dir}/{model_arch}_epoch_{epoch}_umatrix.png (rank 0; skipped with a warning when
    matplotlib is missing).  Returns u [rows, cols] float32."""
    u, _, _ = umatrix(model)
    _save_cell_map(model, config, output_dir, "visualize_umatrix", "umatrix", "U-matrix", u, "mean distance to the grid neighbours")
    return u


@torch.no_grad()
def visualize_hit_map(model, config, dataloader, output_dir="experiments/plots"):
    """Samples per unit (evaluate_map_quality's hits) as one image -> {output_dir}/{model_arch}_epoch_{epoch}_hit_map.png
    (rank 0; skipped with a warning when matplotlib is missing).  Returns hits [rows, cols] int64."""
    hits = evaluate_map_quality(model, config, dataloader).hits
    _save_cell_map(model, config, output_dir, "visualize_hit_map", "hit_map", "hit map", hits, "samples", annotate=True)
    return hits


# ------------------------------------------------------------------------------------ silhouette
@torch.no_grad()
def _som_latents(model, config, dataloader, who):
    """(X [N, D] float32, bmu [N] int64) over the loader, on the device: the rows the SOM layer was given and the unit
    each of them won (_Arch.som_input), copied before the next batch overwrites them.  With model.world_size > 1 every
    rank gathers all rows, rank 0's first."""
    arch = _Arch(model, config, who).require("som_input")
    return _whole_set(arch, dataloader, arch.som_input, labels=False)


@torch.no_grad()
def evaluate_silhouette(model, config, dataloader, clusters="bmu", metric=None, n_clusters=None, sample_size=None):
    """Silhouette coefficient (silhouette.py: `vsom_silhouette`) of the latents the SOM layer sees -> SilhouetteReport.  No
    labels are read.
    clusters="bmu": every sample's cluster is the unit it won; the report has one cluster per unit of the map
        (per_cluster / counts indexed by unit, NaN / 0 for a dead unit), so per_cluster shows which cells are clusters of
        their own and which only split a continuum.
    clusters="kmeans": the clusters of the project's KMeans(n_clusters, random_state=0, n_init=10) on those latents
        (n_clusters defaults to data.num_classes).
    metric: "cosine" or "euclidean"; None takes the SOM's distance_fcn when it is one of the two and "euclidean"
        otherwise -- a manhattan map is scored with EUCLIDEAN distances, the kernel has no manhattan contraction.
    sample_size: score a subset only, numpy.random.RandomState(0).permutation(N)[:sample_size], gathered on the device.
    With model.world_size > 1 every rank gathers the rows (as evaluate_kmeans does) and computes the same report."""
    who = "evaluate_silhouette"
    if clusters not in ("bmu", "kmeans"):
        raise ValueError(f"{who}: clusters must be 'bmu' or 'kmeans', got {clusters!r}")
    som = model.som_layer
    if metric is None:
        metric = som.distance_fcn if som.distance_fcn in ("cosine", "euclidean") else "euclidean"
    start = time.time()
    X, units = _som_latents(model, config, dataloader, who)
    if sample_size is not None:
        rows = torch.from_numpy(np.random.RandomState(0).permutation(X.shape[0])[:int(sample_size)]).to(X.device)
        X, units = X[rows].contiguous(), units[rows].contiguous()
    if clusters == "bmu":
        report = cluster_silhouette(X, units, metric=metric, n_clusters=som.n_prototypes)
    else:
        k = int(n_clusters) if n_clusters else int(config["data"]["num_classes"])
        report = cluster_silhouette(X, KMeans(n_clusters=k, random_state=0, n_init=10).fit_predict(X).long(), metric=metric)
    report.inference_time = time.time() - start
    print(f"Silhouette ({clusters}, {metric}): {report.score:.4f} over {report.n_samples} samples in "
          f"{int((report.counts > 0).sum())} clusters, Inference Time: {report.inference_time:.3f}")
    return report


@torch.no_grad()
def visualize_silhouette_map(model, config, dataloader, output_dir="experiments/plots", metric=None):
    """The mean silhouette of every unit's samples (evaluate_silhouette, clusters="bmu") on the grid ->
    {output_dir}/{model_arch}_epoch_{epoch}_silhouette_map.png (rank 0; skipped with a warning when matplotlib is
    missing).  Dead units are left blank.  Returns the values [rows, cols] float64, NaN for a dead unit."""
    rows, cols = model.som_layer.map_size
    values = evaluate_silhouette(model, config, dataloader, clusters="bmu", metric=metric).per_cluster.reshape(rows, cols)
    _save_cell_map(model, config, output_dir, "visualize_silhouette_map", "silhouette_map", "silhouette map",
                   np.ma.masked_invalid(values), "mean silhouette of the unit's samples")
    return values


# ------------------------------------------------------------------------------------ principal components
SPECTRUM_SHARES = (0.5, 0.9, 0.95, 0.99)


def components_for(cumulative_ratio, shares=SPECTRUM_SHARES):
    """{share: the first k (counted from 1) whose cumulative explained-variance ratio reaches it, or None}."""
    c = np.asarray(cumulative_ratio, np.float64)
    return {s: (int(np.argmax(c >= s)) + 1 if bool((c >= s).any()) else None) for s in shares}


def effective_rank(eigenvalues) -> float:
    """exp of the entropy of the given eigenvalues renormalised to sum 1 (Roy & Vetterli 2007) -- of the top-k spectrum
    when only the top k are given: m equal eigenvalues give m, one dominant eigenvalue gives 1."""
    lam = np.maximum(np.asarray(eigenvalues, np.float64), 0.0)
    total = lam.sum()
    if total <= 0:
        return 0.0
    p = lam[lam > 0] / total
    return float(np.exp(-(p * np.log(p)).sum()))


@dataclass
class LatentSpectrum:
    """Host values of one evaluate_latent_spectrum pass: the top of the spectrum of the latents' covariance."""
    explained_variance: np.ndarray           # float64 [k], descending
    explained_variance_ratio: np.ndarray     # float64 [k]: over total_variance
    cumulative_ratio: np.ndarray             # float64 [k]
    total_variance: float                    # the sum of the D column variances
    components_for: dict                     # {0.5, 0.9, 0.95, 0.99} -> first k reaching that share of the variance, or None
    effective_rank: float                    # of the top-k spectrum: exp(entropy of the k eigenvalues renormalised to sum 1)
    residuals: np.ndarray                    # float64 [k]: PCA.residuals_
    n_samples: int
    inference_time: float = 0.0


@torch.no_grad()
def evaluate_latent_spectrum(model, config, dataloader, n_components=64):
    """The spectrum of the latents the SOM layer sees (pca.py, on the device) -> LatentSpectrum: how many directions the
    encoder uses, whether it collapses, how much of the variance a 2-D picture shows.  n_components is cut to
    min(N, D).  With model.world_size > 1 every rank gathers the rows and computes the same report."""
    from .pca import PCA
    start = time.time()
    X, _ = _som_latents(model, config, dataloader, "evaluate_latent_spectrum")
    k = max(1, min(int(n_components), X.shape[0], X.shape[1]))
    p = PCA(n_components=k).fit(X)
    ev = p.explained_variance_.cpu().numpy()
    ratio = p.explained_variance_ratio_.cpu().numpy()
    cum = np.cumsum(ratio)
    report = LatentSpectrum(ev, ratio, cum, p.total_variance_, components_for(cum), effective_rank(ev), p.residuals_.cpu().numpy(),
                            int(X.shape[0]), time.time() - start)
    print(f"Latent spectrum: effective rank {report.effective_rank:.2f} of the top {k}, {report.components_for[0.9]} components "
          f"for 90% of the variance, PC1+PC2 {float(ratio[:2].sum()):.3f}, Inference Time: {report.inference_time:.3f}")
    return report


@torch.no_grad()
def visualize_pca_map(model, config, dataloader, epoch=0, output_dir="experiments/plots/vit_som/pca"):
    """The linear counterpart of visualize_umap_map: the latents projected on their first two principal components
    (pca.py), coloured by label, with the SOM's prototypes `transform`ed into the same plane and the unit grid drawn over
    them -> output_dir/som_pca_map_epoch_{epoch}.png (rank 0 only; skipped with a warning when matplotlib is missing).
    Deterministic and without hyper-parameters, so comparable from epoch to epoch; the axis labels carry the
    explained-variance ratios.  Returns (projection [N, 2] float32, labels [N], prototype_projection [K, 2] float32,
    explained_variance_ratio [2]) as host arrays."""
    from .pca import PCA
    who = "visualize_pca_map"
    arch = _Arch(model, config, who).require("latent")
    X, y = _whole_set(arch, dataloader, arch.latent, labels=True)
    p = PCA(n_components=2).fit(X)
    proj = p.transform(X).cpu().numpy()
    protos = p.transform(model.som_layer.prototypes.detach().float().contiguous()).cpu().numpy()
    ratio, all_labels = p.explained_variance_ratio_.cpu().numpy(), y.cpu().numpy()
    nbr_idx = umatrix(model)[1]
    if _rank(model) == 0:
        axes = (f"PC1 ({100 * ratio[0]:.1f}% of the variance)", f"PC2 ({100 * ratio[1]:.1f}% of the variance)")
        _save_scatter(who, output_dir, f"som_pca_map_epoch_{epoch}.png", proj, all_labels, grid=(protos, nbr_idx),
                      axis_labels=axes, bbox_inches="tight", dpi=400)
    return proj, all_labels, protos, ratio


def _latents_keeping_mode(model, config, dataloader, who, max_rows):
    """_som_latents' rows, at most max_rows of them (the first ones), with the model back in the training or eval mode it
    was in."""
    training = model.training
    try:
        X, _ = _som_latents(model, config, dataloader, who)
    finally:
        model.train(training)
    return X if max_rows is None else X[:int(max_rows)]


@torch.no_grad()
def init_som_from_data(model, config, dataloader, method="pca", max_rows=None):
    """Start the SOM's prototypes from the data (SOMLayer.init_prototypes): the latents of the loader through the CURRENT
    encoder, at most max_rows of them (the first ones), method "pca" or "sample".  Returns the fitted PCA or None."""
    X = _latents_keeping_mode(model, config, dataloader, "init_som_from_data", max_rows)
    return model.som_layer.init_prototypes(X, method=method)


@torch.no_grad()
def fit_som_batch(model, config, dataloader, epochs=10, init=None, sigma=None, max_rows=None):
    """Fit the SOM to the data with Kohonen's batch map (SOMLayer.fit_batch) -> BatchSOMReport: the latents of the loader
    through the CURRENT encoder (a frozen or pretrained one is what this is for), at most max_rows of them (the first ones);
    init "pca" or "sample" first starts the prototypes from those latents (SOMLayer.init_prototypes), None keeps them as
    they are.  sigma as in fit_batch (None: Tmax down to Tmin).  For vit_som and desom; the model's training mode is
    restored.  With model.world_size > 1 every rank holds all rows and computes the same map."""
    X = _latents_keeping_mode(model, config, dataloader, "fit_som_batch", max_rows)
    som = model.som_layer
    if init is not None:
        som.init_prototypes(X, method=init)
    return som.fit_batch(X, epochs=epochs, sigma=sigma)


# ------------------------------------------------------------------------------------ kNN probe
@dataclass
class KNNReport:
    """Host values of one evaluate_knn pass.  confusion[t, p] counts the test samples of class t predicted as p."""
    accuracy: float
    per_class_accuracy: np.ndarray       # float64 [C]: NaN for a class without a test sample
    confusion: np.ndarray                # int64 [C, C]
    n_train: int                         # bank rows (over all ranks)
    n_test: int                          # queries (over all ranks)
    k: int
    inference_time: float


@torch.no_grad()
def evaluate_knn(model, config, train_loader, test_loader, k=20, weights="softmax", metric="cosine", temperature=0.07,
                 bank_rows=4096, num_labels=None):
    """k-nearest-neighbour probe of the latents -> KNNReport: every sample of test_loader is classified by the weighted vote
    (KNNClassifier) of its k nearest samples of train_loader in feature space; nothing is trained.  Features: for vit_som
    model.get_latent_representation(x) (what visualize_umap_progression embeds), for desom the x_encoded that
    evaluate_kmeans clusters; any other model raises ValueError.
    Pass 1 keeps the test features and labels on the device.  Pass 2 copies each training batch's features into a buffer of
    `bank_rows` rows (the loaders and the model reuse their buffers: features are copied, never kept as views) and folds the
    buffer into the neighbour lists whenever it is full and once at the end, so the query matrix is re-read once per
    `bank_rows` training rows, not once per batch; the lists do not depend on bank_rows (knn.py).  Then one vote launch and one
    `vsom_contingency` launch.  No host synchronisation inside either loop.  Labels must lie in [0, num_labels) (default
    data.num_classes, or 256 when the config has none; at most 1024).
    With model.world_size > 1 each rank keeps its own shard of the test queries and every bank buffer is all-gathered
    (rank 0's rows first) before it is folded, so every rank must see the same number of training rows; the confusion
    counts are summed over the ranks and every rank returns the whole set's report."""
    arch = _Arch(model, config, "evaluate_knn").require("latent")
    dev, L = arch.device, _label_count(config, num_labels, False)
    bank_rows = int(bank_rows)
    if bank_rows < 1:
        raise ValueError(f"evaluate_knn: bank_rows must be positive, got {bank_rows}")
    clf = KNNClassifier(n_neighbors=k, weights=weights, metric=metric, temperature=temperature, n_classes=L)
    clf._validate()
    world, start = _world(model), time.time()
    Q, yq = _rows(arch, test_loader, arch.latent, labels=True, what="test loader")
    clf.partial_fit_query(Q)
    buf = torch.empty(bank_rows, Q.shape[1], dtype=torch.float32, device=dev)
    ybuf = torch.empty(bank_rows, dtype=torch.int64, device=dev)
    fill = 0

    def fold(n):
        bx, by = buf[:n], ybuf[:n]
        if world > 1:
            bx, by = _gather_rows(bx, world).contiguous(), _gather_rows(by, world).contiguous()
        if bx.shape[0]:
            clf.update(bx, by)

    batches = arch.batches(train_loader, arch.own)
    for x, y in batches:
        f = arch.latent(x)
        f = f.reshape(f.shape[0], -1)
        off = 0
        while off < f.shape[0]:
            n = min(f.shape[0] - off, bank_rows - fill)
            buf[fill:fill + n].copy_(f[off:off + n])
            ybuf[fill:fill + n].copy_(y[off:off + n])
            fill, off = fill + n, off + n
            if fill == bank_rows:
                fold(fill)
                fill = 0
    if fill or world > 1:
        fold(fill)
    n_train = clf._seen
    if n_train < clf.n_neighbors:
        raise ValueError(f"evaluate_knn: k={clf.n_neighbors} exceeds the {n_train} training samples")
    pred = clf.predict()
    table = _Table(L, L, dev)
    table.add(yq, pred)                                   # cm[true, pred]; a label outside [0, L) is counted and raises below
    cm = table.numpy(world)
    refused = clf._status[:1].long()
    if world > 1:
        import torch.distributed as dist
        dist.all_reduce(refused)
    if int(refused.item()):
        raise ValueError(f"evaluate_knn: {int(refused.item())} neighbour labels fell outside [0, {L}); pass num_labels= for larger label sets")
    inference_time = time.time() - start
    true_sum = cm.sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        per_class = np.where(true_sum > 0, np.diag(cm) / true_sum, np.nan)
    n_test = int(cm.sum())
    report = KNNReport(accuracy=float(np.diag(cm).sum() / n_test) if n_test else float("nan"), per_class_accuracy=per_class,
                       confusion=cm.astype(np.int64), n_train=int(n_train), n_test=n_test, k=int(clf.n_neighbors),
                       inference_time=inference_time)
    print(f"kNN accuracy (k={report.k}, {weights}, {metric}): {report.accuracy:.3f}, Inference Time: {inference_time:.3f}")
    return report


@torch.no_grad()
def evaluate_classification(model, config, dataloader):
    """evaluation.py:93-128 -> (accuracy, precision, recall, f1, inference_time) (macro averages); summed over the
    ranks like evaluate_clustering."""
    arch = _Arch(model, config, "evaluate_classification")
    ncls = config["data"]["num_classes"]
    table, pred, start = _Table(ncls, ncls, arch.device), None, time.time()
    batches = arch.batches(dataloader, arch.images)
    for x, y in batches:
        _, logits = model.predict(x)
        if pred is None or pred.numel() != logits.shape[0]:
            pred = torch.empty(logits.shape[0], dtype=torch.int64, device=arch.device)
        ops.argmax_rows(logits, pred)
        table.add(y, pred)                                # cm[true, pred]
    acc, precision, recall, f1 = classification_from_table(table.numpy(_world(model)))
    inference_time = time.time() - start
    print(f"Accuracy: {acc:.3f}, Precision: {precision:.3f}, Recall: {recall:.3f}, F1-score: {f1:.3f}, Inference Time: {inference_time:.3f}")
    return acc, precision, recall, f1, inference_time
