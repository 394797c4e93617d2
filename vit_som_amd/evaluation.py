"""On-device evaluation mirroring the reference's tools/evaluation.py entry points
(evaluate_clustering :18-52, evaluate_kmeans :54-91, evaluate_classification :93-128, calculate_purity :130-151).

The model forward runs on the HIP kernels (encoder + SOM only: `ViTSOM.predict`); BMU / label
pairs are folded into a contingency table ON DEVICE batch by batch (`vsom_contingency`, integer
atomics), so the only device->host traffic of a whole evaluation pass is that table.  Purity, NMI
(sklearn's arithmetic-mean normalisation) and the macro precision / recall / F1 are O(classes^2)
host arithmetic on the table.  evaluate_kmeans keeps the model outputs in one device buffer and clusters them with
the HIP k-means (kmeans.py); visualize_umap_progression (:267-323) embeds the latent representations with the HIP
UMAP (umap.py), and visualize_umap_map (no counterpart) places the SOM's prototypes into that embedding with
UMAP.transform and draws the unit grid over it.  The two pictures of the map itself: visualize_decoded_prototypes / decode_prototype (:153-222) push the
prototypes through the ViT decoder in batches and assemble the mosaic on the device (`vsom_proto_mosaic`);
visualize_label_heatmap (:224-265) folds (BMU, label) pairs into a last-label-per-cell table (`vsom_last_label`).
Map quality has no counterpart in the reference: evaluate_map_quality folds the distances and BMUs every predict() leaves
in the SOM layer's buffers into quantization error, topographic error, hit map and nearest sample per unit
(`vsom_map_stats`), umatrix / visualize_umatrix / visualize_hit_map draw the map without labels (`vsom_umatrix`).
evaluate_knn (no counterpart either) asks how much class information the latents carry: every test sample is classified by
a weighted vote of its k nearest training samples in latent space (knn.py: `vsom_knn_query` / `vsom_knn_vote`), the training
set streamed through a fixed-size device buffer.
evaluate_embedding_quality (no counterpart either) says how far the UMAP pictures can be believed: trustworthiness and
continuity of the embedding against the latents (embedding_quality.py: `vsom_umap_knn` / `vsom_knn_ranks`); map_neighbourhood
asks the same of the map itself, the prototypes against their grid.
evaluate_silhouette (no counterpart either) says whether the clusters -- the SOM's units, or k-means' -- are compact and
separated in latent space, without labels (silhouette.py: `vsom_silhouette`); visualize_silhouette_map draws it per unit.
Principal components (pca.py: `vsom_pca_*`; no counterpart either): evaluate_latent_spectrum says how many directions the
encoder uses, visualize_pca_map is the linear, deterministic counterpart of visualize_umap_map, and init_som_from_data
starts the map on the plane of the latents' first two principal components (SOMLayer.init_prototypes).
"""
import os
import time
from dataclasses import dataclass

import numpy as np
import torch

from . import ops
from .embedding_quality import EmbeddingQuality, embedding_quality, subset_scores
from .kmeans import KMeans
from .knn import KNNClassifier
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


def evaluate_clustering(model, config, dataloader, num_labels=None):
    """evaluation.py:18-52 -> (purity, nmi, inference_time) from the model's native BMU assignments.  No host
    synchronisation inside the loop: labels outside [0, num_labels) are counted on the device and reported once at the
    end (num_labels defaults to max(data.num_classes, 256)).  With model.world_size > 1 every rank folds its shard and
    the tables are summed, so all ranks return the metrics of the whole set."""
    model.eval()
    d = config["data"]
    C, S = d["num_channels"], d["input_size"]
    K = model.som_layer.n_prototypes
    dev = model.arena.device
    L = int(num_labels) if num_labels else max(int(d.get("num_classes", 0)), 256)
    table, start = _Table(K, L, dev), time.time()
    for x, y in dataloader:
        x = x.to(dev, non_blocking=True).reshape(-1, C, S, S)
        y = y.to(dev, non_blocking=True)
        bmu, _ = model.predict(x)
        table.add(bmu, y.view(-1))
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


def evaluate_kmeans(model, config, dataloader, num_labels=None):
    """evaluation.py:54-91 -> (purity, nmi, inference_time) of KMeans(n_clusters=len(unique(labels)), random_state=0,
    n_init=10) on the model's outputs.  The features are what the reference clusters: for vit_som the SECOND output of
    ViTSOM.forward, i.e. recon_img flattened to C*H*W (the reference calls it x_encoded, vit_som.py:67-78), for desom
    the encoder latent x_encoded (desom.py:50-54).  Features and labels stay on the device; the fit is the HIP k-means
    (kmeans.py).  Labels must lie in [0, num_labels) (default max(data.num_classes, 256)).  With model.world_size > 1
    every rank gathers the whole set and runs the same deterministic fit, so all ranks report the whole set's metrics."""
    model.eval()
    d = config["data"]
    C, S = d["num_channels"], d["input_size"]
    arch = config["hyperparameters"]["model_arch"]
    dev = model.arena.device
    L = int(num_labels) if num_labels else max(int(d.get("num_classes", 0)), 256)
    feats, labels, start = [], [], time.time()
    with torch.no_grad():                                  # evaluation.py:67
        for x, y in dataloader:
            x = x.to(dev, non_blocking=True)
            y = y.to(dev, non_blocking=True)
            if arch == "vit_som":
                _, f, *_ = model(x.reshape(-1, C, S, S))
            elif arch == "desom":
                _, f, *_ = model(x.reshape(x.shape[0], -1))
            else:
                raise ValueError(f"evaluate_kmeans: unknown model_arch {arch!r}")
            feats.append(f.reshape(f.shape[0], -1))
            labels.append(y.reshape(-1).long())
    X, y = torch.cat(feats), torch.cat(labels)
    world = _world(model)
    if world > 1:
        X, y = _gather_rows(X, world), _gather_rows(y, world)
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


def _umap_latents(model, config, dataloader, feats):
    """feats(x, C, S) of every batch (copied: the model's buffers are reused by the next batch) and the labels, as device
    tensors over the whole set: with model.world_size > 1 every rank gathers all rows, rank 0's first."""
    model.eval()
    d = config["data"]
    C, S = d["num_channels"], d["input_size"]
    dev = model.arena.device
    lat, labels = [], []
    with torch.no_grad():
        for x, y in dataloader:
            x = x.to(dev, non_blocking=True)
            y = y.to(dev, non_blocking=True)
            z = feats(x, C, S)
            lat.append(z.reshape(z.shape[0], -1).float().clone())
            labels.append(y.reshape(-1).long())
    X, y = torch.cat(lat), torch.cat(labels)
    world = _world(model)
    if world > 1:
        X, y = _gather_rows(X, world), _gather_rows(y, world)
    return X.contiguous(), y


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


def _draw_grid(plt, protos, nbr_idx):
    """The unit grid over a scatter plot: a line between units the topology makes adjacent, a marker per unit."""
    for u, row in enumerate(nbr_idx):
        for v in row[row > u]:                               # every grid edge once
            plt.plot(protos[[u, v], 0], protos[[u, v], 1], color="black", linewidth=0.4, alpha=0.8)
    plt.scatter(protos[:, 0], protos[:, 1], c="black", s=8, marker="o", edgecolor="white", linewidth=0.3, zorder=3)


def _umap_scatter(plt, embedding, all_labels):
    """The reference's scatter plot of an embedding, on a new figure."""
    plt.figure(figsize=(10, 8), dpi=300)
    plt.axis("off")
    scatter = plt.scatter(embedding[:, 0], embedding[:, 1], c=all_labels, cmap="tab10", s=3, alpha=0.7,
                          edgecolor="none", rasterized=True)
    cbar = plt.colorbar(scatter, ticks=range(10), drawedges=True)
    cbar.set_ticklabels([str(i) for i in range(10)])
    cbar.ax.tick_params(labelsize=10, width=0.5)
    cbar.outline.set_linewidth(0.5)


def visualize_umap_progression(model, config, dataloader, epoch=0, output_dir="experiments/plots/vit_som/umap", fit_rows=None):
    """evaluation.py:267-323: UMAP(n_neighbors=15, min_dist=0.1, metric='cosine', random_state=42) of
    model.get_latent_representation(x) over the whole set, fitted on the device (umap.py), drawn as the reference's
    scatter plot into output_dir/som_umap_epoch_{epoch}.png (rank 0 only; skipped with a warning when matplotlib is
    missing).  With model.world_size > 1 every rank gathers all rows and runs the same deterministic fit.  fit_rows (not in
    the reference): fit on a fixed subset of that many rows and transform() the others into it (_umap_embed), for sets
    whose host-side graph and spectral initialisation would take too long.  Returns (embedding [N, 2] float32, labels [N])
    as host arrays (the reference returns None)."""
    X, y = _umap_latents(model, config, dataloader, lambda x, C, S: model.get_latent_representation(x.reshape(-1, C, S, S)))
    embedding = _umap_embed(X, fit_rows)[1].cpu().numpy()
    all_labels = y.cpu().numpy()
    if int(getattr(model, "rank", 0)) == 0:
        plt = _pyplot("visualize_umap_progression")
        if plt is None:
            return embedding, all_labels
        os.makedirs(output_dir, exist_ok=True)
        _umap_scatter(plt, embedding, all_labels)
        plt.savefig(os.path.join(output_dir, f"som_umap_epoch_{epoch}.png"), bbox_inches="tight", pad_inches=0,
                    transparent=False, dpi=400)
        plt.close()
    return embedding, all_labels


def visualize_umap_map(model, config, dataloader, epoch=0, output_dir="experiments/plots/vit_som/umap", fit_rows=None):
    """The map in data space (no counterpart in the reference): the embedding of visualize_umap_progression (same
    latents, same UMAP, same fit_rows) with the SOM's K prototypes placed INTO it by UMAP.transform -- they live in the
    space of the latents -- and the unit grid drawn over the scatter plot: a marker per unit and a line between units the
    layer's topology makes adjacent (umatrix's neighbour table, square and hexagonal) ->
    output_dir/som_umap_map_epoch_{epoch}.png (rank 0 only; skipped with a warning when matplotlib is missing).  Latents:
    model.get_latent_representation(x) for vit_som, x_encoded for desom, as evaluate_knn chooses them; any other model
    raises ValueError.  Returns (embedding [N, 2] float32, labels [N], prototype_embedding [K, 2] float32) as host arrays."""
    feats = _knn_features(model, config["hyperparameters"]["model_arch"], "visualize_umap_map")
    X, y = _umap_latents(model, config, dataloader, feats)
    reducer, embedding = _umap_embed(X, fit_rows)
    protos = reducer.transform(model.som_layer.prototypes.detach().float().contiguous()).cpu().numpy()
    embedding, all_labels = embedding.cpu().numpy(), y.cpu().numpy()
    nbr_idx = umatrix(model)[1]
    if int(getattr(model, "rank", 0)) == 0:
        plt = _pyplot("visualize_umap_map")
        if plt is None:
            return embedding, all_labels, protos
        os.makedirs(output_dir, exist_ok=True)
        _umap_scatter(plt, embedding, all_labels)
        _draw_grid(plt, protos, nbr_idx)
        plt.savefig(os.path.join(output_dir, f"som_umap_map_epoch_{epoch}.png"), bbox_inches="tight", pad_inches=0,
                    transparent=False, dpi=400)
        plt.close()
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


def evaluate_embedding_quality(model, config, dataloader, n_neighbors=15, fit_rows=None):
    """Trustworthiness and continuity (embedding_quality.py) of the picture visualize_umap_map draws -> EmbeddingQualityReport.
    Same latents (_knn_features: get_latent_representation for vit_som, x_encoded for desom), same UMAP(n_neighbors=15,
    min_dist=0.1, metric='cosine', random_state=42) and same fit_rows subset; the latents are compared by cosine distance,
    the embedding by euclidean, ties take the lowest rank.  With fit_rows the measures are also given over the fitted rows
    and over the transformed rows alone -- what the shortcut costs; every neighbour list is still taken over all rows.
    With model.world_size > 1 every rank gathers the rows and computes the same numbers."""
    feats = _knn_features(model, config["hyperparameters"]["model_arch"], "evaluate_embedding_quality")
    start = time.time()
    X, _ = _umap_latents(model, config, dataloader, feats)
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


def _pyplot(who):
    """matplotlib.pyplot, or None with a warning when matplotlib is not installed (no plot is written then)."""
    try:
        import matplotlib.pyplot as plt
        return plt
    except ImportError:
        import warnings
        warnings.warn(f"{who}: matplotlib is not installed; no plot written")
        return None


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


def draw_decoded_prototypes(canvas, output_dir, model_arch, epoch):
    """One imshow of the mosaic, axis off -> {output_dir}/{model_arch}_epoch_{epoch}_decoded_prototypes.png (host only).
    Returns the path, or None when matplotlib is missing."""
    plt = _pyplot("visualize_decoded_prototypes")
    if plt is None:
        return None
    os.makedirs(output_dir, exist_ok=True)
    fig = plt.figure(figsize=(10, 10 * canvas.shape[0] / canvas.shape[1]))
    plt.imshow(canvas, interpolation="nearest")
    plt.axis("off")
    path = os.path.join(output_dir, f"{model_arch}_epoch_{epoch}_decoded_prototypes.png")
    plt.savefig(path, bbox_inches="tight")
    plt.close(fig)
    return path


def visualize_decoded_prototypes(model, config, output_dir="experiments/plots", return_decoded=False, chunk=512, gap=1):
    """evaluation.py:153-207: the SOM prototypes decoded into image space and drawn on the map grid.  The reference runs
    one decoder pass and one Axes per prototype; here the prototypes go through the decoder `chunk` at a time and the
    picture is ONE image assembled on the device (decoded_prototype_canvas), drawn by rank 0.  Returns the
    [K, C, S, S] array when return_decoded, else None."""
    model.eval()
    hp = config["hyperparameters"]
    model_arch = hp["model_arch"]
    if model_arch != "vit_som" or hp.get("som", {}).get("use_reduced", False):
        print("Visualization supported only for vit_som with use_reduced=False.")
        return None
    images, canvas = decoded_prototype_canvas(model, config, chunk=chunk, gap=gap)
    if int(getattr(model, "rank", 0)) == 0:
        if draw_decoded_prototypes(canvas, output_dir, model_arch, _epoch(model)) is not None:
            print(f"Saved decoded prototypes visualization to {output_dir}")
    return images if return_decoded else None


def draw_label_heatmap(heatmap, output_dir, model_arch, epoch):
    """The reference's sns.heatmap(annot=True, fmt="d", cmap="viridis") in plain matplotlib ->
    {output_dir}/{model_arch}_epoch_{epoch}_label_heatmap.png (host only).  Returns the path, or None without matplotlib."""
    plt = _pyplot("visualize_label_heatmap")
    if plt is None:
        return None
    os.makedirs(output_dir, exist_ok=True)
    fig = plt.figure(figsize=(10, 8))
    im = plt.imshow(heatmap, cmap="viridis", aspect="auto")
    plt.colorbar(im)
    mid = 0.5 * (float(heatmap.min()) + float(heatmap.max()))
    size = max(3.0, min(10.0, 200.0 / max(heatmap.shape)))
    for (r, c), v in np.ndenumerate(heatmap):
        plt.text(c, r, str(int(v)), ha="center", va="center", fontsize=size, color="white" if v <= mid else "black")
    plt.xticks(range(heatmap.shape[1]))
    plt.yticks(range(heatmap.shape[0]))
    path = os.path.join(output_dir, f"{model_arch}_epoch_{epoch}_label_heatmap.png")
    plt.savefig(path)
    plt.close(fig)
    return path


def visualize_label_heatmap(model, config, dataloader, output_dir="experiments/plots"):
    """evaluation.py:224-265: the ground-truth label that lands on each map cell, as an annotated heat-map.  Where several
    samples hit a cell the LAST one in loader order wins, as in the reference's loop; the fold runs on the device
    (`vsom_last_label`: an atomic max over (sample ordinal, label) words), one launch per batch and no host
    synchronisation in the loop.  With model.world_size > 1 every rank folds its shard, ordinals are shifted so that rank
    r's samples follow rank r - 1's, and one MAX all-reduce combines the tables.  Returns the int64 [rows, cols] array
    of the whole set (the reference returns None); a cell no sample hit holds 0."""
    model.eval()
    d = config["data"]
    C, S = d["num_channels"], d["input_size"]
    model_arch = config["hyperparameters"]["model_arch"]
    if model_arch not in ("vit_som", "desom"):
        raise ValueError(f"visualize_label_heatmap: unknown model_arch {model_arch!r}")
    rows, cols = model.som_layer.map_size
    dev = model.arena.device
    cells = torch.zeros(rows * cols, dtype=torch.int64, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    seen = 0
    for x, y in dataloader:
        x = x.to(dev, non_blocking=True)
        y = y.to(dev, non_blocking=True).reshape(-1).long().contiguous()
        x = x.reshape(-1, C, S, S) if model_arch == "vit_som" else x.reshape(x.shape[0], -1)
        bmu, _ = model.predict(x)
        ops.last_label(bmu.contiguous().view(-1), y, seen, cells, bad)
        seen += y.numel()
    world = _world(model)
    if world > 1:
        import torch.distributed as dist
        counts = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(world)]
        dist.all_gather(counts, torch.tensor([seen], dtype=torch.int64, device=dev))
        before = sum(int(c) for c in counts[:int(getattr(model, "rank", 0))])
        if sum(int(c) for c in counts) >= 2 ** 31:
            raise ValueError("visualize_label_heatmap: more than 2^31 - 1 samples")
        cells = torch.where(cells != 0, cells + (before << 32), cells)
        dist.all_reduce(cells, op=dist.ReduceOp.MAX)
        bad = bad.long()
        dist.all_reduce(bad)
    nbad = int(bad.item())
    if nbad:
        raise ValueError(f"{nbad} BMU indices fell outside the {rows} x {cols} map or labels outside [0, 2^31)")
    heatmap = (cells & 0xFFFFFFFF).view(rows, cols).cpu().numpy()
    if int(getattr(model, "rank", 0)) == 0:
        if draw_label_heatmap(heatmap, output_dir, model_arch, _epoch(model)) is not None:
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
    model.eval()
    d = config["data"]
    C, S = d["num_channels"], d["input_size"]
    model_arch = config["hyperparameters"]["model_arch"]
    if model_arch not in ("vit_som", "desom"):
        raise ValueError(f"evaluate_map_quality: unknown model_arch {model_arch!r}")
    som = model.som_layer
    rows, cols = som.map_size
    K = rows * cols
    dev = model.arena.device
    adj_r2 = som.adjacency_radius2()
    sums = torch.zeros(2 * K + 1, dtype=torch.int64, device=dev)          # hits | qe_fix | te: one all-reduce
    hits, qe_fix, te = sums[:K], sums[K:2 * K], sums[2 * K:]
    nearest = torch.full((K,), -1, dtype=torch.int64, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    seen, start = 0, time.time()
    for x, _ in dataloader:
        x = x.to(dev, non_blocking=True)
        x = x.reshape(-1, C, S, S) if model_arch == "vit_som" else x.reshape(x.shape[0], -1)
        bmu, _ = model.predict(x)
        s = som._buffers_for(bmu.shape[0], bmu.device)                  # the set predict() has just written
        if s.bmu.data_ptr() != bmu.data_ptr():
            raise RuntimeError("evaluate_map_quality: predict() did not leave its distances in the SOM layer's buffers")
        ops.map_stats(s.dist, s.bmu, som.grid_positions, adj_r2, seen, hits, qe_fix, te, nearest, bad)
        seen += bmu.shape[0]
    world = _world(model)
    if world > 1:
        import torch.distributed as dist
        counts = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(world)]
        dist.all_gather(counts, torch.tensor([seen], dtype=torch.int64, device=dev))
        before = sum(int(c) for c in counts[:int(getattr(model, "rank", 0))])
        seen = sum(int(c) for c in counts)
        if seen >= 2 ** 31:
            raise ValueError("evaluate_map_quality: more than 2^31 - 1 samples")
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


def _draw_map(who, values, label, annotate, path):
    plt = _pyplot(who)
    if plt is None:
        return None
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    fig = plt.figure(figsize=(10, 8))
    im = plt.imshow(values, cmap="viridis", interpolation="nearest")
    plt.colorbar(im, label=label)
    if annotate and max(values.shape) <= 24:
        mid = 0.5 * (float(values.min()) + float(values.max()))
        for (r, c), v in np.ndenumerate(values):
            plt.text(c, r, str(int(v)), ha="center", va="center", fontsize=7, color="white" if v <= mid else "black")
    plt.axis("off")
    plt.savefig(path, bbox_inches="tight")
    plt.close(fig)
    return path


def visualize_umatrix(model, config, output_dir="experiments/plots"):
    """The U-matrix as one image -> {output_dir}/{model_arch}_epoch_{epoch}_umatrix.png (rank 0; skipped with a warning when
    matplotlib is missing).  Returns u [rows, cols] float32."""
    model_arch = config["hyperparameters"]["model_arch"]
    u, _, _ = umatrix(model)
    if int(getattr(model, "rank", 0)) == 0:
        path = os.path.join(output_dir, f"{model_arch}_epoch_{_epoch(model)}_umatrix.png")
        if _draw_map("visualize_umatrix", u, "mean distance to the grid neighbours", False, path) is not None:
            print(f"Saved U-matrix visualization to {output_dir}")
    return u


def visualize_hit_map(model, config, dataloader, output_dir="experiments/plots"):
    """Samples per unit (evaluate_map_quality's hits) as one image -> {output_dir}/{model_arch}_epoch_{epoch}_hit_map.png
    (rank 0; skipped with a warning when matplotlib is missing).  Returns hits [rows, cols] int64."""
    model_arch = config["hyperparameters"]["model_arch"]
    hits = evaluate_map_quality(model, config, dataloader).hits
    if int(getattr(model, "rank", 0)) == 0:
        path = os.path.join(output_dir, f"{model_arch}_epoch_{_epoch(model)}_hit_map.png")
        if _draw_map("visualize_hit_map", hits, "samples", True, path) is not None:
            print(f"Saved hit map visualization to {output_dir}")
    return hits


# ------------------------------------------------------------------------------------ silhouette
def _som_latents(model, config, dataloader, who):
    """(X [N, D] float32, bmu [N] int64) over the loader, on the device: the rows the SOM layer was given and the unit
    each of them won.  vit_som: predict() leaves the BMUs in the SOM layer's buffers and the encoder output in the ViT's;
    both are copied before the next batch overwrites them.  desom: forward() returns both.  With model.world_size > 1
    every rank gathers all rows, rank 0's first."""
    model.eval()
    d = config["data"]
    C, S = d["num_channels"], d["input_size"]
    arch = config["hyperparameters"]["model_arch"]
    dev = model.arena.device
    lat, units = [], []
    with torch.no_grad():
        for x, _ in dataloader:
            x = x.to(dev, non_blocking=True)
            if arch == "vit_som" and hasattr(model, "_som_input"):
                x = x.reshape(-1, C, S, S)
                bmu, _ = model.predict(x)
                z = model._som_input(model.vit._buffers_for(x.shape[0], x.device))
            elif arch == "desom" and hasattr(model, "autoencoder"):
                _, z, _, bmu = model(x.reshape(x.shape[0], -1))
            else:
                raise ValueError(f"{who}: needs a vit_som or a desom model; got {type(model).__name__} with model_arch {arch!r}")
            lat.append(z.reshape(z.shape[0], -1).float().clone())
            units.append(bmu.reshape(-1).long().clone())
    if not lat:
        raise ValueError(f"{who}: the loader is empty")
    X, u = torch.cat(lat), torch.cat(units)
    world = _world(model)
    if world > 1:
        X, u = _gather_rows(X, world), _gather_rows(u, world)
    return X.contiguous(), u.contiguous()


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


def visualize_silhouette_map(model, config, dataloader, output_dir="experiments/plots", metric=None):
    """The mean silhouette of every unit's samples (evaluate_silhouette, clusters="bmu") on the grid ->
    {output_dir}/{model_arch}_epoch_{epoch}_silhouette_map.png (rank 0; skipped with a warning when matplotlib is
    missing).  Dead units are left blank.  Returns the values [rows, cols] float64, NaN for a dead unit."""
    model_arch = config["hyperparameters"]["model_arch"]
    rows, cols = model.som_layer.map_size
    values = evaluate_silhouette(model, config, dataloader, clusters="bmu", metric=metric).per_cluster.reshape(rows, cols)
    if int(getattr(model, "rank", 0)) == 0:
        path = os.path.join(output_dir, f"{model_arch}_epoch_{_epoch(model)}_silhouette_map.png")
        if _draw_map("visualize_silhouette_map", np.ma.masked_invalid(values), "mean silhouette of the unit's samples", False,
                     path) is not None:
            print(f"Saved silhouette map visualization to {output_dir}")
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


def visualize_pca_map(model, config, dataloader, epoch=0, output_dir="experiments/plots/vit_som/pca"):
    """The linear counterpart of visualize_umap_map: the latents projected on their first two principal components
    (pca.py), coloured by label, with the SOM's prototypes `transform`ed into the same plane and the unit grid drawn over
    them -> output_dir/som_pca_map_epoch_{epoch}.png (rank 0 only; skipped with a warning when matplotlib is missing).
    Deterministic and without hyper-parameters, so comparable from epoch to epoch; the axis labels carry the
    explained-variance ratios.  Returns (projection [N, 2] float32, labels [N], prototype_projection [K, 2] float32,
    explained_variance_ratio [2]) as host arrays."""
    from .pca import PCA
    feats = _knn_features(model, config["hyperparameters"]["model_arch"], "visualize_pca_map")
    X, y = _umap_latents(model, config, dataloader, feats)
    p = PCA(n_components=2).fit(X)
    proj = p.transform(X).cpu().numpy()
    protos = p.transform(model.som_layer.prototypes.detach().float().contiguous()).cpu().numpy()
    ratio, all_labels = p.explained_variance_ratio_.cpu().numpy(), y.cpu().numpy()
    nbr_idx = umatrix(model)[1]
    if int(getattr(model, "rank", 0)) == 0:
        plt = _pyplot("visualize_pca_map")
        if plt is None:
            return proj, all_labels, protos, ratio
        os.makedirs(output_dir, exist_ok=True)
        _umap_scatter(plt, proj, all_labels)
        plt.axis("on")
        plt.xlabel(f"PC1 ({100 * ratio[0]:.1f}% of the variance)")
        plt.ylabel(f"PC2 ({100 * ratio[1]:.1f}% of the variance)")
        _draw_grid(plt, protos, nbr_idx)
        plt.savefig(os.path.join(output_dir, f"som_pca_map_epoch_{epoch}.png"), bbox_inches="tight", dpi=400)
        plt.close()
    return proj, all_labels, protos, ratio


def init_som_from_data(model, config, dataloader, method="pca", max_rows=None):
    """Start the SOM's prototypes from the data (SOMLayer.init_prototypes): the latents of the loader through the CURRENT
    encoder, at most max_rows of them (the first ones), method "pca" or "sample".  Returns the fitted PCA or None."""
    training = model.training
    X, _ = _som_latents(model, config, dataloader, "init_som_from_data")
    model.train(training)
    if max_rows is not None:
        X = X[:int(max_rows)]
    return model.som_layer.init_prototypes(X, method=method)


def fit_som_batch(model, config, dataloader, epochs=10, init=None, sigma=None, max_rows=None):
    """Fit the SOM to the data with Kohonen's batch map (SOMLayer.fit_batch) -> BatchSOMReport: the latents of the loader
    through the CURRENT encoder (a frozen or pretrained one is what this is for), at most max_rows of them (the first ones);
    init "pca" or "sample" first starts the prototypes from those latents (SOMLayer.init_prototypes), None keeps them as
    they are.  sigma as in fit_batch (None: Tmax down to Tmin).  For vit_som and desom; the model's training mode is
    restored.  With model.world_size > 1 every rank holds all rows and computes the same map."""
    training = model.training
    X, _ = _som_latents(model, config, dataloader, "fit_som_batch")
    model.train(training)
    if max_rows is not None:
        X = X[:int(max_rows)]
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


def _knn_features(model, arch, who="evaluate_knn"):
    """x -> the [B, D] float32 features the probe compares (views of the model's buffers: copy before the next batch)."""
    if arch == "vit_som" and hasattr(model, "get_latent_representation"):
        return lambda x, C, S: model.get_latent_representation(x.reshape(-1, C, S, S))
    if arch == "desom" and hasattr(model, "autoencoder"):
        return lambda x, C, S: model(x.reshape(x.shape[0], -1))[1]
    raise ValueError(f"{who}: needs a vit_som model (get_latent_representation) or a desom model (x_encoded); got "
                     f"{type(model).__name__} with model_arch {arch!r}")


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
    model.eval()
    d = config["data"]
    C, S = d["num_channels"], d["input_size"]
    feats = _knn_features(model, config["hyperparameters"]["model_arch"])
    dev = model.arena.device
    L = int(num_labels) if num_labels else (int(d.get("num_classes", 0)) if int(d.get("num_classes", 0)) > 0 else 256)
    bank_rows = int(bank_rows)
    if bank_rows < 1:
        raise ValueError(f"evaluate_knn: bank_rows must be positive, got {bank_rows}")
    clf = KNNClassifier(n_neighbors=k, weights=weights, metric=metric, temperature=temperature, n_classes=L)
    clf._validate()
    world, start = _world(model), time.time()
    queries, labels = [], []
    with torch.no_grad():
        for x, y in test_loader:
            f = feats(x.to(dev, non_blocking=True), C, S)
            queries.append(f.reshape(f.shape[0], -1).float().clone())
            labels.append(y.to(dev, non_blocking=True).reshape(-1).long())
        if not queries:
            raise ValueError("evaluate_knn: the test loader is empty")
        Q, yq = torch.cat(queries).contiguous(), torch.cat(labels).contiguous()
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

        for x, y in train_loader:
            f = feats(x.to(dev, non_blocking=True), C, S)
            f = f.reshape(f.shape[0], -1)
            y = y.to(dev, non_blocking=True).reshape(-1)
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


def evaluate_classification(model, config, dataloader):
    """evaluation.py:93-128 -> (accuracy, precision, recall, f1, inference_time) (macro averages); summed over the
    ranks like evaluate_clustering."""
    model.eval()
    d = config["data"]
    C, S, ncls = d["num_channels"], d["input_size"], d["num_classes"]
    dev = model.arena.device
    table, pred, start = _Table(ncls, ncls, dev), None, time.time()
    for x, y in dataloader:
        x = x.to(dev, non_blocking=True).reshape(-1, C, S, S)
        y = y.to(dev, non_blocking=True)
        _, logits = model.predict(x)
        if pred is None or pred.numel() != logits.shape[0]:
            pred = torch.empty(logits.shape[0], dtype=torch.int64, device=dev)
        ops.argmax_rows(logits, pred)
        table.add(y.view(-1), pred)                       # cm[true, pred]
    acc, precision, recall, f1 = classification_from_table(table.numpy(_world(model)))
    inference_time = time.time() - start
    print(f"Accuracy: {acc:.3f}, Precision: {precision:.3f}, Recall: {recall:.3f}, F1-score: {f1:.3f}, Inference Time: {inference_time:.3f}")
    return acc, precision, recall, f1, inference_time
