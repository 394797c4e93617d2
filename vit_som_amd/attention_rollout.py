"""Attention rollout (Abnar and Zuidema 2020; head fusion as in the vit-explain recipe): which part of an image the
encoder looked at, and -- what no other tool offers -- what the samples won by each SOM unit look at.

The quantity.  For one block with saved qkv, P_h[i, j] = softmax_j(q_i . k_j / sqrt(hd)), F = the mean, max or min of the
P_h over the heads, and A[i, j] = (alpha F[i, j] + (1 - alpha) [i == j]) / (alpha sum_j F[i, j] + (1 - alpha)) with
residual = 1 - alpha.  The rollout of query weights w [B, N] over the blocks start_layer .. L - 1 is
w A_{L-1} A_{L-2} ... A_{start_layer}: one query row of the product of the matrices, computed as a vector-matrix chain
(`ops.attention_rollout`, csrc/attention_rollout.hip) from the qkv buffers a forward leaves on the device.  The state is
[B, N]; no N x N matrix exists anywhere.  Every row of every A sums to 1, so the result sums to sum(w).  With alpha = 1,
start_layer = L - 1, the CLS query and "mean" it is the head-mean CLS attention of the last block (the DINO picture).

Not built, on purpose: vit-explain's discard_ratio (a selection over N^2 entries per sample), gradient-weighted rollout,
the full N x N rollout matrix, decoder blocks, per-head maps, attention distance and entropy per layer, a sharded
evaluate_attention, and the matrix cores for the score products.

The model methods (ViTAutoencoder / ViTSOM / ViTClassifier .attention_rollout) and the evaluation entries
(evaluate_attention, visualize_attention_rollout, visualize_attention_map) all end here."""
import os
import time
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import ops

HEAD_FUSIONS = ("mean", "max", "min")
QUERIES = ("cls", "patches")


# ---------------------------------------------------------------- arguments
def check_arguments(who, head_fusion, residual, start_layer, depth):
    """The refusals shared by every entry -> alpha = 1 - residual."""
    if head_fusion not in HEAD_FUSIONS:
        raise ValueError(f"{who}: head_fusion must be one of 'mean', 'max', 'min', got {head_fusion!r}")
    if isinstance(residual, bool) or not isinstance(residual, (int, float)) or not 0.0 <= float(residual) < 1.0:
        raise ValueError(f"{who}: residual must be a number in [0, 1) (the weight of the identity; 0.5 is the usual rollout), "
                         f"got {residual!r}")
    if isinstance(start_layer, bool) or not isinstance(start_layer, (int, np.integer)) or not 0 <= int(start_layer) < depth:
        raise ValueError(f"{who}: start_layer must be an int in [0, {depth}) (the first encoder block of the chain), "
                         f"got {start_layer!r}")
    return 1.0 - float(residual)


def _bad_query(who, query, N):
    got = f"a {query.dtype} tensor of shape {tuple(query.shape)}" if isinstance(query, torch.Tensor) else repr(query)
    return ValueError(f"{who}: query must be 'cls', 'patches', a token index in [0, {N}) or a non-negative float tensor of "
                      f"shape [{N}] or [B, {N}], got {got}")


def patch_grid(vit):
    """(gh, gw) of the ViT's patch grid."""
    g = vit.img_size // vit.patch_embed.patch_size[0]
    return g, g


def query_weights(query, B, N, device, who="attention_rollout", check_sign=True):
    """The query weights w f32 [B, N] on `device`.  'cls': all weight on token 0.  'patches': 1 / n on each of the n = N - 1
    patch tokens, 0 on CLS.  An int: that token.  A floating-point tensor [N] or [B, N]: taken as it is (check_sign: one
    host read refuses a negative entry)."""
    if isinstance(query, torch.Tensor):
        if not query.is_floating_point() or query.dim() not in (1, 2) or query.shape[-1] != N or (query.dim() == 2 and query.shape[0] != B):
            raise _bad_query(who, query, N)
        w = query.detach().to(device=device, dtype=torch.float32)
        if check_sign and bool((~(w >= 0)).any().item()):
            raise ValueError(f"{who}: query must be non-negative (and not NaN) everywhere; it holds the weight of every token")
        return (w.unsqueeze(0).expand(B, N) if w.dim() == 1 else w).contiguous()
    w = torch.zeros(B, N, dtype=torch.float32, device=device)
    if isinstance(query, str):
        if query == "cls":
            w[:, 0] = 1.0
        elif query == "patches" and N > 1:
            w[:, 1:] = 1.0 / (N - 1)
        else:
            raise _bad_query(who, query, N)
        return w
    if isinstance(query, bool) or not isinstance(query, (int, np.integer)) or not 0 <= int(query) < N:
        raise _bad_query(who, query, N)
    w[:, int(query)] = 1.0
    return w


# ---------------------------------------------------------------- the chain on a ViT's buffers
def rollout_from_acts(vit, a, query="cls", head_fusion="mean", residual=0.5, start_layer=0, who="attention_rollout", check_sign=True):
    """[B, N] f32 from the qkv buffers of the encoder blocks in `a`, which a full encoder forward has just filled
    (ViTAutoencoder._rollout).  Launches only; nothing is read back unless a tensor query is sign-checked."""
    alpha = check_arguments(who, head_fusion, residual, start_layer, len(vit.blocks))
    w = query_weights(query, a.B, a.N, a.device, who, check_sign)
    H = vit.num_heads
    qkvs = [L.qkv for L in a.enc[int(start_layer):]]
    return ops.attention_rollout(qkvs, w, H, vit.embed_dim // H, head_fusion, alpha)


def patch_map(vit, r):
    """Columns 1: of a rollout [B, N] as [B, gh, gw] on the patch grid."""
    gh, gw = patch_grid(vit)
    if r.dim() != 2 or r.shape[1] != gh * gw + 1:
        raise ValueError(f"patch_map: expected a rollout of shape [B, {gh * gw + 1}], got {tuple(r.shape)}")
    return r[:, 1:].reshape(r.shape[0], gh, gw)


def patch_distribution(r):
    """(p [B, n] f32 contiguous, cls share [B]): the patch part of a rollout [B, N] renormalised to sum 1 per sample, and the
    share of the sample's mass that sat on the CLS column before that."""
    patches = r[:, 1:]
    mass = patches.sum(dim=1, keepdim=True)
    cls = r[:, 0] / (r[:, 0] + mass[:, 0])
    return (patches / mass).contiguous(), cls


# ---------------------------------------------------------------- evaluation
@dataclass
class AttentionReport:
    """What evaluate_attention returns.  A map is a distribution over the gh x gw patch grid (sums to 1).  class_sums /
    unit_sums are the fp64 sums the maps were divided out of, each a chain over its samples in loader order -- bit for bit
    np.add.at of the per-sample maps."""
    mean_map: np.ndarray                      # [gh, gw]
    class_maps: np.ndarray                    # [C, gh, gw]; zeros for a class without samples
    class_counts: np.ndarray                  # [C] int64
    unit_maps: Optional[np.ndarray]           # [K, gh, gw]; None for a classifier
    unit_counts: Optional[np.ndarray]         # [K] int64
    cls_mass: float                           # mean share of the mass left on the CLS column before the renormalisation
    entropy: float                            # mean Shannon entropy of the per-sample patch map / log n; 1 means uniform
    query: object
    head_fusion: str
    residual: float
    start_layer: int
    n_samples: int
    inference_time: float
    class_sums: np.ndarray = None             # [C, gh, gw] float64
    unit_sums: Optional[np.ndarray] = None    # [K, gh, gw] float64


def _attention_model(model, config, who):
    """-> (the model's ViTAutoencoder, is it a vit_som).  The config is asked first: a DESOM model is refused with the reason."""
    name = config.get("hyperparameters", {}).get("model_arch")
    if name == "desom":
        raise ValueError(f"{who}: a DESOM model has no attention layers (its encoder is fully connected); attention rollout "
                         f"needs a vit_som or a vit model")
    if name not in ("vit_som", "vit") or not hasattr(model, "_vit"):
        raise ValueError(f"{who}: needs a vit_som or a vit model; got {type(model).__name__} with model_arch {name!r}")
    return model._vit, name == "vit_som"


def _default_query(model, is_som, query):
    if query is not None:
        return query
    return ("cls" if model.use_reduced else "patches") if is_som else "cls"


def _loader_query(query, N, device, who):
    """A query for a whole loader: a [B, N] tensor cannot follow the batches; a [N] tensor is sign-checked once, here."""
    if isinstance(query, torch.Tensor):
        if query.dim() != 1:
            raise ValueError(f"{who}: a tensor query must have shape [{N}] here (one weight per token for every batch), got "
                             f"{tuple(query.shape)}")
        return query_weights(query, 1, N, device, who)[0].clone()
    return query


def _divide(sums, counts):
    out = np.zeros_like(sums)
    has = counts > 0
    out[has] = sums[has] / counts[has][:, None, None]
    return out


@torch.no_grad()
def evaluate_attention(model, config, dataloader, query=None, head_fusion="mean", residual=0.5, start_layer=0, num_labels=None):
    """Attention rollout over a loader -> AttentionReport: the mean patch map, one per class and -- for a vit_som -- one per
    SOM unit (what the samples a unit wins look at), with the mean CLS share and the mean normalised entropy of the maps.
    query None: what the SOM is fed ('patches', or 'cls' with use_reduced); 'cls' for a vit classifier.  One loader pass and
    no host synchronisation inside it: for a vit_som the rollout reads the buffers predict() has just filled (no second
    encoder pass); a vit classifier runs a full encode, because its pruned last block keeps no qkv for all queries.  The
    folds are `ops.som_batch_accumulate`: fp64, every (class or unit, cell) one chain over its samples in loader order.
    Labels must lie in [0, num_labels) (default data.num_classes, 256 when the config has none).
    model.world_size > 1 is refused with ValueError: the per-rank sums would have to be exchanged in a fixed order, and that
    path has not been built."""
    from . import evaluation as E                         # its loader pass and model adapter; evaluation imports this module
    who = "evaluate_attention"
    vit, is_som = _attention_model(model, config, who)
    if E._world(model) > 1:
        raise ValueError(f"{who}: model.world_size > 1 is not supported; run it on one rank")
    check_arguments(who, head_fusion, residual, start_layer, len(vit.blocks))
    arch = E._Arch(model, config, who)
    dev = arch.device
    gh, gw = patch_grid(vit)
    n, N = gh * gw, gh * gw + 1
    query = _default_query(model, is_som, query)
    q = _loader_query(query, N, dev, who)
    query_weights(q, 1, N, dev, who, check_sign=False)     # refuses a bad query before any batch is read
    C = E._label_count(config, num_labels, False)
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)          # noqa: E731
    i64 = lambda *s: torch.zeros(*s, dtype=torch.int64, device=dev)            # noqa: E731
    class_sums, class_counts = f64(C, n), i64(C)
    K = model.som_layer.n_prototypes if is_som else 0
    unit_sums, unit_counts = (f64(K, n), i64(K)) if is_som else (None, None)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    totals = f64(2)                                        # the sums of the CLS shares and of the entropies
    seen = 0
    start = time.time()
    batches = arch.batches(dataloader, arch.images)
    for x, y in batches:
        if is_som:
            bmu, _ = model.predict(x)
            r = rollout_from_acts(vit, vit._buffers_for(x.shape[0], x.device), q, head_fusion, residual, start_layer, who, False)
        else:
            bmu, r = None, vit.attention_rollout(x, q, head_fusion, residual, start_layer, _check_sign=False)
        p, cls = patch_distribution(r)
        ops.som_batch_accumulate(p, y, class_sums, class_counts, accumulate=True, bad=bad)
        if is_som:
            ops.som_batch_accumulate(p, bmu.reshape(-1).long().contiguous(), unit_sums, unit_counts, accumulate=True, bad=bad)
        totals[0] += cls.double().sum()
        totals[1] -= torch.xlogy(p, p).double().sum()
        seen += x.shape[0]
    if not seen:
        raise ValueError(f"{who}: the loader is empty")
    n_bad = int(bad.item())
    if n_bad:
        raise ValueError(f"{who}: {n_bad} labels fell outside [0, {C}); pass num_labels= for larger label sets")
    cls_mass, ent = (float(v) / seen for v in totals.cpu().numpy())
    entropy = ent / np.log(n) if n > 1 else 1.0
    cs, cc = class_sums.cpu().numpy().reshape(C, gh, gw), class_counts.cpu().numpy()
    classes = int(config["data"].get("num_classes", 0))
    keep = C if num_labels else max(classes, (int(np.flatnonzero(cc).max()) + 1) if cc.any() else 0)
    cs, cc = cs[:keep], cc[:keep]
    us = uc = um = None
    if is_som:
        us, uc = unit_sums.cpu().numpy().reshape(K, gh, gw), unit_counts.cpu().numpy()
        um = _divide(us, uc)
    inference_time = time.time() - start
    report = AttentionReport(mean_map=cs.sum(axis=0) / seen, class_maps=_divide(cs, cc), class_counts=cc, unit_maps=um, unit_counts=uc,
                             cls_mass=cls_mass, entropy=float(entropy), query=query, head_fusion=head_fusion, residual=float(residual),
                             start_layer=int(start_layer), n_samples=seen, inference_time=float(inference_time), class_sums=cs,
                             unit_sums=us)
    print(f"Attention rollout ({head_fusion}, residual {float(residual):g}, from block {int(start_layer)}): "
          f"Rollout entropy: {report.entropy:.3f}, CLS mass: {report.cls_mass:.3f}, Inference Time: {inference_time:.3f}")
    return report


# ---------------------------------------------------------------- figures
def _upsample(m, S):
    """A [gh, gw] map as an [S, S] image, every cell a block of pixels."""
    gh, gw = m.shape
    return np.kron(m, np.ones((S // gh, S // gw)))


def draw_attention_rollout(images, maps, path, who="visualize_attention_rollout"):
    """Two rows per strip: the images [n, S, S, C] (host, any range; shown min-max scaled) and the same with their maps
    [n, gh, gw] laid over them -> path, or None without matplotlib."""
    from .plots import _pyplot
    plt = _pyplot(who)
    if plt is None:
        return None
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    n = len(images)
    fig, axes = plt.subplots(2, n, figsize=(1.6 * n, 3.4), squeeze=False)
    for k in range(n):
        img = images[k].astype(np.float64)
        lo, hi = float(img.min()), float(img.max())
        img = (img - lo) / (hi - lo) if hi > lo else np.zeros_like(img)
        img = img[..., 0] if img.shape[-1] == 1 else img[..., :3]
        for row in (0, 1):
            ax = axes[row][k]
            ax.imshow(img, cmap="gray" if img.ndim == 2 else None, interpolation="nearest")
            ax.axis("off")
        m = _upsample(maps[k], img.shape[0])
        axes[1][k].imshow(m, cmap="inferno", alpha=0.6, interpolation="bilinear", extent=(-0.5, img.shape[1] - 0.5, img.shape[0] - 0.5, -0.5))
    fig.savefig(path, bbox_inches="tight", dpi=150)
    plt.close(fig)
    return path


def draw_attention_map(unit_maps, unit_counts, map_size, class_maps, class_counts, path, who="visualize_attention_map"):
    """The K unit maps as one mosaic on the SOM grid (a unit without samples stays empty) above a row of the per-class maps
    -> path, or None without matplotlib.  unit_maps None (a classifier): the row of class maps alone."""
    from .plots import _pyplot
    plt = _pyplot(who)
    if plt is None:
        return None
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    shown = [c for c in range(len(class_counts)) if class_counts[c] > 0][:16]
    rows = (1 if unit_maps is not None else 0) + (1 if shown else 0)
    fig = plt.figure(figsize=(10, 8 if unit_maps is not None else 2.5))
    grid = fig.add_gridspec(max(rows, 1), 1, height_ratios=([6] if unit_maps is not None else []) + ([1] if shown else []) or [1])
    if unit_maps is not None:
        mh, mw = int(map_size[0]), int(map_size[1])
        gh, gw = unit_maps.shape[1:]
        canvas = np.full((mh * (gh + 1) - 1, mw * (gw + 1) - 1), np.nan)
        for u in range(mh * mw):
            if unit_counts[u] > 0:
                r, c = divmod(u, mw)
                top = unit_maps[u].max()
                canvas[r * (gh + 1):r * (gh + 1) + gh, c * (gw + 1):c * (gw + 1) + gw] = unit_maps[u] / top if top > 0 else 0.0
        ax = fig.add_subplot(grid[0])
        ax.imshow(canvas, cmap="inferno", interpolation="nearest", vmin=0.0, vmax=1.0)
        ax.set_title("what the samples of each SOM unit look at (each cell scaled to its own maximum)", fontsize=9)
        ax.axis("off")
    if shown:
        sub = grid[rows - 1].subgridspec(1, len(shown))
        for k, c in enumerate(shown):
            ax = fig.add_subplot(sub[k])
            ax.imshow(class_maps[c], cmap="inferno", interpolation="nearest")
            ax.set_title(f"class {c}", fontsize=7)
            ax.axis("off")
    fig.savefig(path, bbox_inches="tight", dpi=150)
    plt.close(fig)
    return path


@torch.no_grad()
def visualize_attention_rollout(model, config, dataloader, n_images=16, output_dir="experiments/plots", query=None, head_fusion="mean",
                                residual=0.5, start_layer=0):
    """The first n_images images of the loader with their rollout map laid over them ->
    {output_dir}/{model_arch}_attention_rollout.png (rank 0 draws; skipped with a warning when matplotlib is missing).
    Returns (maps [n, gh, gw] float32 host array of the patch distributions, the path or None)."""
    from . import evaluation as E
    who = "visualize_attention_rollout"
    vit, is_som = _attention_model(model, config, who)
    check_arguments(who, head_fusion, residual, start_layer, len(vit.blocks))
    if isinstance(n_images, bool) or not isinstance(n_images, (int, np.integer)) or n_images < 1:
        raise ValueError(f"{who}: n_images must be an int >= 1, got {n_images!r}")
    arch = E._Arch(model, config, who)
    gh, gw = patch_grid(vit)
    q = _loader_query(_default_query(model, is_som, query), gh * gw + 1, arch.device, who)
    images, maps, have = [], [], 0
    batches = arch.batches(dataloader, arch.images, labels=False)
    for x, _ in batches:
        x = x[:n_images - have]
        r = vit.attention_rollout(x, q, head_fusion, residual, start_layer, _check_sign=False)
        maps.append(patch_distribution(r)[0].reshape(-1, gh, gw).cpu().numpy())
        images.append(x.float().permute(0, 2, 3, 1).cpu().numpy())
        have += x.shape[0]
        if have >= n_images:
            break
    if not have:
        raise ValueError(f"{who}: the loader is empty")
    maps, images = np.concatenate(maps), np.concatenate(images)
    path = None
    if E._rank(model) == 0:
        path = draw_attention_rollout(images, maps, os.path.join(output_dir, f"{arch.name}_attention_rollout.png"), who)
    return maps, path


@torch.no_grad()
def visualize_attention_map(model, config, dataloader, output_dir="experiments/plots", query=None, head_fusion="mean", residual=0.5,
                            start_layer=0, num_labels=None):
    """evaluate_attention's unit maps as one mosaic on the SOM grid -- what each cell of the map looks at -- over a row of the
    per-class maps -> {output_dir}/{model_arch}_attention_map.png (rank 0 draws; skipped with a warning when matplotlib is
    missing).  Returns (the AttentionReport, the path or None)."""
    from . import evaluation as E
    who = "visualize_attention_map"
    _attention_model(model, config, who)
    report = evaluate_attention(model, config, dataloader, query, head_fusion, residual, start_layer, num_labels)
    path = None
    if E._rank(model) == 0:
        name = config["hyperparameters"]["model_arch"]
        map_size = model.som_layer.map_size if report.unit_maps is not None else None
        path = draw_attention_map(report.unit_maps, report.unit_counts, map_size, report.class_maps, report.class_counts,
                                  os.path.join(output_dir, f"{name}_attention_map.png"), who)
    return report, path
