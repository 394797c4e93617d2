"""The pictures evaluation.py writes, drawn from host arrays with matplotlib: no model, no device, no rank.  A function
that writes a file returns its path, or None with one warning when matplotlib is not installed; the caller decides which
rank draws."""
import os

import numpy as np


def _pyplot(who):
    """matplotlib.pyplot, or None with a warning when matplotlib is not installed (no plot is written then)."""
    try:
        import matplotlib.pyplot as plt
        return plt
    except ImportError:
        import warnings
        warnings.warn(f"{who}: matplotlib is not installed; no plot written")
        return None


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


def _draw_map(who, values, label, annotate, path):
    """One value per map cell as an image with a colour bar -> path, or None without matplotlib."""
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


def _save_scatter(who, output_dir, name, points, labels, grid=None, axis_labels=None, **savefig):
    """The tail of the scatter entries: _umap_scatter of points [N, 2] coloured by labels, the axes switched on and named
    when axis_labels = (x, y) is given, the unit grid over it when grid = (prototypes [K, 2], neighbour table) is given
    -> {output_dir}/{name}, saved with the caller's own savefig keywords.  Returns the path, or None without matplotlib."""
    plt = _pyplot(who)
    if plt is None:
        return None
    os.makedirs(output_dir, exist_ok=True)
    _umap_scatter(plt, points, labels)
    if axis_labels is not None:
        plt.axis("on")
        plt.xlabel(axis_labels[0])
        plt.ylabel(axis_labels[1])
    if grid is not None:
        _draw_grid(plt, *grid)
    path = os.path.join(output_dir, name)
    plt.savefig(path, **savefig)
    plt.close()
    return path
