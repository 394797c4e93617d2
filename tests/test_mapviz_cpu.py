"""The map pictures without a GPU: host-side argument checks of vsom_proto_mosaic / vsom_last_label, the drawing helpers on
given arrays, and the float64 restatements the GPU tests (test_mapviz_gpu.py) compare the kernels with."""
import os
import warnings

import numpy as np
import pytest


# ------------------------------------------------------------------ restatements (float64 numpy)
def unpatchify_np(pred, n, p, C):
    """pred [chunk, n + 1, p*p*C] -> [chunk, C, S, S]: the CLS row dropped, vit.py:141-153 (nhwpqc -> nchpwq)."""
    g = int(round(n ** 0.5))
    x = pred[:, 1:].reshape(pred.shape[0], g, g, p, p, C)
    return np.einsum("nhwpqc->nchpwq", x).reshape(pred.shape[0], C, g * p, g * p)


def mosaic_restatement(images, rows, cols, gap):
    """What the canvas must hold for images [K, C, S, S] (any float dtype; computed in float64).  Returns
    (levels uint8 [H, W, 3], margin float64 [H, W, 3]): the level floor(255 t + 0.5) with t = clip(v, 0, 1) (C == 3) or
    (v - min) / (max - min) over the image (C == 1, 0 for a constant image), and the distance of 255 t from the nearest
    rounding boundary k + 0.5 in levels (0.5 on the gap pixels, which are 255)."""
    v = np.asarray(images, dtype=np.float64)
    K, C, S, _ = v.shape
    assert K == rows * cols and C in (1, 3)
    if C == 3:
        t = np.clip(v, 0.0, 1.0)
    else:
        lo, hi = v.min(axis=(1, 2, 3), keepdims=True), v.max(axis=(1, 2, 3), keepdims=True)
        span = np.where(hi > lo, hi - lo, 1.0)
        t = np.repeat(np.where(hi > lo, (v - lo) / span, 0.0), 3, axis=1)
    x = 255.0 * t + 0.5
    level, margin = np.floor(x), np.abs(x - np.round(x))
    H, W = rows * S + (rows - 1) * gap, cols * S + (cols - 1) * gap
    levels, margins = np.full((H, W, 3), 255, dtype=np.uint8), np.full((H, W, 3), 0.5)
    for k in range(K):
        r, c = divmod(k, cols)
        y0, x0 = r * (S + gap), c * (S + gap)
        levels[y0:y0 + S, x0:x0 + S] = level[k].transpose(1, 2, 0).astype(np.uint8)
        margins[y0:y0 + S, x0:x0 + S] = margin[k].transpose(1, 2, 0)
    return levels, margins


def check_canvas(got, images, rows, cols, gap, zone, max_excused):
    """got == the restatement wherever 255 t is more than `zone` levels from a rounding boundary, within one level
    everywhere, and the pixels so excused are at most `max_excused` of all.  Returns the excused fraction."""
    levels, margins = mosaic_restatement(images, rows, cols, gap)
    assert got.shape == levels.shape and got.dtype == np.uint8
    diff = np.abs(got.astype(np.int64) - levels.astype(np.int64))
    excused = margins <= zone
    frac = float(excused.mean())
    print(f"canvas {rows}x{cols} gap {gap}: {int((diff != 0).sum())} of {diff.size} values differ, max {int(diff.max())}, "
          f"{frac:.4%} within {zone} of a boundary")
    assert diff.max() <= 1, int(diff.max())
    assert (diff[~excused] == 0).all(), int((diff[~excused] != 0).sum())
    assert frac <= max_excused, frac
    return frac


def last_label_loop(bmus, labels, rows, cols):
    """tools/evaluation.py:253-258."""
    heatmap = np.zeros((rows, cols), dtype=np.int64)
    for b, y in zip(bmus, labels):
        r, c = divmod(int(b), cols)
        heatmap[r, c] = y
    return heatmap


def test_restatement_on_known_values():
    img = np.zeros((2, 1, 2, 2))
    img[0, 0] = [[0.0, 1.0], [2.0, 4.0]]                     # range 4: levels 0, 63.75 -> 64, 127.5 -> 128, 255
    img[1, 0] = 7.0                                          # constant -> 0
    lv, mg = mosaic_restatement(img, 1, 2, 1)
    assert lv.shape == (2, 5, 3)
    assert lv[:, :2, 0].tolist() == [[0, 64], [128, 255]] and (lv[:, 2] == 255).all() and (lv[:, 3:] == 0).all()
    assert mg[1, 0, 0] == 0.0 and abs(mg[0, 1, 0] - 0.25) < 1e-12
    rgb = np.array([-3.0, 0.5, 9.0]).reshape(1, 3, 1, 1)
    assert mosaic_restatement(rgb, 1, 1, 0)[0].tolist() == [[[0, 128, 255]]]
    assert last_label_loop([0, 5, 0], [3, 4, 9], 2, 3).tolist() == [[9, 0, 0], [0, 0, 4]]


# ------------------------------------------------------------------ the C-ABI on the host
def test_new_entries_reject_bad_calls_on_the_host():
    from vit_som_amd._lib import last_error, lib
    ok = dict(pred=16, chunk=2, n=4, p=2, C=1, images=16, canvas=16, k0=0, K=6, rows=2, cols=3, gap=1)

    def mosaic(**kw):
        a = {**ok, **kw}
        return lib.vsom_proto_mosaic(a["pred"], a["chunk"], a["n"], a["p"], a["C"], a["images"], a["canvas"], a["k0"], a["K"],
                                     a["rows"], a["cols"], a["gap"], None)
    assert mosaic(pred=None) == -1 and "null" in last_error()
    assert mosaic(images=None, canvas=None) == -1
    assert mosaic(C=2) == -3 and mosaic(C=4) == -3 and "channels" in last_error()
    assert mosaic(rows=2, cols=2) == -1 and "map" in last_error()
    assert mosaic(gap=-1) == -1 and "gap" in last_error()
    assert mosaic(n=5) == -1 and "square" in last_error()
    assert mosaic(k0=5) == -1                                # k0 + chunk > K
    assert mosaic(chunk=0) == -1 and mosaic(p=0) == -1
    assert lib.vsom_last_label(None, 16, 4, 0, 6, 16, 16, None) == -1 and "null" in last_error()
    assert lib.vsom_last_label(16, 16, 4, 0, 6, None, 16, None) == -1
    assert lib.vsom_last_label(16, 16, 4, 0, 6, 16, None, None) == -1
    assert lib.vsom_last_label(16, 16, 4, -1, 6, 16, 16, None) == -1
    assert lib.vsom_last_label(16, 16, 4, 0, 0, 16, 16, None) == -1
    assert lib.vsom_last_label(16, 16, 4, 2 ** 31 - 4, 6, 16, 16, None) == -3 and "2^31" in last_error()
    assert lib.vsom_last_label(16, 16, 0, 0, 6, 16, 16, None) == 0          # nothing to fold, nothing launched


def test_public_names():
    import vit_som_amd
    ev = vit_som_amd.evaluation
    for name in ("visualize_decoded_prototypes", "decode_prototype", "visualize_label_heatmap", "decoded_prototype_canvas"):
        assert callable(getattr(ev, name))
    assert vit_som_amd.ViTSOM.current_epoch == 0 and vit_som_amd.DESOM.current_epoch == 0
    assert vit_som_amd.ViTClassifier.current_epoch == 0


# ------------------------------------------------------------------ drawing, given arrays
def _have_matplotlib():
    try:
        import matplotlib  # noqa: F401
        return True
    except ImportError:
        return False


def test_drawing_helpers_write_the_reference_file_names(tmp_path):
    from vit_som_amd.evaluation import draw_decoded_prototypes, draw_label_heatmap
    rng = np.random.default_rng(0)
    canvas = rng.integers(0, 256, size=(3 * 8 + 2, 5 * 8 + 4, 3), dtype=np.uint8)
    heat = rng.integers(0, 10, size=(3, 5)).astype(np.int64)
    out = tmp_path / "plots" / "nested"
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        a = draw_decoded_prototypes(canvas, str(out), "vit_som", 7)
        b = draw_label_heatmap(heat, str(out), "desom", 0)
    if _have_matplotlib():
        assert a == str(out / "vit_som_epoch_7_decoded_prototypes.png") and os.path.getsize(a) > 0
        assert b == str(out / "desom_epoch_0_label_heatmap.png") and os.path.getsize(b) > 0
    else:
        assert a is None and b is None and len(w) == 2 and not out.exists()


@pytest.mark.parametrize("arch,reduced", [("desom", False), ("vit", False), ("vit_som", True)])
def test_decoded_prototypes_refused_like_the_reference(arch, reduced, capsys):
    """evaluation.py:162-164: the message and None, before anything of the model is touched."""
    from vit_som_amd.evaluation import visualize_decoded_prototypes

    class Model:
        def eval(self):
            return self
    hp = {"model_arch": arch}
    if arch != "vit":
        hp["som"] = {"use_reduced": True} if reduced else {}
    assert visualize_decoded_prototypes(Model(), {"hyperparameters": hp, "data": {}}) is None
    assert "Visualization supported only for vit_som with use_reduced=False." in capsys.readouterr().out
