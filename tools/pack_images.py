"""Decode an ImageFolder-style tree once, on the host, into the ragged .npz that vit_som_amd.data.RaggedDeviceDataset.from_npz
and `python -m vit_som_amd.train --data-npz` read: every image as uint8 planar [C][H][W] in one flat buffer.

    python tools/pack_images.py ROOT OUT.npz [--gray] [--test-fraction 0.1] [--seed 0]

ROOT/<class>/<file>: the sorted class sub-directories give the labels 0, 1, ..., the files of a class are taken in sorted
order.  Files are decoded with PIL: Image.open(f).convert("RGB") (or "L" with --gray).  --test-fraction F moves a seeded
random fraction F of the images into test_data / test_offsets / test_shapes / test_labels.  The images must already be on
this machine: nothing is fetched.
"""
import argparse
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")


def list_tree(root):
    """[(path, label)] and the class names, in ImageFolder's order."""
    classes = sorted(d for d in os.listdir(root) if os.path.isdir(os.path.join(root, d)))
    if not classes:
        raise SystemExit(f"pack_images: no class directory under {root}")
    files = []
    for label, name in enumerate(classes):
        for f in sorted(os.listdir(os.path.join(root, name))):
            if f.lower().endswith(EXTENSIONS):
                files.append((os.path.join(root, name, f), label))
    if not files:
        raise SystemExit(f"pack_images: no image file under {root}")
    return files, classes


def pack(root, out, gray=False, test_fraction=0.0, seed=0):
    from vit_som_amd.data import pack_ragged                   # the layout lives in one place
    files, classes = list_tree(root)
    mode = "L" if gray else "RGB"
    images = []
    for path, _ in files:
        with Image.open(path) as im:
            images.append(np.asarray(im.convert(mode)))
    labels = np.array([label for _, label in files], np.int64)
    test = np.zeros(len(files), bool)
    if test_fraction > 0:
        k = min(max(int(round(test_fraction * len(files))), 1), len(files) - 1)
        test[np.random.default_rng(seed).permutation(len(files))[:k]] = True
    arrays = {"channels": np.int64(1 if gray else 3), "classes": np.array(classes)}
    for prefix, keep in (("", ~test), ("test_", test)):
        if keep.any():
            data, offsets, shapes, _ = pack_ragged([im for im, k in zip(images, keep) if k], layout=None if gray else "HWC")
            arrays.update({prefix + "data": data, prefix + "offsets": offsets, prefix + "shapes": shapes, prefix + "labels": labels[keep]})
    np.savez(out, **arrays)
    return arrays


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("root")
    ap.add_argument("out")
    ap.add_argument("--gray", action="store_true", help='decode with convert("L"): one channel')
    ap.add_argument("--test-fraction", type=float, default=0.0)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    arrays = pack(a.root, a.out, a.gray, a.test_fraction, a.seed)
    n, nt = len(arrays["labels"]), len(arrays.get("test_labels", ()))
    print(f"{a.out}: {n} images ({arrays['data'].nbytes / 1e6:.1f} MB), {nt} held out, {len(arrays['classes'])} classes, "
          f"sides up to {int(arrays['shapes'].max())}")


if __name__ == "__main__":
    main()
