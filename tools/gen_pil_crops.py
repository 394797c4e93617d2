"""Write tests/golden/pil_bicubic_crops.npz: what PIL's `Image.crop(box).resize((S, S), Image.BICUBIC)` makes of a few
uint8 images, for the boxes a random-resized-crop draws and the edge cases (whole image, one pixel wide or high, h != w),
one- and two-stage, and the evaluation geometry (whole image -> R x R -> centre S x S window).  Needs PIL (made with 12.2.0).

Per group g (one launch of vsom_augment_batch in tests/test_data_gpu.py):
    g<k>_src [n_src, C, H, H] uint8, g<k>_index [n] int64, g<k>_params [n, 16] int32 (i1 j1 h1 w1 i2 j2 h2 w2 0 ...; unused
    for evaluation groups), g<k>_geom int32 [S, R, off, uses_params], g<k>_out [n, C, S, S] uint8 (PIL's bytes).

    python tools/gen_pil_crops.py
"""
import math
import os

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sources(rng, C, H):
    noise = rng.integers(0, 256, (C, H, H), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:H]
    smooth = np.stack([(127.5 + 127.5 * np.sin(xx * rng.uniform(0.1, 0.8) + rng.uniform(0, 6)) * np.cos(yy * rng.uniform(0.1, 0.8)))
                       .astype(np.uint8) for _ in range(C)])
    return np.stack([noise, smooth])


def draw_box(rng, H, scale=(0.08, 1.0), ratio=(0.75, 1.3333)):
    area = H * H * rng.uniform(*scale)
    ar = math.exp(rng.uniform(math.log(ratio[0]), math.log(ratio[1])))
    w, h = max(min(int(round(math.sqrt(area * ar))), H), 1), max(min(int(round(math.sqrt(area / ar))), H), 1)
    return int(rng.integers(0, H - h + 1)), int(rng.integers(0, H - w + 1)), h, w


def to_pil(img):
    return Image.fromarray(img[0]) if img.shape[0] == 1 else Image.fromarray(np.ascontiguousarray(img.transpose(1, 2, 0)))


def from_pil(im, C):
    a = np.asarray(im)
    return a[None] if C == 1 else np.ascontiguousarray(a.transpose(2, 0, 1))


def crop_resize(im, box, S):
    i, j, h, w = box
    return im.crop((j, i, j + w, i + h)).resize((S, S), Image.BICUBIC)


def train_group(rng, C, H, S, n_one, n_two):
    src = sources(rng, C, H)
    edge = [(0, 0, H, H), (0, H // 2, H, 1), (H // 3, 0, 1, H), (0, 2, H, 3), (H - 2, H - 5, 2, 5), (1, 1, H - 1, H // 2)]
    boxes = edge + [draw_box(rng, H) for _ in range(n_one - len(edge))]
    params, index, outs = [], [], []
    for t in range(n_one + n_two):
        k = t % 2
        b1 = boxes[t] if t < n_one else draw_box(rng, H)
        b2 = (0, 0, 0, 0)
        im = crop_resize(to_pil(src[k]), b1, S)
        if t >= n_one:
            b2 = [(0, 0, S, S), (S // 2, 0, 1, S)][t - n_one] if t - n_one < 2 else draw_box(rng, S, ratio=(3 / 4, 4 / 3))
            im = crop_resize(im, b2, S)
        params.append(list(b1) + list(b2) + [0] * 8)
        index.append(k)
        outs.append(from_pil(im, C))
    return src, np.array(index, np.int64), np.array(params, np.int32), np.array([S, S, 0, 1], np.int32), np.stack(outs)


def eval_group(rng, C, H, S):
    src = sources(rng, C, H)
    R = int(S / 0.875)
    off = int(round((R - S) / 2.0))
    outs = [from_pil(to_pil(s).resize((R, R), Image.BICUBIC).crop((off, off, off + S, off + S)), C) for s in src]
    return src, np.arange(2, dtype=np.int64), np.zeros((2, 16), np.int32), np.array([S, R, off, 0], np.int32), np.stack(outs)


def main():
    rng = np.random.default_rng(20240611)
    groups = [train_group(rng, 1, 28, 28, 30, 10), train_group(rng, 3, 32, 32, 50, 30), train_group(rng, 3, 64, 32, 30, 10),
              train_group(rng, 3, 64, 64, 10, 6), train_group(rng, 1, 32, 32, 12, 4),
              eval_group(rng, 3, 32, 32), eval_group(rng, 1, 28, 28), eval_group(rng, 3, 64, 64), eval_group(rng, 3, 64, 32)]
    arrays = {}
    for k, g in enumerate(groups):
        for name, a in zip(("src", "index", "params", "geom", "out"), g):
            arrays[f"g{k}_{name}"] = a
    path = os.path.join(ROOT, "tests", "golden", "pil_bicubic_crops.npz")
    np.savez_compressed(path, **arrays)
    print(f"{path}: {sum(len(g[1]) for g in groups)} cases in {len(groups)} groups, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
