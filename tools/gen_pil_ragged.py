"""Write tests/golden/pil_ragged_crops.npz: what PIL makes of rectangular sources of different sizes with
`Image.crop(box).resize((S, S), Image.BICUBIC)` once or twice (training) and with
`Image.resize((OW, OH), Image.BICUBIC).crop(window)` (evaluation: Resize of the shorter side to R, CenterCrop(S)), for the
cases the variable-size pipeline has to get right: both orientations, 1 x W and H x 1 images, boxes one pixel wide or high,
the whole image, a crop side of exactly 8 x its output (33 taps) and one just below 4, upsampling from a handful of pixels,
one channel, crops so tall that a band of output rows is walked in several chunks, and one training and one evaluation case
at S = 224.  Needs PIL (made with 12.2.0).

The sources are not stored: they are tests/ragged_ref.py's formula_image(h, w, c, k).  The file holds `cases` (int32
[n, 20], columns ragged_ref.COLS: shape, formula key, mode, sizes, the geometry, the boxes) and `out` (uint8, PIL's
[c, S, S] bytes of every case, one after the other).

    python tools/gen_pil_ragged.py
"""
import os
import sys

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ragged_ref as G  # noqa: E402


def to_pil(img):
    return Image.fromarray(img[0]) if img.shape[0] == 1 else Image.fromarray(np.ascontiguousarray(img.transpose(1, 2, 0)))


def from_pil(im, C):
    a = np.asarray(im)
    return a[None] if C == 1 else np.ascontiguousarray(a.transpose(2, 0, 1))


def crop_resize(im, box, S):
    i, j, h, w = box
    return im.crop((j, i, j + w, i + h)).resize((S, S), Image.BICUBIC)


def train_case(h, w, c, k, S, box1, box2=None):
    im = crop_resize(to_pil(G.formula_image(h, w, c, k)), box1, S)
    if box2 is not None:
        im = crop_resize(im, box2, S)
    row = [h, w, c, k, G.ONE_CROP if box2 is None else G.TWO_CROPS, S, S, S, S, 0, 0, *box1, *(box2 or (0, 0, 0, 0)), 0]
    return row, from_pil(im, c)


def eval_case(h, w, c, k, S, R):
    # torchvision's Resize(R) + CenterCrop(S), written out
    if w <= h:
        OW, OH = R, int(R * h / w)
    else:
        OH, OW = R, int(R * w / h)
    top, left = int(round((OH - S) / 2.0)), int(round((OW - S) / 2.0))
    im = to_pil(G.formula_image(h, w, c, k)).resize((OW, OH), Image.BICUBIC).crop((left, top, left + S, top + S))
    return [h, w, c, k, G.EVAL, S, R, OH, OW, top, left, 0, 0, h, w, 0, 0, 0, 0, 0], from_pil(im, c)


def main():
    cases = [
        # rectangles of both orientations, inner boxes
        train_case(50, 90, 3, 0, 24, (10, 20, 30, 40)), train_case(90, 50, 3, 1, 24, (20, 5, 60, 40)),
        train_case(57, 91, 3, 2, 16, (3, 11, 50, 75)), train_case(91, 57, 1, 4, 40, (7, 2, 80, 49)),
        # 1 x W and H x 1 images
        train_case(1, 77, 3, 0, 16, (0, 0, 1, 77)), train_case(63, 1, 1, 2, 16, (0, 0, 63, 1)), train_case(1, 1, 3, 6, 16, (0, 0, 1, 1)),
        # boxes one pixel wide / high
        train_case(60, 80, 3, 0, 16, (5, 17, 40, 1)), train_case(60, 80, 3, 3, 16, (33, 2, 1, 70)),
        # the whole image
        train_case(37, 53, 3, 0, 24, (0, 0, 37, 53)), train_case(53, 37, 1, 1, 24, (0, 0, 53, 37)), train_case(24, 24, 3, 2, 24, (0, 0, 24, 24)),
        # a crop side exactly 8 x the output (33 taps), on both axes and on one (no source side exceeds 8 S: the entry's limit)
        train_case(128, 128, 3, 0, 16, (0, 0, 128, 128)), train_case(128, 70, 3, 2, 16, (0, 3, 128, 60)),
        train_case(70, 128, 1, 4, 16, (5, 0, 40, 128)), train_case(192, 192, 3, 6, 24, (0, 1, 192, 191)),
        # just below 4 (the fixed-size kernels' limit) and just above it
        train_case(70, 66, 3, 0, 16, (2, 1, 63, 63)), train_case(70, 66, 3, 2, 16, (2, 0, 65, 66)),
        # upsampling from a handful of pixels
        train_case(5, 3, 3, 0, 40, (0, 0, 5, 3)), train_case(5, 3, 3, 2, 24, (1, 0, 2, 3)), train_case(2, 9, 1, 4, 16, (0, 3, 2, 2)),
        # one channel
        train_case(45, 61, 1, 0, 24, (4, 6, 33, 50)), train_case(45, 61, 1, 3, 16, (0, 0, 45, 61)),
        # tall crops: a band of 32 output rows reads more source rows than the ring holds, so it is walked in several chunks and
        # a chunk boundary falls mid-image (S = 40: 273 rows in the ring, 8 x 32 + 32 needed); the second band is a short one
        train_case(320, 50, 3, 0, 40, (0, 3, 320, 40)), train_case(300, 44, 3, 2, 40, (0, 0, 300, 44)), train_case(320, 41, 1, 4, 40, (1, 0, 319, 41)),
        # two crops
        train_case(80, 60, 3, 0, 24, (8, 4, 60, 50), (3, 5, 17, 14)), train_case(60, 80, 3, 2, 24, (0, 0, 60, 80), (0, 0, 24, 24)),
        train_case(48, 100, 3, 1, 16, (10, 30, 30, 60), (7, 0, 1, 16)), train_case(100, 48, 1, 4, 16, (30, 10, 64, 30), (0, 9, 16, 1)),
        train_case(75, 75, 3, 6, 40, (5, 9, 66, 50), (11, 2, 25, 33)),
        # evaluation: portrait, landscape, square; R = int(S / 0.875); (27 - 24) / 2 and (37 - 24) / 2 are half-integers
        eval_case(70, 50, 3, 0, 24, 27), eval_case(50, 70, 3, 2, 24, 27), eval_case(48, 48, 3, 4, 24, 27),
        eval_case(33, 100, 1, 0, 16, 18), eval_case(100, 33, 3, 1, 16, 18), eval_case(61, 47, 3, 2, 40, 45),
        eval_case(144, 100, 3, 6, 16, 18), eval_case(20, 30, 3, 0, 24, 27),
        # S = 224: two crops from 333 x 250, evaluation of 300 x 400 at 256 / 224
        train_case(333, 250, 3, 0, 224, (21, 13, 290, 215), (30, 18, 170, 190)),
        eval_case(300, 400, 3, 1, 224, 256),
    ]
    table = np.array([row for row, _ in cases], np.int32)
    assert table.shape[1] == len(G.COLS)
    out = np.concatenate([o.reshape(-1) for _, o in cases])
    path = G.GOLDEN_FILE
    np.savez_compressed(path, cases=table, out=out)
    print(f"{path}: {len(cases)} cases, {os.path.getsize(path)} bytes (PIL {PIL.__version__})")


if __name__ == "__main__":
    main()
