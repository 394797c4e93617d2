"""What the variable-size data-pipeline tests compare against (tests/test_ragged_cpu.py, tests/test_ragged_gpu.py): the
formula images tools/gen_pil_ragged.py fed to PIL (the golden file stores no source), and a numpy restatement of the
transform built on data_ref.coeffs, generalised to a rectangular output of which a window is computed."""
import functools
import os

import numpy as np

import data_ref as R

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pil_ragged_crops.npz")
# columns of the golden file's `cases` table (int32): the source formula_image(h, w, c, k); mode 0 = one crop, 1 = two crops,
# 2 = evaluation; the resize's output OH x OW and the S x S window at (top, left); box 1 (on h x w), box 2 (on S x S)
COLS = ("h", "w", "c", "k", "mode", "S", "R", "OH", "OW", "top", "left", "i1", "j1", "h1", "w1", "i2", "j2", "h2", "w2", "pad")
ONE_CROP, TWO_CROPS, EVAL = 0, 1, 2


def formula_image(h, w, c, k):
    """uint8 [c, h, w] from integers alone.  Even k: a hash of (channel, y, x, k), every byte unrelated to its neighbours;
    odd k: diagonal ramps with hard edges every 256 levels."""
    ch, y, x = np.meshgrid(np.arange(c, dtype=np.uint64), np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64), indexing="ij")
    k = np.uint64(k)
    if int(k) % 2 == 0:
        v = (y * np.uint64(131071) + x * np.uint64(8191) + ch * np.uint64(524287) + k * np.uint64(127) + np.uint64(12345)) & np.uint64(0xFFFFFFFF)
        v = (v ^ (v >> np.uint64(15))) * np.uint64(2246822519) & np.uint64(0xFFFFFFFF)
        v = (v ^ (v >> np.uint64(13))) * np.uint64(3266489917) & np.uint64(0xFFFFFFFF)
        v = v ^ (v >> np.uint64(16))
        return (v & np.uint64(255)).astype(np.uint8)
    return ((y * (np.uint64(3) + k) + x * (np.uint64(5) + ch) + ch * np.uint64(60) + k * np.uint64(17)) & np.uint64(255)).astype(np.uint8)


coeffs = functools.lru_cache(maxsize=None)(R.coeffs)


def resize_window(img, OH, OW, top, left, S):
    """The S x S window at (top, left) of uint8 [C, h, w] resized to OH x OW: horizontal pass, 8-bit intermediate, vertical."""
    C, h, w = img.shape
    src = img.astype(np.int64)
    half = 1 << (R.PREC - 1)
    tmp = np.empty((C, h, S), np.int64)
    ch = coeffs(w, OW)
    for xx in range(S):
        x0, k = ch[left + xx]
        tmp[:, :, xx] = np.clip((half + (src[:, :, x0:x0 + len(k)] * k).sum(-1)) >> R.PREC, 0, 255)
    res = np.empty((C, S, S), np.int64)
    cv = coeffs(h, OH)
    for yy in range(S):
        y0, k = cv[top + yy]
        res[:, yy, :] = np.clip((half + (tmp[:, y0:y0 + len(k), :] * k[None, :, None]).sum(1)) >> R.PREC, 0, 255)
    return res.astype(np.uint8)


def eval_geometry(h, w, Rsz, S):
    """torchvision's Resize(Rsz) of an h x w image (shorter side -> Rsz, longer -> int(Rsz * long / short)) and
    CenterCrop(S) (top = int(round((OH - S) / 2.0)), left likewise; Python's round is half to even) -> (OH, OW, top, left)."""
    short, long_ = (w, h) if w <= h else (h, w)
    new_short, new_long = Rsz, int(Rsz * long_ / short)
    OW, OH = (new_short, new_long) if w <= h else (new_long, new_short)
    return OH, OW, int(round((OH - S) / 2.0)), int(round((OW - S) / 2.0))


def train_u8(src, box1, box2, S):
    """Crop box1 of src -> S x S, then (box2 not None) box2 of that -> S x S."""
    i, j, h, w = (int(v) for v in box1)
    img = resize_window(src[:, i:i + h, j:j + w], S, S, 0, 0, S)
    if box2 is not None:
        i, j, h, w = (int(v) for v in box2)
        img = resize_window(img[:, i:i + h, j:j + w], S, S, 0, 0, S)
    return img


def eval_u8(src, Rsz, S):
    OH, OW, top, left = eval_geometry(src.shape[1], src.shape[2], Rsz, S)
    return resize_window(src, OH, OW, top, left, S)


def case_u8(row):
    """The restatement's bytes for one row of the golden file's `cases` table."""
    c = dict(zip(COLS, (int(v) for v in row)))
    src = formula_image(c["h"], c["w"], c["c"], c["k"])
    if c["mode"] == EVAL:
        return resize_window(src, c["OH"], c["OW"], c["top"], c["left"], c["S"])
    box2 = (c["i2"], c["j2"], c["h2"], c["w2"]) if c["mode"] == TWO_CROPS else None
    return train_u8(src, (c["i1"], c["j1"], c["h1"], c["w1"]), box2, c["S"])


def golden_cases():
    """[(row of `cases`, PIL's bytes [c, S, S])] of the committed file."""
    with np.load(GOLDEN_FILE) as z:
        cases, out = z["cases"], z["out"]
    res, pos = [], 0
    for row in cases:
        c = dict(zip(COLS, (int(v) for v in row)))
        n = c["c"] * c["S"] * c["S"]
        res.append((row, out[pos:pos + n].reshape(c["c"], c["S"], c["S"])))
        pos += n
    assert pos == len(out)
    return res


def params_of(rows):
    """Plan rows int32 [n, 16] holding the boxes of golden rows (no flip, no erase)."""
    p = np.zeros((len(rows), R.PARAMS), np.int32)
    for b, row in enumerate(rows):
        c = dict(zip(COLS, (int(v) for v in row)))
        p[b, 0:4] = c["i1"], c["j1"], c["h1"], c["w1"]
        if c["mode"] == TWO_CROPS:
            p[b, 4:8] = c["i2"], c["j2"], c["h2"], c["w2"]
    return p
