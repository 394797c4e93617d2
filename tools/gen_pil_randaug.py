"""Write tests/golden/pil_randaug_ops.npz: what PIL makes of a few uint8 images under every primitive that torchvision's
RandAugment and timm's rand-m9 auto-augment are built from -- Image.transform(AFFINE) with NEAREST and BICUBIC, Image.rotate,
the four ImageEnhance classes, ImageOps.posterize / solarize / invert / autocontrast / equalize and timm's solarize-add
look-up table -- with both signs, factors on both sides of 1 and the edge cases (a constant channel, equalize's step == 0,
posterize to 8 and 0 bits, a translate that pushes the whole image out).  Needs PIL (made with 12.2.0).  Every parameter is
rounded to an fp32-representable value before PIL sees it.

Per group g (one image shape):
    g<k>_src [n_src, C, S, S] uint8, g<k>_index [n] int64 (the source of each case), g<k>_slot [n, 16] int32 (one op slot of
    the record of vsom_augment_batch_ra: op, integer parameter, fp32 factor bits, fill R | G << 8 | B << 16, six doubles),
    g<k>_out [n, C, S, S] uint8 (PIL's bytes).  The rotate cases hold the matrix of Image.rotate's recipe and the bytes of
    Image.rotate itself.

    python tools/gen_pil_randaug.py
"""
import math
import os
import sys

import numpy as np
from PIL import Image, ImageEnhance, ImageOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import randaug_ref as RA  # noqa: E402  (codes, record layout and the rotate recipe; no primitive of it is used here)

NOISE, SMOOTH, NARROW, TWO_LEVEL = range(4)


def f32(v):
    return float(np.float32(v))


def sources(rng, C, S):
    noise = rng.integers(0, 256, (C, S, S), dtype=np.uint8)
    yy, xx = np.mgrid[0:S, 0:S]
    smooth = np.stack([(127.5 + 127.5 * np.sin(xx * rng.uniform(0.1, 0.8) + rng.uniform(0, 6)) * np.cos(yy * rng.uniform(0.1, 0.8)))
                       .astype(np.uint8) for _ in range(C)])
    narrow = rng.integers(60, 180, (C, S, S), dtype=np.uint8)
    narrow[C // 2] = 93                                       # a constant channel: autocontrast and equalize leave it alone
    two = np.full((C, S, S), 200, np.uint8)                   # all but a few pixels in the last bin: equalize's step == 0
    two[:, 1, 2:9] = 10
    return np.stack([noise, smooth, narrow, two])


def to_pil(img):
    return Image.fromarray(img[0]) if img.shape[0] == 1 else Image.fromarray(np.ascontiguousarray(img.transpose(1, 2, 0)))


def from_pil(im, C):
    a = np.asarray(im)
    return a[None] if C == 1 else np.ascontiguousarray(a.transpose(2, 0, 1))


def solarize_add(im, add, thresh=128):
    lut = [min(255, i + add) if i < thresh else i for i in range(256)]
    return im.point(lut * len(im.getbands()))


def cases(C, S, subset):
    """(source, op, integer parameter, factor, coefficients or rotate angle, fill, PIL call) of one group."""
    mean_fill = (125, 123, 114)[:C] if C == 3 else (128,)
    out = []
    pilfill = lambda fill: fill[0] if C == 1 else tuple(fill)                                   # noqa: E731

    def affine(src, resample, a, fill):
        a = tuple(f32(v) for v in a)
        op = RA.AFFINE_NEAREST if resample == Image.NEAREST else RA.AFFINE_BICUBIC
        out.append((src, op, 0, 1.0, a, fill, lambda im: im.transform((S, S), Image.AFFINE, a, resample=resample, fillcolor=pilfill(fill))))

    def rotate(src, resample, angle, fill):
        angle = f32(angle)
        op = RA.AFFINE_NEAREST if resample == Image.NEAREST else RA.AFFINE_BICUBIC
        out.append((src, op, 0, 1.0, RA.rotate_matrix(angle, S), fill, lambda im: im.rotate(angle, resample=resample, fillcolor=pilfill(fill))))

    def enhance(src, op, f):
        f = f32(f)
        cls = {RA.BRIGHTNESS: ImageEnhance.Brightness, RA.COLOR: ImageEnhance.Color, RA.CONTRAST: ImageEnhance.Contrast,
               RA.SHARPNESS: ImageEnhance.Sharpness}[op]
        out.append((src, op, 0, f, (0.0,) * 6, (0, 0, 0), lambda im: cls(im).enhance(f)))

    def lut(src, op, ip=0):
        call = {RA.POSTERIZE: lambda im: ImageOps.posterize(im, ip), RA.SOLARIZE: lambda im: ImageOps.solarize(im, ip),
                RA.SOLARIZE_ADD: lambda im: solarize_add(im, ip), RA.INVERT: ImageOps.invert,
                RA.AUTOCONTRAST: ImageOps.autocontrast, RA.EQUALIZE: ImageOps.equalize}[op]
        out.append((src, op, ip, 1.0, (0.0,) * 6, (0, 0, 0), call))

    t = RA.tv_translate(S)
    if subset:                                                # 64 x 64: the ops whose loops depend on the size, both images
        for src in (NOISE, SMOOTH):
            affine(src, Image.NEAREST, (1, -0.09, 0, 0, 1, 0), (0, 0, 0))
            rotate(src, Image.NEAREST, 9.0, (0, 0, 0))
            affine(src, Image.BICUBIC, (1, 0, 0, 0.27, 1, 0), mean_fill)
            affine(src, Image.BICUBIC, (1, 0, -0.405 * S, 0, 1, 0), mean_fill)
            rotate(src, Image.BICUBIC, -27.3, mean_fill)
            for op, f in ((RA.BRIGHTNESS, 1.27), (RA.COLOR, 0.19), (RA.CONTRAST, 1.81), (RA.SHARPNESS, 1.9)):
                enhance(src, op, f)
            lut(src, RA.AUTOCONTRAST)
            lut(src, RA.EQUALIZE)
        lut(NARROW, RA.EQUALIZE)
        lut(TWO_LEVEL, RA.EQUALIZE)
        return out
    for k, sg in enumerate((1, -1)):
        src = k                                               # + on noise, - on the smooth image
        affine(src, Image.NEAREST, (1, sg * 0.09, 0, 0, 1, 0), (0, 0, 0))
        affine(src, Image.NEAREST, (1, 0, 0, sg * 0.09, 1, 0), (0, 0, 0))
        affine(src, Image.NEAREST, (1, 0, -sg * t, 0, 1, 0), (0, 0, 0))
        affine(src, Image.NEAREST, (1, 0, 0, 0, 1, -sg * t), (0, 0, 0))
        rotate(src, Image.NEAREST, sg * 9.0, (0, 0, 0))
        affine(src, Image.BICUBIC, (1, sg * 0.27, 0, 0, 1, 0), mean_fill)
        affine(src, Image.BICUBIC, (1, 0, 0, sg * 0.2613, 1, 0), mean_fill)
        affine(src, Image.BICUBIC, (1, 0, sg * 0.405 * S, 0, 1, 0), mean_fill)
        affine(src, Image.BICUBIC, (1, 0, 0, 0, 1, sg * 0.3871 * S), mean_fill)
        rotate(src, Image.BICUBIC, sg * 27.0, mean_fill)
        rotate(1 - src, Image.BICUBIC, sg * 13.37, mean_fill)
        for op in (RA.BRIGHTNESS, RA.COLOR, RA.CONTRAST, RA.SHARPNESS):
            enhance(src, op, 1.0 + sg * 0.27)                 # torchvision's bin 9
            enhance(1 - src, op, max(0.1, 1.0 + sg * 0.9))    # timm at m = 10: 1.9 and the floor 0.1
    affine(NOISE, Image.NEAREST, (1, 0, 0.37 - t, 0, 1, 0.81), (7, 200, 31)[:C])               # fractional, a fill of its own
    affine(NOISE, Image.NEAREST, (1, 0, S + 1, 0, 1, 0), (0, 0, 0))                             # the whole image pushed out
    affine(SMOOTH, Image.BICUBIC, (1, 0, 0, 0, 1, -(S + 0.5)), mean_fill)
    affine(NOISE, Image.BICUBIC, (1, 0, 0, 0, 1, 0), mean_fill)                                 # the identity map
    enhance(NARROW, RA.CONTRAST, 1.27)
    enhance(TWO_LEVEL, RA.SHARPNESS, 0.1)
    enhance(NOISE, RA.COLOR, 1.0)
    for bits in (8, 7, 4, 1, 0):
        lut(NOISE, RA.POSTERIZE, bits)
    for thr in (179, 0, 256, 26):
        lut(SMOOTH, RA.SOLARIZE, thr)
    for add in (0, 55, 128):
        lut(NOISE, RA.SOLARIZE_ADD, add)
    lut(NOISE, RA.INVERT)
    for src in (NOISE, SMOOTH, NARROW, TWO_LEVEL):
        lut(src, RA.AUTOCONTRAST)
        lut(src, RA.EQUALIZE)
    return out


def group(rng, C, S, subset=False):
    src = sources(rng, C, S)
    index, slots, outs = [], [], []
    for s, op, ip, f, a, fill, call in cases(C, S, subset):
        row = RA.empty_record()[0]
        RA.put_slot(row, 0, op, ip, f, fill, a)
        index.append(s)
        slots.append(row[RA.SLOT0:RA.SLOT0 + RA.SLOT_WORDS].copy())
        outs.append(from_pil(call(to_pil(src[s])), C))
    return src, np.array(index, np.int64), np.stack(slots), np.stack(outs)


def main():
    rng = np.random.default_rng(20240612)
    groups = [group(rng, 3, 32), group(rng, 1, 16), group(rng, 3, 64, subset=True)]
    arrays = {}
    for k, g in enumerate(groups):
        for name, a in zip(("src", "index", "slot", "out"), g):
            arrays[f"g{k}_{name}"] = a
    path = os.path.join(ROOT, "tests", "golden", "pil_randaug_ops.npz")
    np.savez_compressed(path, **arrays)
    print(f"{path}: {sum(len(g[1]) for g in groups)} cases in {len(groups)} groups, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
