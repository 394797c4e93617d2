"""numpy restatements the RandAugment / rand-m9 tests compare against (tests/test_randaug_cpu.py, tests/test_randaug_gpu.py):
the PIL primitives the two policies are built from (Image.transform(AFFINE) with NEAREST and BICUBIC, ImageEnhance's blend
and its four degenerate images, the ImageOps look-up tables), the per-sample record of vsom_randaug_plan, and the whole
two-stage transform of vsom_augment_batch_ra.  PIL itself pins the primitives (tests/golden/pil_randaug_ops.npz)."""
import math

import numpy as np

import data_ref as D

WORDS, SLOT0, SLOT_WORDS, SLOTS = 72, 8, 16, 4
(NONE, AFFINE_NEAREST, AFFINE_BICUBIC, BRIGHTNESS, COLOR, CONTRAST, SHARPNESS, POSTERIZE, SOLARIZE, SOLARIZE_ADD, INVERT,
 AUTOCONTRAST, EQUALIZE) = range(13)
N_OPS = 13
STREAM = 2                    # Philox stream of the record (0: crop / erase plan, 1: erase noise)

# torchvision RandAugment(num_ops, magnitude=9, num_magnitude_bins=31): name, signed
TV_OPS = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast", "Sharpness",
          "Posterize", "Solarize", "AutoContrast", "Equalize")
TV_BIN = 9 / 30                                             # magnitude bin 9 of linspace(0, max, 31)
TV_SHEAR, TV_ROTATE, TV_ENHANCE = 0.3 * TV_BIN, 30.0 * TV_BIN, 0.9 * TV_BIN
TV_POSTERIZE, TV_SOLARIZE = 8 - int(round(9 / (30 / 4))), 255.0 - 255.0 * TV_BIN
# timm rand-m9-mstd0.5-inc1: _RAND_INCREASING_TRANSFORMS, two layers, each applied with probability 1/2
TIMM_OPS = ("AutoContrast", "Equalize", "Invert", "Rotate", "PosterizeIncreasing", "SolarizeIncreasing", "SolarizeAdd",
            "ColorIncreasing", "ContrastIncreasing", "BrightnessIncreasing", "SharpnessIncreasing", "ShearX", "ShearY",
            "TranslateXRel", "TranslateYRel")
TIMM_M, TIMM_MSTD, TIMM_MMAX, TIMM_P = 9.0, 0.5, 10.0, 0.5


def tv_translate(S):
    return int(150.0 / 331.0 * S * 0.3)


def timm_fill(mean):
    return tuple(min(255, round(255 * m)) for m in mean)


# ---------------------------------------------------------------- the record
def empty_record(n=1):
    return np.zeros((n, WORDS), np.int32)


def put_slot(row, s, op, ip=0, f=1.0, fill=(0, 0, 0), a=(0.0,) * 6):
    """Write slot s of one record row (int32 [72]): {op, integer parameter, fp32 factor bits, fill R | G << 8 | B << 16,
    six doubles}."""
    w = SLOT0 + s * SLOT_WORDS
    fill = tuple(fill) + (0,) * (3 - len(fill))
    row[w:w + 4] = np.array([op, ip, np.array(f, np.float32).view(np.int32), fill[0] | fill[1] << 8 | fill[2] << 16], np.int32)
    row[w + 4:w + 16] = np.array(a, np.float64).view(np.int32)


def get_slot(row, s):
    w = SLOT0 + s * SLOT_WORDS
    v = np.ascontiguousarray(row[w:w + SLOT_WORDS]).astype(np.int32)
    fill = int(v[3])
    return dict(op=int(v[0]), ip=int(v[1]), f=float(v[2:3].view(np.float32)[0]), fill=(fill & 255, fill >> 8 & 255, fill >> 16 & 255),
                a=tuple(float(x) for x in v[4:16].view(np.float64)))


def coefficients(rec):
    """float64 [n, 4, 6]: the affine coefficients of every slot."""
    rec = np.ascontiguousarray(rec, np.int32)
    return np.stack([rec[:, SLOT0 + s * SLOT_WORDS + 4:SLOT0 + (s + 1) * SLOT_WORDS].copy().view(np.float64) for s in range(SLOTS)], 1)


def factors(rec):
    rec = np.ascontiguousarray(rec, np.int32)
    return np.stack([rec[:, SLOT0 + s * SLOT_WORDS + 2].copy().view(np.float32) for s in range(SLOTS)], 1)


def integer_words(rec):
    """The words of a record that hold integers: header, and per slot op / integer parameter / fill."""
    rec = np.asarray(rec)
    cols = list(range(SLOT0)) + [SLOT0 + s * SLOT_WORDS + k for s in range(SLOTS) for k in (0, 1, 3)]
    return rec[:, cols]


# ---------------------------------------------------------------- Image.transform(AFFINE)
def affine_nearest(ch, a, fill):
    """libImaging/Geometry.c affine_fixed on one channel: 16.16 fixed point."""
    S = ch.shape[0]

    def fix(v):
        return math.floor(v * 65536.0 + 0.5)
    a0, a1, a3, a4 = fix(a[0]), fix(a[1]), fix(a[3]), fix(a[4])
    a2, a5 = fix(a[2] + a[0] * 0.5 + a[1] * 0.5), fix(a[5] + a[3] * 0.5 + a[4] * 0.5)
    y, x = np.mgrid[0:S, 0:S].astype(np.int64)
    xi, yi = (a2 + a1 * y + a0 * x) >> 16, (a5 + a4 * y + a3 * x) >> 16
    ok = (xi >= 0) & (xi < S) & (yi >= 0) & (yi < S)
    out = np.full((S, S), fill, np.uint8)
    out[ok] = ch[yi[ok], xi[ok]]
    return out


def _sequential(start, step, n):
    """start, start + step, (start + step) + step, ...: n values, each one rounded addition after the last."""
    return np.cumsum(np.concatenate([[start], np.full(n - 1, step)]))


def _cubic(v1, v2, v3, v4, d):
    p1, p2, p3, p4 = v2, -v1 + v3, 2 * (v1 - v2) + v3 - v4, -v1 + v2 - v3 + v4
    return p1 + d * (p2 + d * (p3 + d * p4))


def affine_bicubic(ch, a, fill):
    """Geometry.c's generic affine loop with bicubic_filter8: doubles, coordinates accumulated pixel by pixel."""
    S = ch.shape[0]
    src = ch.astype(np.float64)
    r2 = _sequential(a[2] + a[0] * 0.5 + a[1] * 0.5, a[1], S)
    r5 = _sequential(a[5] + a[3] * 0.5 + a[4] * 0.5, a[4], S)
    xx = np.stack([_sequential(r2[y], a[0], S) for y in range(S)])
    yy = np.stack([_sequential(r5[y], a[3], S) for y in range(S)])
    ok = ~((xx < 0) | (xx >= S) | (yy < 0) | (yy >= S))
    xi, yi = xx - 0.5, yy - 0.5
    x0, y0 = np.floor(xi), np.floor(yi)
    dx, dy = xi - x0, yi - y0
    x0, y0 = x0.astype(np.int64) - 1, y0.astype(np.int64) - 1
    cols = [np.clip(x0 + k, 0, S - 1) for k in range(4)]
    rows = [_cubic(*[src[np.clip(y0 + r, 0, S - 1), c] for c in cols], dx) for r in range(4)]
    v = _cubic(rows[0], rows[1], rows[2], rows[3], dy)
    res = np.where(v <= 0, 0, np.where(v >= 255, 255, np.trunc(np.clip(v, 0, 255)))).astype(np.uint8)
    return np.where(ok, res, np.uint8(fill))


def rotate_matrix(angle, S):
    """Image.rotate's inverse map about the centre (S / 2, S / 2)."""
    angle = angle % 360.0
    t = -math.radians(angle)
    m = [round(math.cos(t), 15), round(math.sin(t), 15), 0.0, round(-math.sin(t), 15), round(math.cos(t), 15), 0.0]
    cx = cy = S / 2.0
    m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return tuple(m)


# ---------------------------------------------------------------- ImageEnhance
def blend(a, b, alpha):
    """Image.blend(a, b, alpha) on uint8 arrays: fp32, truncated; clipped outside [0, 1]."""
    al = np.float32(alpha)
    a, b = a.astype(np.float32), b.astype(np.float32)
    t = a + al * (b - a)
    if 0.0 <= float(al) <= 1.0:
        return t.astype(np.int32).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.clip(t, 0, 255).astype(np.int32))).astype(np.uint8)


def luminance(img):
    if img.shape[0] == 1:
        return img[0].astype(np.int64)
    r, g, b = (img[c].astype(np.int64) for c in range(3))
    return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16


def smooth(img):
    """ImageFilter.SMOOTH: 3 x 3, fp32 weights, accumulated from 0.5, truncated; the border is copied."""
    C, S, _ = img.shape
    out = img.copy()
    if S < 3:
        return out
    k = np.array([1, 1, 1, 1, 5, 1, 1, 1, 1], np.float32) / np.float32(13)
    acc = np.full((C, S - 2, S - 2), 0.5, np.float32)
    i = 0
    for dy in (1, 0, -1):
        row = np.zeros((C, S - 2, S - 2), np.float32)
        for dx in (-1, 0, 1):
            row = row + k[i] * img[:, 1 + dy:S - 1 + dy, 1 + dx:S - 1 + dx].astype(np.float32)
            i += 1
        acc = acc + row
    out[:, 1:-1, 1:-1] = np.clip(acc.astype(np.int32), 0, 255)
    return out


def enhance(img, op, f):
    if op == BRIGHTNESS:
        deg = np.zeros_like(img)
    elif op == COLOR:
        deg = np.broadcast_to(luminance(img).astype(np.uint8), img.shape)
    elif op == CONTRAST:
        L = luminance(img)
        deg = np.full_like(img, int(float(L.sum()) / L.size + 0.5))
    else:
        deg = smooth(img)
    return blend(deg, img, f)


# ---------------------------------------------------------------- ImageOps
def lut_of(ch, op, ip):
    i = np.arange(256)
    if op == POSTERIZE:
        return (i & ((0xFF << (8 - ip)) & 0xFF)).astype(np.uint8)
    if op == SOLARIZE:
        return np.where(i < ip, i, 255 - i).astype(np.uint8)
    if op == SOLARIZE_ADD:
        return np.where(i < 128, np.minimum(255, i + ip), i).astype(np.uint8)
    if op == INVERT:
        return (255 - i).astype(np.uint8)
    h = np.bincount(ch.ravel(), minlength=256)
    nz = np.flatnonzero(h)
    if op == AUTOCONTRAST:
        lo, hi = int(nz[0]), int(nz[-1])
        if hi <= lo:
            return i.astype(np.uint8)
        scale = 255.0 / (hi - lo)
        offset = -lo * scale
        return np.array([min(255, max(0, int(k * scale + offset))) for k in range(256)], np.uint8)
    step = (int(h.sum()) - int(h[nz[-1]])) // 255                       # EQUALIZE
    if len(nz) <= 1 or step == 0:
        return i.astype(np.uint8)
    n = step // 2 + np.concatenate([[0], np.cumsum(h)[:-1]])
    return np.minimum(255, n // step).astype(np.uint8)


def apply_slot(img, slot):
    """One primitive on a uint8 [C, S, S] image."""
    op = slot["op"]
    if op == NONE:
        return img
    if op in (AFFINE_NEAREST, AFFINE_BICUBIC):
        f = affine_nearest if op == AFFINE_NEAREST else affine_bicubic
        return np.stack([f(img[c], slot["a"], slot["fill"][c]) for c in range(img.shape[0])])
    if op in (BRIGHTNESS, COLOR, CONTRAST, SHARPNESS):
        return enhance(img, op, slot["f"])
    return np.stack([lut_of(img[c], op, slot["ip"])[img[c]] for c in range(img.shape[0])])


def transform_u8(src, p, row, S):
    """The 8-bit image vsom_augment_batch_ra normalises: crop 1 -> slots 0, 1 -> flip 1 -> crop 2 -> flip 2 -> slots 2, 3."""
    H = src.shape[1]
    i, j, h, w = (int(v) for v in p[:4])
    img = D.resize_u8(src[:, i:i + h, j:j + w], S)
    for s in (0, 1):
        img = apply_slot(img, get_slot(row, s))
    if row[0]:
        img = img[:, :, ::-1]
    if p[6] > 0 and p[7] > 0:
        i, j, h, w = (int(v) for v in p[4:8])
        img = D.resize_u8(np.ascontiguousarray(img[:, i:i + h, j:j + w]), S)
    if row[1]:
        img = img[:, :, ::-1]
    for s in (2, 3):
        img = apply_slot(np.ascontiguousarray(img), get_slot(row, s))
    return np.ascontiguousarray(img)


# ---------------------------------------------------------------- the plan (vsom_randaug_plan)
def uniforms(index, epoch, seed, nblocks=9):
    """u[n, block, 2]: the two 53-bit uniforms of each Philox block of the record's stream."""
    index = np.asarray(index, np.uint64)
    blk = np.arange(nblocks, dtype=np.uint64)[None, :]
    r = D.philox4x32_10(blk, index[:, None], STREAM, epoch, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return np.stack([D.u53(r[0], r[1]), D.u53(r[2], r[3])], -1)


def pick(u, n):
    return min(int(u * n), n - 1)


def tv_slot(k, neg, S):
    """Primitive of torchvision op k at magnitude bin 9: (op, ip, f, a)."""
    sg = -1.0 if neg else 1.0
    name = TV_OPS[k]
    if name in ("ShearX", "ShearY"):
        v = sg * math.tan(math.radians(math.degrees(math.atan(TV_SHEAR))))
        return AFFINE_NEAREST, 0, 1.0, (1.0, v, 0.0, 0.0, 1.0, 0.0) if name == "ShearX" else (1.0, 0.0, 0.0, v, 1.0, 0.0)
    if name in ("TranslateX", "TranslateY"):
        v = sg * tv_translate(S)
        return AFFINE_NEAREST, 0, 1.0, (1.0, 0.0, -v, 0.0, 1.0, 0.0) if name == "TranslateX" else (1.0, 0.0, 0.0, 0.0, 1.0, -v)
    if name == "Rotate":
        return AFFINE_NEAREST, 0, 1.0, rotate_matrix(sg * TV_ROTATE, S)
    if name in ("Brightness", "Color", "Contrast", "Sharpness"):
        return {"Brightness": BRIGHTNESS, "Color": COLOR, "Contrast": CONTRAST, "Sharpness": SHARPNESS}[name], 0, 1.0 + sg * TV_ENHANCE, (0.0,) * 6
    if name == "Posterize":
        return POSTERIZE, TV_POSTERIZE, 1.0, (0.0,) * 6
    if name == "Solarize":
        return SOLARIZE, math.ceil(TV_SOLARIZE), 1.0, (0.0,) * 6        # i < 178.5 <=> i < 179
    return {"Identity": NONE, "AutoContrast": AUTOCONTRAST, "Equalize": EQUALIZE}[name], 0, 1.0, (0.0,) * 6


def timm_slot(k, neg, m, S):
    """Primitive of timm op k at magnitude m (0 .. 10)."""
    sg = -1.0 if neg else 1.0
    name, lv = TIMM_OPS[k], m / 10.0
    if name in ("ShearX", "ShearY"):
        v = sg * (lv * 0.3)
        return AFFINE_BICUBIC, 0, 1.0, (1.0, v, 0.0, 0.0, 1.0, 0.0) if name == "ShearX" else (1.0, 0.0, 0.0, v, 1.0, 0.0)
    if name in ("TranslateXRel", "TranslateYRel"):
        v = sg * (lv * 0.45) * S
        return AFFINE_BICUBIC, 0, 1.0, (1.0, 0.0, v, 0.0, 1.0, 0.0) if name == "TranslateXRel" else (1.0, 0.0, 0.0, 0.0, 1.0, v)
    if name == "Rotate":
        return AFFINE_BICUBIC, 0, 1.0, rotate_matrix(sg * (lv * 30.0), S)
    if name.endswith("Increasing") and name[:-10] in ("Color", "Contrast", "Brightness", "Sharpness"):
        op = {"Color": COLOR, "Contrast": CONTRAST, "Brightness": BRIGHTNESS, "Sharpness": SHARPNESS}[name[:-10]]
        return op, 0, max(0.1, 1.0 + sg * (lv * 0.9)), (0.0,) * 6
    if name == "PosterizeIncreasing":
        return POSTERIZE, 4 - int(lv * 4), 1.0, (0.0,) * 6
    if name == "SolarizeIncreasing":
        return SOLARIZE, 256 - int(lv * 256), 1.0, (0.0,) * 6
    if name == "SolarizeAdd":
        return SOLARIZE_ADD, min(128, int(lv * 110)), 1.0, (0.0,) * 6
    return {"AutoContrast": AUTOCONTRAST, "Equalize": EQUALIZE, "Invert": INVERT}[name], 0, 1.0, (0.0,) * 6


def plan(index, epoch, seed, S, randaug_n, autoaugment, flip1_p, fill):
    """int32 [n, 72] as vsom_randaug_plan writes them.  Header: flip 1, flip 2, the policy's pick for slots 0 .. 3 (-1: the
    stage is empty), the bits of the timm slots that are applied, 0.  Blocks: 0 flips; 1, 2 the torchvision slots (pick,
    sign); 3 + 3 t, 4 + 3 t, 5 + 3 t timm slot t (pick and apply; the two uniforms of the normal draw; sign)."""
    u = uniforms(index, epoch, seed)
    out = empty_record(len(index))
    for n in range(len(index)):
        row = out[n]
        row[0], row[1] = u[n, 0, 0] < flip1_p, u[n, 0, 1] < 0.5
        row[2:6] = -1
        for s in range(randaug_n):
            k = pick(u[n, 1 + s, 0], len(TV_OPS))
            op, ip, f, a = tv_slot(k, u[n, 1 + s, 1] < 0.5, S)
            row[2 + s] = k
            if op != NONE:                              # Identity leaves the slot empty (all zero)
                put_slot(row, s, op, ip, f, (0, 0, 0), a)
        for t in range(2 if autoaugment else 0):
            b = 3 + 3 * t
            k = pick(u[n, b, 0], len(TIMM_OPS))
            row[4 + t] = k
            if not u[n, b, 1] < TIMM_P:
                continue
            row[6] |= 1 << t
            z = math.sqrt(-2.0 * math.log(1.0 - u[n, b + 1, 0])) * math.cos(6.283185307179586 * u[n, b + 1, 1])
            m = min(TIMM_MMAX, max(0.0, TIMM_M + TIMM_MSTD * z))
            op, ip, f, a = timm_slot(k, u[n, b + 2, 0] < 0.5, m, S)
            put_slot(row, 2 + t, op, ip, f, fill if op == AFFINE_BICUBIC else (0, 0, 0), a)
    return out
