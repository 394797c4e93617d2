"""numpy restatements the data-pipeline tests compare against (tests/test_data_cpu.py, tests/test_data_gpu.py):
PIL's 8-bit antialiased bicubic resampler, Philox4x32-10, and the augmentation plan of vsom_augment_plan."""
import math

import numpy as np

PREC = 22                     # PIL's PRECISION_BITS
PARAMS = 16
TIMM_SCALE, TIMM_RATIO = (0.08, 1.0), (3.0 / 4.0, 4.0 / 3.0)
LOG03 = (-1.2039728043259361, 1.2039728043259361)


# ---------------------------------------------------------------- PIL's resampler (libImaging/Resample.c, 8 bits per channel)
def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coeffs(in_size, out_size):
    """[(xmin, int32 taps)] per output pixel: precompute_coeffs + normalize_coeffs_8bpc for the box (0, in_size)."""
    scale = in_size / out_size
    fscale = max(scale, 1.0)
    support, ss = 2.0 * fscale, 1.0 / fscale
    rows = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in k:
            ww += v
        if ww != 0.0:
            k = [v / ww for v in k]
        rows.append((xmin, np.array([int(-0.5 + v * (1 << PREC)) if v < 0 else int(0.5 + v * (1 << PREC)) for v in k], np.int64)))
    return rows


def resize_u8(img, out):
    """uint8 [C, h, w] -> [C, out, out]: horizontal pass, 8-bit intermediate, vertical pass."""
    C, h, w = img.shape
    src = img.astype(np.int64)
    tmp = np.empty((C, h, out), np.int64)
    for xx, (x0, k) in enumerate(coeffs(w, out)):
        tmp[:, :, xx] = np.clip(((1 << (PREC - 1)) + (src[:, :, x0:x0 + len(k)] * k).sum(-1)) >> PREC, 0, 255)
    res = np.empty((C, out, out), np.int64)
    for yy, (y0, k) in enumerate(coeffs(h, out)):
        res[:, yy, :] = np.clip(((1 << (PREC - 1)) + (tmp[:, y0:y0 + len(k), :] * k[None, :, None]).sum(1)) >> PREC, 0, 255)
    return res.astype(np.uint8)


def transform_u8(src, p, S, R, off):
    """The 8-bit image vsom_augment_batch normalises: src uint8 [C, H, H], p = one plan row or None (whole image)."""
    H = src.shape[1]
    i, j, h, w = (0, 0, H, H) if p is None else (int(v) for v in p[:4])
    img = resize_u8(src[:, i:i + h, j:j + w], R)
    if p is not None and R == S and p[6] > 0 and p[7] > 0:
        i, j, h, w = (int(v) for v in p[4:8])
        img = resize_u8(img[:, i:i + h, j:j + w], S)
    img = img[:, off:off + S, off:off + S]
    if p is not None and p[8]:
        img = img[:, :, ::-1]
    return np.ascontiguousarray(img)


# ---------------------------------------------------------------- Philox4x32-10
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Arrays (or scalars) of uint32 counters / keys -> four uint32 arrays."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, np.uint64) & np.uint64(0xFFFFFFFF) for v in np.broadcast_arrays(c0, c1, c2, c3, k0, k1))
    M0, M1, W0, W1, LO = (np.uint64(v) for v in (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF))
    S32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & LO, (p0 >> S32) ^ c3 ^ k1, p0 & LO
        k0, k1 = (k0 + W0) & LO, (k1 + W1) & LO
    return c0, c1, c2, c3


def u53(hi, lo):
    return (((np.asarray(hi, np.uint64) >> np.uint64(5)) << np.uint64(26)) | (np.asarray(lo, np.uint64) >> np.uint64(6))).astype(np.float64) \
        * (1.0 / 9007199254740992.0)


def plan_uniforms(index, epoch, seed, nblocks=25):
    """u[n, block, 2]: the two 53-bit uniforms of each Philox block (counter (block, index, 0, epoch), key seed)."""
    index = np.asarray(index, np.uint64)
    blk = np.arange(nblocks, dtype=np.uint64)[None, :]
    r = philox4x32_10(blk, index[:, None], 0, epoch, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return np.stack([u53(r[0], r[1]), u53(r[2], r[3])], -1)


# ---------------------------------------------------------------- the plan
def _margin(v):
    """Distance of the unrounded v from the nearest rounding boundary (k + 1/2)."""
    return abs(v - math.floor(v) - 0.5)


def box_from_uniforms(ua, ur, ui, uj, H, W, scale, log_ratio):
    """tools/utils.py:93-113 fed four uniforms -> (i, j, h, w), smallest rounding margin."""
    area = (H * W) * (scale[0] + ua * (scale[1] - scale[0]))
    ar = math.exp(log_ratio[0] + ur * (log_ratio[1] - log_ratio[0]))
    fw, fh = math.sqrt(area * ar), math.sqrt(area / ar)
    w, h = max(min(int(round(fw)), W), 1), max(min(int(round(fh)), H), 1)
    i, j = min(int(ui * (H - h + 1)), H - h), min(int(uj * (W - w + 1)), W - w)
    return (i, j, h, w), min(_margin(fw), _margin(fh))


def plan(index, epoch, seed, H, S, scale, ratio, two_stage, flip_p, erase_p):
    """params int32 [n, 16] as vsom_augment_plan writes them, and per sample the smallest rounding margin met."""
    u = plan_uniforms(index, epoch, seed)
    n = len(index)
    out, margin = np.zeros((n, PARAMS), np.int32), np.full(n, 0.5)
    lr = (math.log(ratio[0]), math.log(ratio[1]))
    lr2 = (math.log(TIMM_RATIO[0]), math.log(TIMM_RATIO[1]))
    for s in range(n):
        box, m = box_from_uniforms(u[s, 0, 0], u[s, 0, 1], u[s, 1, 0], u[s, 1, 1], H, H, scale, lr)
        out[s, 0:4], margin[s] = box, m
        if two_stage:
            box, m = box_from_uniforms(u[s, 2, 0], u[s, 2, 1], u[s, 3, 0], u[s, 3, 1], S, S, TIMM_SCALE, lr2)
            out[s, 4:8], margin[s] = box, min(margin[s], m)
        out[s, 8] = u[s, 4, 0] < flip_p
        if u[s, 4, 1] < erase_p:
            for a in range(10):
                area = (S * S) * (0.02 + u[s, 5 + 2 * a, 0] * (1.0 / 3.0 - 0.02))
                ar = math.exp(LOG03[0] + u[s, 5 + 2 * a, 1] * (LOG03[1] - LOG03[0]))
                fh, fw = math.sqrt(area * ar), math.sqrt(area / ar)
                h, w = int(round(fh)), int(round(fw))
                margin[s] = min(margin[s], _margin(fh), _margin(fw))
                if h < S and w < S:
                    out[s, 9] = min(int(u[s, 6 + 2 * a, 0] * (S - h + 1)), S - h)
                    out[s, 10] = min(int(u[s, 6 + 2 * a, 1] * (S - w + 1)), S - w)
                    out[s, 11], out[s, 12] = h, w
                    break
    return out, margin


CIFAR_PLAN = dict(H=32, S=32, scale=(0.08, 1.0), ratio=(0.75, 1.3333), two_stage=True, flip_p=0.5, erase_p=0.25)
TINY_PLAN = dict(H=64, S=64, scale=(0.08, 1.0), ratio=(0.75, 1.3333), two_stage=True, flip_p=0.5, erase_p=0.25)
ONE_STAGE_PLAN = dict(H=28, S=28, scale=(0.3, 1.0), ratio=(0.5, 2.0), two_stage=False, flip_p=0.2, erase_p=0.9)


def gpu_plan_cases():
    """(seed, epoch, index, plan arguments) of the device-against-restatement plan test: 3 x 2 048 samples, each with 4 to 24
    square roots whose rounding is inspected."""
    yield 0, 0, np.arange(2048), CIFAR_PLAN
    yield 20240611, 3, np.arange(50000 - 2048, 50000), TINY_PLAN
    yield (7 << 32) | 5, 41, np.arange(0, 2048 * 13, 13), ONE_STAGE_PLAN
