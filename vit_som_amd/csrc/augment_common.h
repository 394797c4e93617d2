// Device functions shared by the two halves of the data pipeline: augment.hip (fixed-size sets, a sample resident in LDS)
// and augment_ragged.hip (variable-size sets, a sample walked in bands).  The plan's draws, PIL's coefficient rows and the
// erase noise are one piece of code, so the two pipelines agree bit for bit wherever their domains overlap.
#pragma once
#include "common.h"

namespace vsom {

constexpr int AUG_P = 16;          // int32 per sample in the plan (include/vitsom_hip.h lists the fields)
constexpr int AUG_PREC = 22;       // PIL's PRECISION_BITS for 8-bit images

// Philox4x32-10 (Salmon et al., SC'11).  Counter = (block, dataset index, stream, epoch), key = seed.
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t r[4]) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}
constexpr uint32_t AUG_STREAM_PLAN = 0, AUG_STREAM_NOISE = 1;

// ---------------------------------------------------------------- the plan
// 53-bit uniform in [0, 1) from two words
__device__ __forceinline__ double u53(uint32_t hi, uint32_t lo) {
    return (double)(((uint64_t)(hi >> 5) << 26) | (uint64_t)(lo >> 6)) * (1.0 / 9007199254740992.0);
}
__device__ __forceinline__ int randint_below(double u, int n) {       // floor(u n), n >= 1
    const int v = (int)(u * (double)n);
    return v < n ? v : n - 1;
}

struct BoxDraw { double s0, s1, l0, l1; };     // area share U(s0, s1), aspect exp(U(l0, l1)) (logs taken by the host)

// tools/utils.py:93-113 on an Hs x Ws image; two Philox blocks starting at `blk`
__device__ inline void draw_box(const BoxDraw d, int Hs, int Ws, uint32_t blk, uint32_t idx, uint32_t epoch, uint32_t k0, uint32_t k1,
                                int* out) {
#pragma clang fp contract(off)
    uint32_t r[4];
    philox4x32_10(blk, idx, AUG_STREAM_PLAN, epoch, k0, k1, r);
    const double area = (double)(Hs * Ws) * (d.s0 + u53(r[0], r[1]) * (d.s1 - d.s0));
    const double ar = exp(d.l0 + u53(r[2], r[3]) * (d.l1 - d.l0));
    int w = (int)rint(sqrt(area * ar)), h = (int)rint(sqrt(area / ar));      // Python's round: half to even
    w = max(min(w, Ws), 1);
    h = max(min(h, Hs), 1);
    philox4x32_10(blk + 1, idx, AUG_STREAM_PLAN, epoch, k0, k1, r);
    out[0] = randint_below(u53(r[0], r[1]), Hs - h + 1);
    out[1] = randint_below(u53(r[2], r[3]), Ws - w + 1);
    out[2] = h;
    out[3] = w;
}

// One row of the plan for data set row `idx`, whose image is Hs x Ws, and its 16-byte stores.
__device__ inline void plan_row(int Hs, int Ws, int S, BoxDraw d1, BoxDraw d2, int two, double flip_p, double erase_p, uint32_t idx,
                                uint32_t epoch, uint32_t k0, uint32_t k1, int* __restrict__ dst_row) {
#pragma clang fp contract(off)
    int p[AUG_P];
#pragma unroll
    for (int i = 0; i < AUG_P; ++i) p[i] = 0;
    draw_box(d1, Hs, Ws, 0, idx, epoch, k0, k1, p);
    if (two) draw_box(d2, S, S, 2, idx, epoch, k0, k1, p + 4);
    uint32_t r[4];
    philox4x32_10(4, idx, AUG_STREAM_PLAN, epoch, k0, k1, r);
    p[8] = u53(r[0], r[1]) < flip_p ? 1 : 0;
    if (u53(r[2], r[3]) < erase_p) {
        // timm RandomErasing: ten attempts of area U(0.02, 1/3) S^2, aspect exp(U(log 0.3, log 1/0.3))
        const double l0 = -1.2039728043259361, l1 = 1.2039728043259361;        // log(0.3), log(1 / 0.3)
        for (int a = 0; a < 10; ++a) {
            philox4x32_10(5 + 2 * a, idx, AUG_STREAM_PLAN, epoch, k0, k1, r);
            const double area = (double)(S * S) * (0.02 + u53(r[0], r[1]) * (1.0 / 3.0 - 0.02));
            const double ar = exp(l0 + u53(r[2], r[3]) * (l1 - l0));
            const int h = (int)rint(sqrt(area * ar)), w = (int)rint(sqrt(area / ar));
            if (h < S && w < S) {
                philox4x32_10(6 + 2 * a, idx, AUG_STREAM_PLAN, epoch, k0, k1, r);
                p[9] = randint_below(u53(r[0], r[1]), S - h + 1);
                p[10] = randint_below(u53(r[2], r[3]), S - w + 1);
                p[11] = h;
                p[12] = w;
                break;
            }
        }
    }
    int4* dst = reinterpret_cast<int4*>(dst_row);
#pragma unroll
    for (int i = 0; i < AUG_P / 4; ++i) dst[i] = make_int4(p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3]);
}

// ---------------------------------------------------------------- the resampler
__device__ __forceinline__ double bicubic_filter(double x) {
#pragma clang fp contract(off)
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// Geometry of row xx of PIL's precompute_coeffs for in -> out pixels: first tap and tap count (at most maxt).
struct TapRange { int xmin, n; double center, ss; };
__device__ __forceinline__ TapRange tap_range(int in, int out, int xx, int maxt) {
#pragma clang fp contract(off)
    const double scale = (double)in / (double)out;
    const double fscale = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * fscale;
    TapRange t;
    t.ss = 1.0 / fscale;
    t.center = (xx + 0.5) * scale;
    int xmin = (int)(t.center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(t.center + support + 0.5);
    if (xmax > in) xmax = in;
    xmax -= xmin;
    if (xmax > maxt) xmax = maxt;                          // never taken inside the entries' shrink limits
    t.xmin = xmin;
    t.n = xmax;
    return t;
}
// Sum of the row's filter values in PIL's order, and tap x of normalize_coeffs_8bpc: double arithmetic in PIL's operation
// order, nothing contracted into an FMA (x86-64 C does not contract), so the 22-bit integers are PIL's.
__device__ __forceinline__ double tap_sum(const TapRange& t) {
#pragma clang fp contract(off)
    double ww = 0.0;
    for (int x = 0; x < t.n; ++x) ww += bicubic_filter((x + t.xmin - t.center + 0.5) * t.ss);
    return ww;
}
__device__ __forceinline__ int tap_coef(const TapRange& t, double ww, int x) {
#pragma clang fp contract(off)
    double w = bicubic_filter((x + t.xmin - t.center + 0.5) * t.ss);
    if (ww != 0.0) w /= ww;
    return w < 0 ? (int)(-0.5 + w * (double)(1 << AUG_PREC)) : (int)(0.5 + w * (double)(1 << AUG_PREC));
}

__device__ __forceinline__ unsigned char clip8(int v) {
    v >>= AUG_PREC;
    return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// ---------------------------------------------------------------- the output stage
// Four standard normal draws for the element group g (elements 4g .. 4g + 3 of the sample's [C, S, S] output): Box-Muller
// in fp32 on one Philox block.
__device__ __forceinline__ void noise4(uint32_t g, uint32_t idx, uint32_t epoch, uint32_t k0, uint32_t k1, float n[4]) {
    uint32_t r[4];
    philox4x32_10(g, idx, AUG_STREAM_NOISE, epoch, k0, k1, r);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        // odd multiples of 2^-24, exact in fp32 and strictly inside (0, 1): the radius is never 0 and the angle never a
        // multiple of pi / 2, so no draw is exactly 0
        const float u1 = (float)(2u * (r[2 * h] >> 9) + 1u) * 0x1p-24f;
        const float u2 = (float)(2u * (r[2 * h + 1] >> 9) + 1u) * 0x1p-24f;
        const float rad = sqrtf(-2.f * logf(u1));
        float s, c;
        sincosf(6.283185307179586f * u2, &s, &c);
        n[2 * h] = rad * c;
        n[2 * h + 1] = rad * s;
    }
}

// ToTensor + Normalize of one 8-bit level: two true fp32 divides
__device__ __forceinline__ float normalized(unsigned char lv, float mean, float stdv) {
    return __fdiv_rn(__fdiv_rn((float)lv, 255.f) - mean, stdv);
}

}  // namespace vsom
