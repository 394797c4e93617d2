// The input side of a training step on the device (data/data.py:254-315, tools/utils.py:86-113): gather the batch's rows
// from a resident uint8 data set, random-resized-crop with PIL's antialiased 8-bit bicubic (once or twice), flip, ToTensor,
// Normalize, RandomErasing(mode='pixel'); and the evaluation transform (Resize -> CenterCrop -> ToTensor -> Normalize)
// through the same stages.  vsom_augment_plan draws every sample's boxes from (seed, epoch, dataset index) alone.
#include "common.h"

namespace vsom {

constexpr int AUG_P = 16;          // int32 per sample in the plan (include/vitsom_hip.h lists the fields)
constexpr int AUG_THREADS = 512;
constexpr int AUG_MAXT = 17;       // taps of one output pixel: 2 ceil(2 scale) + 1 with scale <= 4
constexpr int AUG_KPAD = 20;       // ... padded with zero coefficients to whole groups of four
constexpr int AUG_KLD = 21;        // row stride of the coefficient table in LDS (odd: rows fall on different banks)
constexpr int AUG_MAXO = 73;       // largest output size of one pass: int(64 / 0.875)
constexpr int AUG_SRC_BYTES = 3 * 64 * 64 + 256;   // slack: a padded tap group may read up to 3 rows past the image
constexpr int AUG_BUF_BYTES = 16384;   // >= 3 * 64 * 73 (horizontal pass of the evaluation resize) and >= 3 * 73 * 73
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
__device__ void draw_box(const BoxDraw d, int Hs, int Ws, uint32_t blk, uint32_t idx, uint32_t epoch, uint32_t k0, uint32_t k1,
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

__global__ __launch_bounds__(256) void augment_plan_kernel(const int64_t* __restrict__ index, long N, int B, int H, int S, BoxDraw d1,
                                                           BoxDraw d2, int two, double flip_p, double erase_p, uint32_t k0,
                                                           uint32_t k1, uint32_t epoch, int* __restrict__ params) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    long row = index[b];
    row = row < 0 ? 0 : (row >= N ? N - 1 : row);          // clamped as augment_batch_kernel clamps it: one key for both
    const uint32_t idx = (uint32_t)row;
    int p[AUG_P];
#pragma unroll
    for (int i = 0; i < AUG_P; ++i) p[i] = 0;
    draw_box(d1, H, H, 0, idx, epoch, k0, k1, p);
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
    int4* dst = reinterpret_cast<int4*>(params + (long)b * AUG_P);
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

struct CoefTab {
    int kk[AUG_MAXO][AUG_KLD];
    short xmin[AUG_MAXO], n[AUG_MAXO];
};

// Row xx of PIL's precompute_coeffs + normalize_coeffs_8bpc for in -> out pixels: double arithmetic in PIL's operation
// order, nothing contracted into an FMA (x86-64 C does not contract), so the 22-bit integers are PIL's.
__device__ void coef_row(CoefTab& t, int in, int out, int xx) {
#pragma clang fp contract(off)
    const double scale = (double)in / (double)out;
    const double fscale = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * fscale, ss = 1.0 / fscale;
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    xmax -= xmin;
    if (xmax > AUG_MAXT) xmax = AUG_MAXT;                  // never taken for in <= 4 out (checked by the host)
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) ww += bicubic_filter((x + xmin - center + 0.5) * ss);
    for (int x = 0; x < xmax; ++x) {
        double w = bicubic_filter((x + xmin - center + 0.5) * ss);
        if (ww != 0.0) w /= ww;
        t.kk[xx][x] = w < 0 ? (int)(-0.5 + w * (double)(1 << AUG_PREC)) : (int)(0.5 + w * (double)(1 << AUG_PREC));
    }
    for (int x = xmax; x < AUG_KPAD; ++x) t.kk[xx][x] = 0;
    t.xmin[xx] = (short)xmin;
    t.n[xx] = (short)xmax;
}

__device__ __forceinline__ unsigned char clip8(int v) {
    v >>= AUG_PREC;
    return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// One crop-resize of the C planes in `src` (plane stride sps, row stride sld), box (i, j, h, w) -> out x out, horizontal
// pass first with the 8-bit intermediate PIL keeps (tmp: [C][h][out]), result dst: [C][out][out].  Ends synchronised.
// Lanes run along the output row (the next power of two lanes per row, so no index needs a division); taps go in groups
// of four, loads first: a group past the last tap multiplies whatever bytes lie there (inside the buffers' slack) by zero.
__device__ void crop_resize(const unsigned char* src, int sps, int sld, int i, int j, int h, int w, int C, int out,
                            unsigned char* tmp, unsigned char* dst, CoefTab& th, CoefTab& tv) {
    const int tid = threadIdx.x;
    if (tid < out) coef_row(th, w, out, tid);
    else if (tid >= AUG_THREADS / 2 && tid - AUG_THREADS / 2 < out) coef_row(tv, h, out, tid - AUG_THREADS / 2);
    __syncthreads();
    const int sh = out > 1 ? 32 - __clz(out - 1) : 0;      // lanes per row = 1 << sh >= out
    const int xx = tid & ((1 << sh) - 1), r0 = tid >> sh, rstep = AUG_THREADS >> sh;
    if (xx < out) {
        int k[AUG_KPAD];
#pragma unroll
        for (int q = 0; q < AUG_KPAD; ++q) k[q] = th.kk[xx][q];
        const int n = th.n[xx];
        const unsigned char* col0 = src + i * sld + j + th.xmin[xx];
        for (int c = 0; c < C; ++c) {
            for (int y = r0; y < h; y += rstep) {
                const unsigned char* row = col0 + c * sps + y * sld;
                int acc = 1 << (AUG_PREC - 1);
#pragma unroll
                for (int q = 0; q < AUG_KPAD; q += 4) {
                    if (q < n) {
                        const int b0 = row[q], b1 = row[q + 1], b2 = row[q + 2], b3 = row[q + 3];
                        acc += b0 * k[q] + b1 * k[q + 1] + b2 * k[q + 2] + b3 * k[q + 3];
                    }
                }
                tmp[(c * h + y) * out + xx] = clip8(acc);
            }
        }
    }
    __syncthreads();
    if (xx < out) {
        for (int c = 0; c < C; ++c) {
            for (int yy = r0; yy < out; yy += rstep) {
                const int n = tv.n[yy];
                const int* k = tv.kk[yy];
                const unsigned char* col = tmp + (c * h + tv.xmin[yy]) * out + xx;
                int acc = 1 << (AUG_PREC - 1);
                for (int q = 0; q < n; q += 4) {
                    const int b0 = col[q * out], b1 = col[(q + 1) * out], b2 = col[(q + 2) * out], b3 = col[(q + 3) * out];
                    acc += b0 * k[q] + b1 * k[q + 1] + b2 * k[q + 2] + b3 * k[q + 3];
                }
                dst[(c * out + yy) * out + xx] = clip8(acc);
            }
        }
    }
    __syncthreads();
}

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

// One workgroup (8 waves) per sample.  R = size of the first resize (S when training; int(S / 0.875) for the evaluation
// transform, whose centre window starts at `off`).
__global__ __launch_bounds__(AUG_THREADS) void augment_batch_kernel(const unsigned char* __restrict__ src, long N, int C, int H,
                                                            const int64_t* __restrict__ index, const int* __restrict__ params,
                                                            int S, int R, int off, const float* __restrict__ mean,
                                                            const float* __restrict__ stdv, uint32_t k0, uint32_t k1,
                                                            uint32_t epoch, float* __restrict__ out,
                                                            unsigned char* __restrict__ out_u8) {
    __shared__ __attribute__((aligned(16))) unsigned char bufA[AUG_SRC_BYTES];
    __shared__ __attribute__((aligned(16))) unsigned char bufB[AUG_BUF_BYTES];
    __shared__ __attribute__((aligned(16))) unsigned char bufC[AUG_BUF_BYTES];
    __shared__ CoefTab th, tv;
    const int tid = threadIdx.x, b = blockIdx.x;
    long idx = index[b];
    idx = idx < 0 ? 0 : (idx >= N ? N - 1 : idx);          // a bad index reads a wrong row, never outside the set

    // the plan, made safe: whatever the caller wrote, every box lies inside its image
    int p[13];
    if (params) {
#pragma unroll
        for (int i = 0; i < 13; ++i) p[i] = params[(long)b * AUG_P + i];
    } else {
        p[0] = 0; p[1] = 0; p[2] = H; p[3] = H;
#pragma unroll
        for (int i = 4; i < 13; ++i) p[i] = 0;
    }
    const int h1 = min(max(p[2], 1), H), w1 = min(max(p[3], 1), H);
    const int i1 = min(max(p[0], 0), H - h1), j1 = min(max(p[1], 0), H - w1);
    const bool two = R == S && p[6] > 0 && p[7] > 0;
    const int h2 = min(max(p[6], 1), S), w2 = min(max(p[7], 1), S);
    const int i2 = min(max(p[4], 0), S - h2), j2 = min(max(p[5], 0), S - w2);
    const bool flip = p[8] != 0;
    const int eh = min(max(p[11], 0), S), ew = min(max(p[12], 0), S);
    const int et = min(max(p[9], 0), S - eh), el = min(max(p[10], 0), S - ew);

    const int img = C * H * H;
    const unsigned char* g = src + idx * img;
    if ((img & 15) == 0 && ((uintptr_t)src & 15) == 0) {
        for (int e = tid; e < img / 16; e += AUG_THREADS) reinterpret_cast<uint4*>(bufA)[e] = reinterpret_cast<const uint4*>(g)[e];
    } else {
        for (int e = tid; e < img; e += AUG_THREADS) bufA[e] = g[e];
    }
    __syncthreads();

    crop_resize(bufA, H * H, H, i1, j1, h1, w1, C, R, bufB, bufC, th, tv);
    const unsigned char* fin = bufC;
    // torchvision's RandAugment (data.py:301) would act here, on the 8-bit image in bufC: after crop 1, before crop 2
    if (two) {
        crop_resize(bufC, S * S, S, i2, j2, h2, w2, C, S, bufA, bufB, th, tv);
        fin = bufB;
        // ... and timm's rand-m9 auto-augment (inside create_transform, data.py:288-298) here, on bufB: after crop 2
    }

    // flip, ToTensor, Normalize, erase; element (c, y, x) of the output reads level (y + off, x + off) of the R x R image
    float* o = out + (long)b * C * S * S;
    unsigned char* o8 = out_u8 ? out_u8 + (long)b * C * S * S : nullptr;
    const uint32_t uidx = (uint32_t)idx;
    auto level = [&](int c, int y, int x) { return fin[(c * R + y + off) * R + (flip ? S - 1 - x : x) + off]; };
    auto value = [&](int c, unsigned char lv) { return __fdiv_rn(__fdiv_rn((float)lv, 255.f) - mean[c], stdv[c]); };
    if ((S & 3) == 0) {
        const int q4 = S >> 2, sh = q4 > 1 ? 32 - __clz(q4 - 1) : 0;         // lanes per output row, as in crop_resize
        const int xg = tid & ((1 << sh) - 1), r0 = tid >> sh, rstep = AUG_THREADS >> sh, x = 4 * xg;
        if (xg < q4) {
            for (int c = 0; c < C; ++c) {
                for (int y = r0; y < S; y += rstep) {
                    const int e4 = (c * S + y) * q4 + xg;
                    unsigned char lv[4];
                    float v[4];
#pragma unroll
                    for (int t = 0; t < 4; ++t) { lv[t] = level(c, y, x + t); v[t] = value(c, lv[t]); }
                    if (y >= et && y < et + eh && x + 3 >= el && x < el + ew) {
                        float nz[4];
                        noise4((uint32_t)e4, uidx, epoch, k0, k1, nz);
#pragma unroll
                        for (int t = 0; t < 4; ++t) if (x + t >= el && x + t < el + ew) v[t] = nz[t];
                    }
                    f32x4 vv = {v[0], v[1], v[2], v[3]};
                    *reinterpret_cast<f32x4*>(o + e4 * 4) = vv;
                    if (o8) *reinterpret_cast<uchar4*>(o8 + e4 * 4) = make_uchar4(lv[0], lv[1], lv[2], lv[3]);
                }
            }
        }
    } else {
        for (int e = tid; e < C * S * S; e += AUG_THREADS) {
            const int x = e % S, y = (e / S) % S, c = e / (S * S);
            const unsigned char lv = level(c, y, x);
            float v = value(c, lv);
            if (y >= et && y < et + eh && x >= el && x < el + ew) {
                float nz[4];
                noise4((uint32_t)(e >> 2), uidx, epoch, k0, k1, nz);
                v = nz[e & 3];
            }
            o[e] = v;
            if (o8) o8[e] = lv;
        }
    }
}

}  // namespace vsom

extern "C" {

int vsom_augment_plan(const int64_t* index, long N, int B, int H, int S, double scale0, double scale1, double log_ratio0,
                      double log_ratio1, int two_stage, double scale2_0, double scale2_1, double log_ratio2_0,
                      double log_ratio2_1, double flip_p, double erase_p, uint64_t seed, int epoch, int32_t* params,
                      vsom_stream_t stream) {
    VSOM_REQUIRE(index && params, VSOM_EINVAL, "augment_plan: null pointer");
    VSOM_REQUIRE(N > 0 && B > 0 && H > 0 && S > 0 && epoch >= 0, VSOM_EINVAL,
                 "augment_plan: bad sizes (N=%ld B=%d H=%d S=%d epoch=%d)", N, B, H, S, epoch);
    VSOM_REQUIRE(H <= 64 && S <= 64 && N < (1L << 31), VSOM_EUNSUPPORTED, "augment_plan: H=%d, S=%d (at most 64), N=%ld (below 2^31)",
                 H, S, N);
    VSOM_REQUIRE(scale0 > 0 && scale0 <= scale1 && log_ratio0 <= log_ratio1, VSOM_EINVAL, "augment_plan: bad scale / ratio range");
    VSOM_REQUIRE(!two_stage || (scale2_0 > 0 && scale2_0 <= scale2_1 && log_ratio2_0 <= log_ratio2_1), VSOM_EINVAL,
                 "augment_plan: bad scale / ratio range of the second crop");
    VSOM_REQUIRE(flip_p >= 0 && flip_p <= 1 && erase_p >= 0 && erase_p <= 1, VSOM_EINVAL, "augment_plan: probability outside [0, 1]");
    VSOM_REQUIRE(vsom::aligned16(params), VSOM_EALIGN, "augment_plan: params must be 16-byte aligned");
    const vsom::BoxDraw d1 = {scale0, scale1, log_ratio0, log_ratio1}, d2 = {scale2_0, scale2_1, log_ratio2_0, log_ratio2_1};
    VSOM_LAUNCH(vsom::augment_plan_kernel, dim3(vsom::cdiv(B, 256)), dim3(256), 0, stream, index, N, B, H, S, d1, d2, two_stage,
                flip_p, erase_p, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)epoch, params);
    VSOM_LAUNCH_CHECK("augment_plan_kernel");
}

int vsom_augment_batch(const unsigned char* src, long N, int C, int H, int W, const int64_t* index, const int32_t* params, int B,
                       int S, int R, int off, const float* mean, const float* std, uint64_t seed, int epoch, float* out,
                       unsigned char* out_u8, vsom_stream_t stream) {
    VSOM_REQUIRE(src && index && mean && std && out, VSOM_EINVAL, "augment_batch: null pointer");
    VSOM_REQUIRE(N > 0 && B > 0 && H > 0 && W > 0 && S > 0 && epoch >= 0, VSOM_EINVAL,
                 "augment_batch: bad sizes (N=%ld B=%d H=%d W=%d S=%d epoch=%d)", N, B, H, W, S, epoch);
    VSOM_REQUIRE(C == 1 || C == 3, VSOM_EUNSUPPORTED, "augment_batch: %d channels (1 or 3)", C);
    VSOM_REQUIRE(H == W && H <= 64, VSOM_EUNSUPPORTED, "augment_batch: %d x %d source (square, at most 64 x 64)", H, W);
    VSOM_REQUIRE(S <= 64 && N < (1L << 31), VSOM_EUNSUPPORTED, "augment_batch: S=%d (at most 64), N=%ld (below 2^31)", S, N);
    VSOM_REQUIRE(R >= S && R <= vsom::AUG_MAXO && off >= 0 && off + S <= R, VSOM_EINVAL,
                 "augment_batch: first resize R=%d, window offset %d do not hold an S=%d window (S <= R <= 73)", R, off, S);
    VSOM_REQUIRE(H <= 4 * S, VSOM_EUNSUPPORTED, "augment_batch: %d -> %d shrinks by more than 4", H, S);
    VSOM_REQUIRE(vsom::aligned16(out) && (!params || vsom::aligned16(params)) && ((uintptr_t)out_u8 & 3) == 0, VSOM_EALIGN,
                 "augment_batch: out and params must be 16-byte aligned");
    VSOM_LAUNCH(vsom::augment_batch_kernel, dim3(B), dim3(vsom::AUG_THREADS), 0, stream, src, N, C, H, index, params, S, R, off, mean, std,
                (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)epoch, out, out_u8);
    VSOM_LAUNCH_CHECK("augment_batch_kernel");
}

}  // extern "C"
