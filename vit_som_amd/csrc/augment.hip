// The input side of a training step on the device (data/data.py:254-315, tools/utils.py:86-113): gather the batch's rows
// from a resident uint8 data set, random-resized-crop with PIL's antialiased 8-bit bicubic (once or twice), flip, ToTensor,
// Normalize, RandomErasing(mode='pixel'); and the evaluation transform (Resize -> CenterCrop -> ToTensor -> Normalize)
// through the same stages.  vsom_augment_plan draws every sample's boxes from (seed, epoch, dataset index) alone.
// vsom_randaug_plan / vsom_augment_batch_ra (second half of the file) add torchvision's RandAugment and timm's rand-m9
// auto-augment to the training transform, as a per-sample record of PIL primitives executed between the crops.
#include "augment_common.h"

namespace vsom {

constexpr int AUG_THREADS = 512;
constexpr int AUG_MAXT = 17;       // taps of one output pixel: 2 ceil(2 scale) + 1 with scale <= 4
constexpr int AUG_KPAD = 20;       // ... padded with zero coefficients to whole groups of four
constexpr int AUG_KLD = 21;        // row stride of the coefficient table in LDS (odd: rows fall on different banks)
constexpr int AUG_MAXO = 73;       // largest output size of one pass: int(64 / 0.875)
constexpr int AUG_SRC_BYTES = 3 * 64 * 64 + 256;   // slack: a padded tap group may read up to 3 rows past the image
constexpr int AUG_BUF_BYTES = 16384;   // >= 3 * 64 * 73 (horizontal pass of the evaluation resize) and >= 3 * 73 * 73

// ---------------------------------------------------------------- the plan (draws: augment_common.h)
__global__ __launch_bounds__(256) void augment_plan_kernel(const int64_t* __restrict__ index, long N, int B, int H, int S, BoxDraw d1,
                                                           BoxDraw d2, int two, double flip_p, double erase_p, uint32_t k0,
                                                           uint32_t k1, uint32_t epoch, int* __restrict__ params) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    long row = index[b];
    row = row < 0 ? 0 : (row >= N ? N - 1 : row);          // clamped as augment_batch_kernel clamps it: one key for both
    const uint32_t idx = (uint32_t)row;
    plan_row(H, H, S, d1, d2, two, flip_p, erase_p, idx, epoch, k0, k1, params + (long)b * AUG_P);
}

// ---------------------------------------------------------------- the resampler
struct CoefTab {
    int kk[AUG_MAXO][AUG_KLD];
    short xmin[AUG_MAXO], n[AUG_MAXO];
};

// Row xx of PIL's precompute_coeffs + normalize_coeffs_8bpc for in -> out pixels (augment_common.h).
__device__ void coef_row(CoefTab& t, int in, int out, int xx) {
    const TapRange r = tap_range(in, out, xx, AUG_MAXT);    // the limit is never met for in <= 4 out (checked by the host)
    const double ww = tap_sum(r);
    for (int x = 0; x < r.n; ++x) t.kk[xx][x] = tap_coef(r, ww, x);
    for (int x = r.n; x < AUG_KPAD; ++x) t.kk[xx][x] = 0;
    t.xmin[xx] = (short)r.xmin;
    t.n[xx] = (short)r.n;
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

// The output stage of both batch kernels: flip, ToTensor, Normalize, erase; element (c, y, x) of the output reads level
// (y + off, x + off) of the R x R image `fin`; erase box (et, el, eh, ew) inside S x S.
__device__ __forceinline__ void emit_output(const unsigned char* fin, int C, int S, int R, int off, bool flip, int et, int el, int eh,
                                            int ew, const float* __restrict__ mean, const float* __restrict__ stdv, long idx,
                                            uint32_t k0, uint32_t k1, uint32_t epoch, float* __restrict__ out,
                                            unsigned char* __restrict__ out_u8) {
    const int tid = threadIdx.x, b = blockIdx.x;
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
    // torchvision's RandAugment (data.py:301) acts here, on the 8-bit image in bufC: after crop 1, before crop 2 ...
    if (two) {
        crop_resize(bufC, S * S, S, i2, j2, h2, w2, C, S, bufA, bufB, th, tv);
        fin = bufB;
        // ... and timm's rand-m9 auto-augment (inside create_transform, data.py:288-298) here, on bufB: after crop 2
        // (augment_batch_ra_kernel below; this kernel applies neither)
    }

    emit_output(fin, C, S, R, off, flip, et, el, eh, ew, mean, stdv, idx, k0, k1, epoch, out, out_u8);
}

// ================================================================ RandAugment / rand-m9 (vsom_randaug_plan, vsom_augment_batch_ra)
// The second per-sample record: RA_WORDS int32 = {flip 1, flip 2, six words the batch kernel does not read}, then four op
// slots of RA_SLOT_WORDS: {primitive, integer parameter, fp32 factor, fill R | G << 8 | B << 16, six doubles}.  A slot is one
// PIL primitive with its parameters; which policy asked for it is the plan's business.
constexpr int RA_WORDS = 72, RA_SLOT0 = 8, RA_SLOT_WORDS = 16;
enum RaOp { RA_NONE = 0, RA_AFFINE_NEAREST, RA_AFFINE_BICUBIC, RA_BRIGHTNESS, RA_COLOR, RA_CONTRAST, RA_SHARPNESS, RA_POSTERIZE,
            RA_SOLARIZE, RA_SOLARIZE_ADD, RA_INVERT, RA_AUTOCONTRAST, RA_EQUALIZE, RA_NOPS };
constexpr uint32_t AUG_STREAM_RA = 2;
constexpr double RA_COEF_MAX = 16384.0;            // |coefficient| bound of a record made safe (PIL's own 16.16 path ends at 32768)

struct RaSlot {
    int op, ip;
    float f;
    uint32_t fill;
    double a[6];
};
struct RaScratch {
    int hist[3][256];
    unsigned char lut[3][256];
    int sum;
};

// A slot as the caller wrote it, made safe: an unknown primitive does nothing, NaN and huge numbers become finite ones.
__device__ RaSlot load_slot(const int* __restrict__ rec, int s) {
    const int* w = rec + RA_SLOT0 + s * RA_SLOT_WORDS;
    RaSlot r;
    r.op = w[0];
    if ((unsigned)r.op >= (unsigned)RA_NOPS) r.op = RA_NONE;
    r.ip = min(max(w[1], 0), 256);
    r.f = __int_as_float(w[2]);
    r.f = r.f == r.f ? fminf(fmaxf(r.f, -1e6f), 1e6f) : 1.f;
    r.fill = (uint32_t)w[3];
    const double* d = reinterpret_cast<const double*>(w + 4);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const double v = d[i];
        r.a[i] = v == v ? fmin(fmax(v, -RA_COEF_MAX), RA_COEF_MAX) : 0.0;
    }
    return r;
}

// Image.transform(AFFINE, NEAREST): libImaging's affine_fixed, 16.16 fixed point (in 64 bits: no wrap for any safe record).
__device__ void affine_nearest(const unsigned char* src, unsigned char* dst, int C, int S, const RaSlot& s) {
#pragma clang fp contract(off)
    auto fix = [](double v) { return (long long)floor(v * 65536.0 + 0.5); };
    const long long a0 = fix(s.a[0]), a1 = fix(s.a[1]), a3 = fix(s.a[3]), a4 = fix(s.a[4]);
    const long long a2 = fix(s.a[2] + s.a[0] * 0.5 + s.a[1] * 0.5), a5 = fix(s.a[5] + s.a[3] * 0.5 + s.a[4] * 0.5);
    const int SS = S * S;
    for (int pos = threadIdx.x; pos < SS; pos += AUG_THREADS) {
        const int y = pos / S, x = pos - y * S;
        const long long xi = (a2 + a1 * y + a0 * x) >> 16, yi = (a5 + a4 * y + a3 * x) >> 16;
        const bool in = xi >= 0 && xi < S && yi >= 0 && yi < S;
        const int from = in ? (int)yi * S + (int)xi : 0;
        for (int c = 0; c < C; ++c) dst[c * SS + pos] = in ? src[c * SS + from] : (unsigned char)(s.fill >> (8 * c));
    }
}

__device__ __forceinline__ double cubic4(double v1, double v2, double v3, double v4, double d) {
#pragma clang fp contract(off)
    const double p1 = v2, p2 = -v1 + v3, p3 = 2 * (v1 - v2) + v3 - v4, p4 = -v1 + v2 - v3 + v4;
    return p1 + d * (p2 + d * (p3 + d * p4));
}

// Image.transform(AFFINE, BICUBIC): libImaging's generic affine loop with bicubic_filter8, in doubles.  PIL walks the
// image adding a0 per pixel and a1 per row; the sums are repeated here addition by addition (a product a0 * x rounds
// differently in the last bit, and a byte follows).  A thread takes a run of consecutive pixels in PIL's order, so it pays
// the additions up to its first pixel once and one addition per pixel after that.
__device__ void affine_bicubic(const unsigned char* src, unsigned char* dst, int C, int S, const RaSlot& s) {
#pragma clang fp contract(off)
    const double a0 = s.a[0], a1 = s.a[1], a3 = s.a[3], a4 = s.a[4];
    double rx = s.a[2] + a0 * 0.5 + a1 * 0.5, ry = s.a[5] + a3 * 0.5 + a4 * 0.5;
    const int SS = S * S, run = (SS + AUG_THREADS - 1) / AUG_THREADS;
    const double lim = (double)S;
    int pos = threadIdx.x * run;
    const int end = min(pos + run, SS);
    if (pos >= end) return;
    const int y = pos / S;
    int x = pos - y * S;
    for (int k = 0; k < y; ++k) { rx += a1; ry += a4; }
    double xx = rx, yy = ry;
    for (int k = 0; k < x; ++k) { xx += a0; yy += a3; }
    for (; pos < end; ++pos) {
        if (xx < 0.0 || xx >= lim || yy < 0.0 || yy >= lim) {
            for (int c = 0; c < C; ++c) dst[c * SS + pos] = (unsigned char)(s.fill >> (8 * c));
        } else {
            const double xin = xx - 0.5, yin = yy - 0.5;
            const double fx = floor(xin), fy = floor(yin);
            const double dx = xin - fx, dy = yin - fy;
            const int x0 = (int)fx - 1, y0 = (int)fy - 1;
            int cx[4], cy[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                cx[k] = min(max(x0 + k, 0), S - 1);
                cy[k] = min(max(y0 + k, 0), S - 1) * S;
            }
            for (int c = 0; c < C; ++c) {
                const unsigned char* pl = src + c * SS;
                double v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const unsigned char* in = pl + cy[r];
                    v[r] = cubic4((double)in[cx[0]], (double)in[cx[1]], (double)in[cx[2]], (double)in[cx[3]], dx);
                }
                const double t = cubic4(v[0], v[1], v[2], v[3], dy);
                dst[c * SS + pos] = t <= 0.0 ? 0 : (t >= 255.0 ? 255 : (unsigned char)(int)t);
            }
        }
        if (++x == S) {
            x = 0;
            rx += a1; ry += a4;
            xx = rx; yy = ry;
        } else {
            xx += a0; yy += a3;
        }
    }
}

// Image.blend(a, b, alpha): fp32, truncated; clipped when alpha lies outside [0, 1]
__device__ __forceinline__ unsigned char blend8(int a, int b, float al) {
#pragma clang fp contract(off)
    const float t = (float)a + al * (float)(b - a);
    if (al >= 0.f && al <= 1.f) return (unsigned char)(int)t;
    return t <= 0.f ? 0 : (t >= 255.f ? 255 : (unsigned char)(int)t);
}

__device__ __forceinline__ int luminance(const unsigned char* img, int C, int SS, int pos) {     // ImageConvert's rgb2l
    if (C == 1) return img[pos];
    return (19595 * img[pos] + 38470 * img[SS + pos] + 7471 * img[2 * SS + pos] + 0x8000) >> 16;
}

// ImageEnhance.Brightness / Color / Contrast (in place) and Sharpness (cur -> alt).  Returns the buffer with the result.
__device__ unsigned char* enhance(unsigned char* cur, unsigned char* alt, int C, int S, const RaSlot& s, RaScratch& sc) {
#pragma clang fp contract(off)
    const int SS = S * S, tid = threadIdx.x;
    if (s.op == RA_SHARPNESS) {
        // ImageFilter.SMOOTH: fp32 weights {1 1 1, 1 5 1, 1 1 1} / 13, a row of three at a time, from 0.5; the border is copied
        const float k1 = 1.f / 13.f, k5 = 5.f / 13.f;
        for (int e = tid; e < C * SS; e += AUG_THREADS) {
            const int pos = e % SS, y = pos / S, x = pos - y * S;
            const unsigned char* p = cur + e;
            int sm = p[0];
            if (x > 0 && y > 0 && x < S - 1 && y < S - 1) {
                float ss = 0.5f;
                ss += (float)p[S - 1] * k1 + (float)p[S] * k1 + (float)p[S + 1] * k1;
                ss += (float)p[-1] * k1 + (float)p[0] * k5 + (float)p[1] * k1;
                ss += (float)p[-S - 1] * k1 + (float)p[-S] * k1 + (float)p[-S + 1] * k1;
                sm = ss <= 0.f ? 0 : (ss >= 255.f ? 255 : (int)ss);
            }
            alt[e] = blend8(sm, p[0], s.f);
        }
        __syncthreads();
        return alt;
    }
    int mean = 0;
    if (s.op == RA_CONTRAST) {                              // int(mean of L + 0.5): ImageStat's sum / count in doubles
        if (tid == 0) sc.sum = 0;
        __syncthreads();
        int part = 0;
        for (int pos = tid; pos < SS; pos += AUG_THREADS) part += luminance(cur, C, SS, pos);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
        if ((tid & 63) == 0) atomicAdd(&sc.sum, part);
        __syncthreads();
        mean = (int)((double)sc.sum / (double)SS + 0.5);
    }
    for (int pos = tid; pos < SS; pos += AUG_THREADS) {
        const int deg = s.op == RA_BRIGHTNESS ? 0 : (s.op == RA_COLOR ? luminance(cur, C, SS, pos) : mean);
        for (int c = 0; c < C; ++c) cur[c * SS + pos] = blend8(deg, cur[c * SS + pos], s.f);
    }
    __syncthreads();
    return cur;
}

// ImageOps.posterize / solarize / invert / autocontrast / equalize and timm's solarize_add: a 256-entry table per channel,
// then one pass over the image, in place.  Waves 0 .. C - 1 scan the histogram of their channel, four bins a lane.
__device__ void lut_op(unsigned char* cur, int C, int S, const RaSlot& s, RaScratch& sc) {
#pragma clang fp contract(off)
    const int SS = S * S, tid = threadIdx.x;
    if (s.op == RA_AUTOCONTRAST || s.op == RA_EQUALIZE) {
        for (int e = tid; e < 3 * 256; e += AUG_THREADS) (&sc.hist[0][0])[e] = 0;
        __syncthreads();
        for (int e = tid; e < C * SS; e += AUG_THREADS) atomicAdd(&sc.hist[e / SS][cur[e]], 1);
        __syncthreads();
        const int w = tid >> 6, l = tid & 63;
        if (w < C) {
            int h[4], part = 0, lo = 256, hi = -1, filled = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                h[q] = sc.hist[w][4 * l + q];
                part += h[q];
                if (h[q]) { lo = min(lo, 4 * l + q); hi = 4 * l + q; ++filled; }
            }
            int incl = part;                                // inclusive scan of the lanes' sums
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int up = __shfl_up(incl, o, 64);
                if (l >= o) incl += up;
            }
            const int total = __shfl(incl, 63, 64);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                lo = min(lo, __shfl_xor(lo, o, 64));
                hi = max(hi, __shfl_xor(hi, o, 64));
                filled += __shfl_xor(filled, o, 64);
            }
            if (s.op == RA_AUTOCONTRAST) {
                const bool same = hi <= lo;
                const double scale = same ? 1.0 : 255.0 / (double)(hi - lo), offset = same ? 0.0 : (double)(-lo) * scale;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int i = 4 * l + q, v = (int)((double)i * scale + offset);
                    sc.lut[w][i] = (unsigned char)(same ? i : min(max(v, 0), 255));
                }
            } else {
                const int step = hi >= 0 ? (total - sc.hist[w][hi]) / 255 : 0;
                const bool same = filled <= 1 || step == 0;
                int n = step / 2 + incl - part;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int i = 4 * l + q;
                    sc.lut[w][i] = (unsigned char)(same ? i : min(255, n / max(step, 1)));
                    n += h[q];
                }
            }
        }
    } else {
        for (int e = tid; e < 256; e += AUG_THREADS) {
            int v = e;
            if (s.op == RA_POSTERIZE) v = e & ((0xFF << (8 - min(s.ip, 8))) & 0xFF);
            else if (s.op == RA_SOLARIZE) v = e < s.ip ? e : 255 - e;
            else if (s.op == RA_SOLARIZE_ADD) v = e < 128 ? min(255, e + s.ip) : e;
            else if (s.op == RA_INVERT) v = 255 - e;
            sc.lut[0][e] = sc.lut[1][e] = sc.lut[2][e] = (unsigned char)v;
        }
    }
    __syncthreads();
    for (int e = tid; e < C * SS; e += AUG_THREADS) cur[e] = sc.lut[e / SS][cur[e]];
    __syncthreads();
}

// One slot on the image in `cur` ([C][S][S]); `alt` is free.  Returns the buffer that holds the result; ends synchronised.
__device__ unsigned char* apply_slot(const int* __restrict__ rec, int slot, unsigned char* cur, unsigned char* alt, int C, int S,
                                     RaScratch& sc) {
    const RaSlot s = load_slot(rec, slot);
    switch (s.op) {
    case RA_NONE:
        return cur;
    case RA_AFFINE_NEAREST:
        affine_nearest(cur, alt, C, S, s);
        __syncthreads();
        return alt;
    case RA_AFFINE_BICUBIC:
        affine_bicubic(cur, alt, C, S, s);
        __syncthreads();
        return alt;
    case RA_BRIGHTNESS: case RA_COLOR: case RA_CONTRAST: case RA_SHARPNESS:
        return enhance(cur, alt, C, S, s, sc);
    default:
        lut_op(cur, C, S, s, sc);
        return cur;
    }
}

__device__ void flip_rows(unsigned char* img, int C, int S) {
    const int half = S >> 1, n = C * S * half;
    for (int e = threadIdx.x; e < n; e += AUG_THREADS) {
        const int x = e % half, r = e / half;
        unsigned char* row = img + r * S;
        const unsigned char t = row[x];
        row[x] = row[S - 1 - x];
        row[S - 1 - x] = t;
    }
    __syncthreads();
}

// vsom_augment_batch_ra: the training transform with both policies.  crop 1 -> slots 0, 1 -> flip 1 -> crop 2 -> flip 2 ->
// slots 2, 3 -> ToTensor / Normalize / erase; one workgroup per sample, the image never leaves LDS.  The merged flip of the
// crop plan (p[8]) is not read.  The image moves between the three buffers; the two it is not in are scratch.
__global__ __launch_bounds__(AUG_THREADS) void augment_batch_ra_kernel(const unsigned char* __restrict__ src, long N, int C, int H,
                                                               const int64_t* __restrict__ index, const int* __restrict__ params,
                                                               const int* __restrict__ ra, int S, const float* __restrict__ mean,
                                                               const float* __restrict__ stdv, uint32_t k0, uint32_t k1,
                                                               uint32_t epoch, float* __restrict__ out,
                                                               unsigned char* __restrict__ out_u8) {
    __shared__ __attribute__((aligned(16))) unsigned char bufA[AUG_SRC_BYTES];
    __shared__ __attribute__((aligned(16))) unsigned char bufB[AUG_BUF_BYTES];
    __shared__ __attribute__((aligned(16))) unsigned char bufC[AUG_BUF_BYTES];
    __shared__ CoefTab th, tv;
    __shared__ RaScratch sc;
    const int tid = threadIdx.x, b = blockIdx.x;
    long idx = index[b];
    idx = idx < 0 ? 0 : (idx >= N ? N - 1 : idx);

    int p[13];
#pragma unroll
    for (int i = 0; i < 13; ++i) p[i] = params[(long)b * AUG_P + i];
    const int h1 = min(max(p[2], 1), H), w1 = min(max(p[3], 1), H);
    const int i1 = min(max(p[0], 0), H - h1), j1 = min(max(p[1], 0), H - w1);
    const bool two = p[6] > 0 && p[7] > 0;
    const int h2 = min(max(p[6], 1), S), w2 = min(max(p[7], 1), S);
    const int i2 = min(max(p[4], 0), S - h2), j2 = min(max(p[5], 0), S - w2);
    const int eh = min(max(p[11], 0), S), ew = min(max(p[12], 0), S);
    const int et = min(max(p[9], 0), S - eh), el = min(max(p[10], 0), S - ew);
    const int* rec = ra + (long)b * RA_WORDS;
    const bool flip1 = rec[0] != 0, flip2 = rec[1] != 0;

    const int img = C * H * H;
    const unsigned char* g = src + idx * img;
    if ((img & 15) == 0 && ((uintptr_t)src & 15) == 0) {
        for (int e = tid; e < img / 16; e += AUG_THREADS) reinterpret_cast<uint4*>(bufA)[e] = reinterpret_cast<const uint4*>(g)[e];
    } else {
        for (int e = tid; e < img; e += AUG_THREADS) bufA[e] = g[e];
    }
    __syncthreads();

    crop_resize(bufA, H * H, H, i1, j1, h1, w1, C, S, bufB, bufC, th, tv);
    unsigned char *cur = bufC, *f1 = bufB, *f2 = bufA;      // the image; two free buffers
    auto slot = [&](int k) {
        unsigned char* r = apply_slot(rec, k, cur, f1, C, S, sc);
        if (r != cur) { f1 = cur; cur = r; }
    };
    slot(0);
    slot(1);
    if (flip1) flip_rows(cur, C, S);
    if (two) {
        crop_resize(cur, S * S, S, i2, j2, h2, w2, C, S, f1, f2, th, tv);
        unsigned char* t = cur; cur = f2; f2 = t;
    }
    if (flip2) flip_rows(cur, C, S);
    slot(2);
    slot(3);
    emit_output(cur, C, S, S, 0, false, et, el, eh, ew, mean, stdv, idx, k0, k1, epoch, out, out_u8);
}

// ---------------------------------------------------------------- the record's draws
struct RaPolicy {
    int n_tv, timm;             // slots of the torchvision stage (0 .. 2); timm stage on / off
    double flip1_p;
    uint32_t fill_tv, fill_timm;
};

// Image.rotate's inverse map about (S / 2, S / 2).  PIL rounds cos and sin to 15 decimals with Python's round(); rint of
// the scaled value is that up to the last bit of the double.
__device__ void rotate_matrix(double angle, int S, double* m) {
#pragma clang fp contract(off)
    angle = fmod(angle, 360.0);
    if (angle < 0.0) angle += 360.0;
    const double t = -(angle * (3.14159265358979323846 / 180.0));
    const double c = rint(cos(t) * 1e15) / 1e15, sn = rint(sin(t) * 1e15) / 1e15;
    const double cx = (double)S / 2.0;
    m[0] = c; m[1] = sn; m[3] = -sn; m[4] = c;
    m[2] = (c * -cx + sn * -cx + 0.0) + cx;
    m[5] = (-sn * -cx + c * -cx + 0.0) + cx;
}

// What a policy draws for one slot; all zero: the slot stays empty.  The matrix is made once, when the slot is written.
enum RaMap { RA_MAP_NONE = 0, RA_MAP_A1, RA_MAP_A3, RA_MAP_A2, RA_MAP_A5, RA_MAP_ROTATE };   // v is that coefficient / the angle
struct SlotDraw {
    int op, ip;
    float f;
    uint32_t fill;
    int map;
    double v;
};

__device__ void write_slot(int* rec, int s, const SlotDraw& d, int S) {
    double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0, m5 = 0.0;
    if (d.map == RA_MAP_ROTATE) {
        double m[6];
        rotate_matrix(d.v, S, m);
        m0 = m[0]; m1 = m[1]; m2 = m[2]; m3 = m[3]; m4 = m[4]; m5 = m[5];
    } else if (d.map != RA_MAP_NONE) {
        m0 = 1.0; m4 = 1.0;
        if (d.map == RA_MAP_A1) m1 = d.v;
        else if (d.map == RA_MAP_A3) m3 = d.v;
        else if (d.map == RA_MAP_A2) m2 = d.v;
        else m5 = d.v;
    }
    auto lo = [](double v) { return (int)(uint32_t)__double_as_longlong(v); };
    auto hi = [](double v) { return (int)(uint32_t)((unsigned long long)__double_as_longlong(v) >> 32); };
    int4* w = reinterpret_cast<int4*>(rec + RA_SLOT0 + s * RA_SLOT_WORDS);
    w[0] = make_int4(d.op, d.ip, __float_as_int(d.f), (int)d.fill);
    w[1] = make_int4(lo(m0), hi(m0), lo(m1), hi(m1));
    w[2] = make_int4(lo(m2), hi(m2), lo(m3), hi(m3));
    w[3] = make_int4(lo(m4), hi(m4), lo(m5), hi(m5));
}

// torchvision RandAugment(num_ops, magnitude 9 of 31 bins): op k of the 14, negated when sg = -1; NEAREST
__device__ SlotDraw tv_draw(int k, double sg, int S, uint32_t fill) {
#pragma clang fp contract(off)
    const double bin = 9.0 / 30.0;
    SlotDraw d = {RA_NONE, 0, 1.f, 0u, RA_MAP_NONE, 0.0};
    switch (k) {
    case 0: d.f = 0.f; break;                                                                            // Identity: empty
    case 1: case 2:                                                                                      // ShearX, ShearY
        d.op = RA_AFFINE_NEAREST; d.fill = fill; d.map = k == 1 ? RA_MAP_A1 : RA_MAP_A3;
        d.v = sg * tan(atan(0.3 * bin));
        break;
    case 3: case 4:                                                                                      // TranslateX, TranslateY
        d.op = RA_AFFINE_NEAREST; d.fill = fill; d.map = k == 3 ? RA_MAP_A2 : RA_MAP_A5;
        d.v = -(sg * (double)(int)(150.0 / 331.0 * (double)S * 0.3));
        break;
    case 5:                                                                                              // Rotate
        d.op = RA_AFFINE_NEAREST; d.fill = fill; d.map = RA_MAP_ROTATE;
        d.v = sg * (30.0 * bin);
        break;
    case 6: case 7: case 8: case 9:                                                                      // Brightness .. Sharpness
        d.op = k == 6 ? RA_BRIGHTNESS : (k == 7 ? RA_COLOR : (k == 8 ? RA_CONTRAST : RA_SHARPNESS));
        d.f = (float)(1.0 + sg * (0.9 * bin));
        break;
    case 10: d.op = RA_POSTERIZE; d.ip = 7; break;                                                       // 8 - round(9 / 7.5) bits
    case 11: d.op = RA_SOLARIZE; d.ip = 179; break;                                                      // i < 178.5
    case 12: d.op = RA_AUTOCONTRAST; break;
    default: d.op = RA_EQUALIZE; break;
    }
    return d;
}

// timm rand-m9-mstd0.5-inc1: op k of the 15 at level lv = m / 10; BICUBIC
__device__ SlotDraw timm_draw(int k, double sg, double lv, int S, uint32_t fill) {
#pragma clang fp contract(off)
    SlotDraw d = {RA_NONE, 0, 1.f, 0u, RA_MAP_NONE, 0.0};
    switch (k) {
    case 0: d.op = RA_AUTOCONTRAST; break;
    case 1: d.op = RA_EQUALIZE; break;
    case 2: d.op = RA_INVERT; break;
    case 3:
        d.op = RA_AFFINE_BICUBIC; d.fill = fill; d.map = RA_MAP_ROTATE;
        d.v = sg * (lv * 30.0);
        break;
    case 4: d.op = RA_POSTERIZE; d.ip = 4 - (int)(lv * 4); break;
    case 5: d.op = RA_SOLARIZE; d.ip = 256 - (int)(lv * 256); break;
    case 6: d.op = RA_SOLARIZE_ADD; d.ip = min(128, (int)(lv * 110)); break;
    case 7: case 8: case 9: case 10:
        d.op = k == 7 ? RA_COLOR : (k == 8 ? RA_CONTRAST : (k == 9 ? RA_BRIGHTNESS : RA_SHARPNESS));
        d.f = (float)fmax(0.1, 1.0 + sg * (lv * 0.9));
        break;
    case 11: case 12:
        d.op = RA_AFFINE_BICUBIC; d.fill = fill; d.map = k == 11 ? RA_MAP_A1 : RA_MAP_A3;
        d.v = sg * (lv * 0.3);
        break;
    default:
        d.op = RA_AFFINE_BICUBIC; d.fill = fill; d.map = k == 13 ? RA_MAP_A2 : RA_MAP_A5;
        d.v = sg * (lv * 0.45) * (double)S;
        break;
    }
    return d;
}

// One thread per sample.  Philox blocks of the record's stream: 0 the flips; 1, 2 the torchvision slots (pick, sign);
// 3 + 3 t, 4 + 3 t, 5 + 3 t timm slot t (pick and apply; the two uniforms of the normal draw; sign).
__global__ __launch_bounds__(256) void randaug_plan_kernel(const int64_t* __restrict__ index, long N, int B, int S, RaPolicy pol,
                                                           uint32_t k0, uint32_t k1, uint32_t epoch, int* __restrict__ out) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    long rowi = index[b];
    rowi = rowi < 0 ? 0 : (rowi >= N ? N - 1 : rowi);
    const uint32_t idx = (uint32_t)rowi;
    int* rec = out + (long)b * RA_WORDS;
    uint32_t r[4];
    philox4x32_10(0, idx, AUG_STREAM_RA, epoch, k0, k1, r);
    const int flip1 = u53(r[0], r[1]) < pol.flip1_p ? 1 : 0, flip2 = u53(r[2], r[3]) < 0.5 ? 1 : 0;
    int pick[4] = {-1, -1, -1, -1}, applied = 0;
    const SlotDraw empty = {RA_NONE, 0, 0.f, 0u, RA_MAP_NONE, 0.0};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        SlotDraw d = empty;
        if (s < pol.n_tv) {
            philox4x32_10(1 + s, idx, AUG_STREAM_RA, epoch, k0, k1, r);
            pick[s] = randint_below(u53(r[0], r[1]), 14);
            d = tv_draw(pick[s], u53(r[2], r[3]) < 0.5 ? -1.0 : 1.0, S, pol.fill_tv);
        }
        write_slot(rec, s, d, S);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        SlotDraw d = empty;
        if (pol.timm) {
            const uint32_t blk = 3 + 3 * t;
            philox4x32_10(blk, idx, AUG_STREAM_RA, epoch, k0, k1, r);
            pick[2 + t] = randint_below(u53(r[0], r[1]), 15);
            if (u53(r[2], r[3]) < 0.5) {
                applied |= 1 << t;
                philox4x32_10(blk + 1, idx, AUG_STREAM_RA, epoch, k0, k1, r);
                const double z = sqrt(-2.0 * log(1.0 - u53(r[0], r[1]))) * cos(6.283185307179586 * u53(r[2], r[3]));
                const double mag = fmin(10.0, fmax(0.0, 9.0 + 0.5 * z));           // clamp(N(9, 0.5), 0, 10)
                philox4x32_10(blk + 2, idx, AUG_STREAM_RA, epoch, k0, k1, r);
                d = timm_draw(pick[2 + t], u53(r[0], r[1]) < 0.5 ? -1.0 : 1.0, mag / 10.0, S, pol.fill_timm);
            }
        }
        write_slot(rec, 2 + t, d, S);
    }
    int4* head = reinterpret_cast<int4*>(rec);
    head[0] = make_int4(flip1, flip2, pick[0], pick[1]);
    head[1] = make_int4(pick[2], pick[3], applied, 0);
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
    return vsom::launch_status("augment_plan_kernel");
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
    return vsom::launch_status("augment_batch_kernel");
}

int vsom_randaug_plan(const int64_t* index, long N, int B, int S, int randaug_n, int autoaugment, double flip1_p, uint32_t fill_tv,
                      uint32_t fill_timm, uint64_t seed, int epoch, int32_t* ra, vsom_stream_t stream) {
    VSOM_REQUIRE(index && ra, VSOM_EINVAL, "randaug_plan: null pointer");
    VSOM_REQUIRE(N > 0 && B > 0 && S > 0 && epoch >= 0, VSOM_EINVAL, "randaug_plan: bad sizes (N=%ld B=%d S=%d epoch=%d)", N, B, S, epoch);
    VSOM_REQUIRE(S <= 64 && N < (1L << 31), VSOM_EUNSUPPORTED, "randaug_plan: S=%d (at most 64), N=%ld (below 2^31)", S, N);
    VSOM_REQUIRE(randaug_n >= 0 && randaug_n <= 2, VSOM_EUNSUPPORTED, "randaug_plan: randaug_n=%d (the record holds 0 to 2 slots)", randaug_n);
    VSOM_REQUIRE(flip1_p >= 0 && flip1_p <= 1, VSOM_EINVAL, "randaug_plan: probability outside [0, 1]");
    VSOM_REQUIRE(fill_tv < (1u << 24) && fill_timm < (1u << 24), VSOM_EINVAL, "randaug_plan: a fill is three 8-bit levels");
    VSOM_REQUIRE(vsom::aligned16(ra), VSOM_EALIGN, "randaug_plan: the record must be 16-byte aligned");
    const vsom::RaPolicy pol = {randaug_n, autoaugment != 0, flip1_p, fill_tv, fill_timm};
    VSOM_LAUNCH(vsom::randaug_plan_kernel, dim3(vsom::cdiv(B, 256)), dim3(256), 0, stream, index, N, B, S, pol, (uint32_t)seed,
                (uint32_t)(seed >> 32), (uint32_t)epoch, ra);
    return vsom::launch_status("randaug_plan_kernel");
}

int vsom_augment_batch_ra(const unsigned char* src, long N, int C, int H, int W, const int64_t* index, const int32_t* params,
                          const int32_t* ra, int B, int S, const float* mean, const float* std, uint64_t seed, int epoch,
                          float* out, unsigned char* out_u8, vsom_stream_t stream) {
    VSOM_REQUIRE(src && index && params && ra && mean && std && out, VSOM_EINVAL, "augment_batch_ra: null pointer");
    VSOM_REQUIRE(N > 0 && B > 0 && H > 0 && W > 0 && S > 0 && epoch >= 0, VSOM_EINVAL,
                 "augment_batch_ra: bad sizes (N=%ld B=%d H=%d W=%d S=%d epoch=%d)", N, B, H, W, S, epoch);
    VSOM_REQUIRE(C == 1 || C == 3, VSOM_EUNSUPPORTED, "augment_batch_ra: %d channels (1 or 3)", C);
    VSOM_REQUIRE(H == W && H <= 64, VSOM_EUNSUPPORTED, "augment_batch_ra: %d x %d source (square, at most 64 x 64)", H, W);
    VSOM_REQUIRE(S <= 64 && N < (1L << 31), VSOM_EUNSUPPORTED, "augment_batch_ra: S=%d (at most 64), N=%ld (below 2^31)", S, N);
    VSOM_REQUIRE(H <= 4 * S, VSOM_EUNSUPPORTED, "augment_batch_ra: %d -> %d shrinks by more than 4", H, S);
    VSOM_REQUIRE(vsom::aligned16(out) && vsom::aligned16(params) && vsom::aligned16(ra) && ((uintptr_t)out_u8 & 3) == 0, VSOM_EALIGN,
                 "augment_batch_ra: out, params and the record must be 16-byte aligned");
    VSOM_LAUNCH(vsom::augment_batch_ra_kernel, dim3(B), dim3(vsom::AUG_THREADS), 0, stream, src, N, C, H, index, params, ra, S, mean,
                std, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)epoch, out, out_u8);
    return vsom::launch_status("augment_batch_ra_kernel");
}

}  // extern "C"
