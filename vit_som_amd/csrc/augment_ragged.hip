// The data pipeline for image sets whose images differ in size (flowers-17 / -102: data/data.py:299-313): the set lives in
// one flat uint8 buffer, each image planar [C][H_n][W_n] at a 16-byte aligned offset, with an (H_n, W_n) table.  The
// transform is augment.hip's -- RandomResizedCrop (once or twice), flip, ToTensor, Normalize, RandomErasing(pixel); Resize ->
// CenterCrop for evaluation -- with PIL's 8-bit antialiased bicubic byte for byte, for sources up to 2048 px a side and
// outputs up to 224 x 224.  A sample does not fit in LDS, so a workgroup owns one sample and one band of output rows and
// walks the band in chunks (ragged_pass_kernel).  Training is two launches of that kernel (crop 1 -> 8-bit scratch; crop 2 of
// the scratch -> output stage), evaluation one.
#include <type_traits>

#include "augment_common.h"

namespace vsom {

constexpr int RG_THREADS = 256;
constexpr int RG_MAXS = 224, RG_MAXR = 256, RG_MAXDIM = 2048, RG_SHRINK = 8;
constexpr int RG_MAXT = 33;            // taps of one output pixel: 2 ceil(2 scale) + 1 with scale <= 8
constexpr int RG_KPAD = 36;            // ... padded with zero coefficients to whole groups of four
constexpr int RG_KLD = 37;             // row stride of the vertical table in LDS (odd: rows fall on different banks)
constexpr int RG_BAND = 32;            // output rows of one workgroup
constexpr int RG_CHUNK = 16;           // output rows of one chunk at most
constexpr int RG_TMP_BYTES = 32768;    // horizontal-pass rows [slot][C][S], a ring over the crop's rows
constexpr int RG_STG_BYTES = 12288;    // staged source row segments, 16 bytes of slack included
constexpr int RG_RES_BYTES = 3 * RG_CHUNK * RG_MAXS;       // a chunk's result before the output stage
// one staged segment: the columns a 224-wide window reaches at shrink 8 (223 * 8 + 2 * 16 + 1), shifted by up to 15 bytes
constexpr int RG_MAXSEG = ((RG_MAXS - 1) * RG_SHRINK + 4 * RG_SHRINK + 1 + 15 + 15) / 16 * 16;
static_assert(3 * RG_MAXSEG + 16 <= RG_STG_BYTES, "one source row of three channels must fit the staging buffer");
static_assert(RG_TMP_BYTES / (3 * RG_MAXS) >= RG_MAXT, "the ring must hold the rows one output row reads");
static_assert(RG_TMP_BYTES + RG_STG_BYTES + RG_RES_BYTES + RG_BAND * (RG_KLD + 1) * 4 <= 65536 - 256,
              "LDS per workgroup at most 64 KiB: two workgroups a CU");

enum RaggedMode { RG_CROP1 = 0, RG_CROP2 = 1, RG_EVAL = 2 };

__global__ __launch_bounds__(256) void augment_plan_ragged_kernel(const int64_t* __restrict__ index, const int* __restrict__ shapes,
                                                                  long N, int B, int S, BoxDraw d1, BoxDraw d2, int two, double flip_p,
                                                                  double erase_p, uint32_t k0, uint32_t k1, uint32_t epoch,
                                                                  int* __restrict__ params) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    long row = index[b];
    row = row < 0 ? 0 : (row >= N ? N - 1 : row);          // clamped as ragged_pass_kernel clamps it: one key for both
    const int Hs = min(max(shapes[2 * row], 1), RG_MAXDIM), Ws = min(max(shapes[2 * row + 1], 1), RG_MAXDIM);
    plan_row(Hs, Ws, S, d1, d2, two, flip_p, erase_p, (uint32_t)row, epoch, k0, k1, params + (long)b * AUG_P);
}

struct RaggedArgs {
    const unsigned char* data;      // the set (RG_CROP1, RG_EVAL) or the 8-bit scratch [B][C][S][S] (RG_CROP2)
    long data_bytes;
    const int64_t* offsets;
    const int* shapes;
    long N;
    int C, max_h, max_w;
    const int64_t* index;
    const int* params;
    int S, R, mode;
    const float *mean, *stdv;
    uint32_t k0, k1, epoch;
    unsigned char* scratch;         // RG_CROP1's result
    float* out;
    unsigned char* out_u8;
};

// A level times a coefficient.  A 32-bit integer multiply runs at a quarter of the 24-bit one's rate and the passes are
// bound by their multiply-adds, so the 24-bit form is used whenever every coefficient of the workgroup fits 24 signed
// bits (|c| < 2^23: always, as far as is known -- a normalised bicubic tap stays below 1.3 * 2^22 -- but the products must be
// PIL's whatever the table holds, so the workgroup checks and keeps the 32-bit form for the other case).
template <bool M24>
__device__ __forceinline__ int mulc(int level, int coef) {
    return M24 ? __mul24(level, coef) : level * coef;
}
__device__ __forceinline__ bool fits24(int coef) { return coef >= -(1 << 23) && coef < (1 << 23); }
// it / C and it % C for C = 1 or 3 and it < 32768, without a division
__device__ __forceinline__ void split_item(int it, int C, int& row, int& c) {
    row = C == 1 ? it : (it * 21846) >> 16;
    c = it - row * C;
}

// One crop-resize pass of one sample, output rows [band * RG_BAND, ...): box (i, j, h, w) of the H x W image at `base` is
// resized to OH x OW, of which the S x S window at (top, left) is computed.  Horizontal pass first with the 8-bit
// intermediate PIL keeps.  A thread owns one output column: its coefficient row stays in registers.  Source rows go through
// LDS in groups, loaded as aligned 16-byte vectors that cover the columns the window reaches; their horizontal results
// enter a ring of rows that the vertical pass of a chunk reads, so a source row is filtered once per band.
__global__ __launch_bounds__(RG_THREADS) void ragged_pass_kernel(const RaggedArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char tmp[RG_TMP_BYTES];
    __shared__ __attribute__((aligned(16))) unsigned char stg[RG_STG_BYTES];
    __shared__ __attribute__((aligned(16))) unsigned char res[RG_RES_BYTES];
    __shared__ int tvk[RG_BAND][RG_KLD];
    __shared__ short tvmin[RG_BAND], tvn[RG_BAND];
    const int tid = threadIdx.x, b = blockIdx.x, C = a.C, S = a.S;
    const int band0 = blockIdx.y * RG_BAND, nband = min(RG_BAND, S - band0);
    long idx = a.index[b];
    idx = idx < 0 ? 0 : (idx >= a.N ? a.N - 1 : idx);      // a bad index reads a wrong row, never outside the set

    // the plan, made safe: whatever the caller wrote, every box lies inside its image
    int p[13];
    if (a.params) {
#pragma unroll
        for (int i = 0; i < 13; ++i) p[i] = a.params[(long)b * AUG_P + i];
    } else {
#pragma unroll
        for (int i = 0; i < 13; ++i) p[i] = 0;
    }
    // the image, made safe: the shape inside the declared bounds, the offset so that the image lies inside the buffer
    int H, W;
    long base;
    if (a.mode == RG_CROP2) {
        H = W = S;
        base = (long)b * C * S * S;
    } else {
        H = min(max(a.shapes[2 * idx], 1), a.max_h);
        W = min(max(a.shapes[2 * idx + 1], 1), a.max_w);
        if ((long)C * H * W > a.data_bytes) H = W = 1;
        base = min(max((long)a.offsets[idx], 0L), a.data_bytes - (long)C * H * W);
    }
    int bi, bj, bh, bw, OH = S, OW = S, top = 0, left = 0;
    if (a.mode == RG_CROP1) {
        bh = min(max(p[2], 1), H); bw = min(max(p[3], 1), W);
        bi = min(max(p[0], 0), H - bh); bj = min(max(p[1], 0), W - bw);
    } else if (a.mode == RG_CROP2 && p[6] > 0 && p[7] > 0) {
        bh = min(max(p[6], 1), S); bw = min(max(p[7], 1), S);
        bi = min(max(p[4], 0), S - bh); bj = min(max(p[5], 0), S - bw);
    } else {
        // the whole image: S -> S passes every byte through (each coefficient row is a single 1); evaluation resizes the
        // shorter side to R and the longer to int(R * long / short) (torchvision's Resize), then takes the centre window
        bi = bj = 0; bh = H; bw = W;
        if (a.mode == RG_EVAL) {
            const int R = a.R;
            if (H <= W) { OH = R; OW = (int)((double)((long)R * W) / (double)H); }
            else { OW = R; OH = (int)((double)((long)R * H) / (double)W); }
            top = (int)rint((double)(OH - S) / 2.0);
            left = (int)rint((double)(OW - S) / 2.0);
        }
    }
    const bool flip = a.mode == RG_CROP2 && p[8] != 0;
    const int eh = a.mode == RG_CROP2 ? min(max(p[11], 0), S) : 0, ew = a.mode == RG_CROP2 ? min(max(p[12], 0), S) : 0;
    const int et = min(max(p[9], 0), S - eh), el = min(max(p[10], 0), S - ew);

    // the vertical table of the band, one thread a row
    bool small = true;                                      // this thread's coefficients fit 24 signed bits
    if (tid < nband) {
        const TapRange r = tap_range(bh, OH, top + band0 + tid, RG_MAXT);
        const double ww = tap_sum(r);
        for (int x = 0; x < r.n; ++x) {
            const int kx = tap_coef(r, ww, x);
            small = small && fits24(kx);
            tvk[tid][x] = kx;
        }
        tvmin[tid] = (short)r.xmin;
        tvn[tid] = (short)r.n;
    }
    // this thread's column: lanes run along the output row (the next power of two lanes per row)
    const int sh = S > 1 ? 32 - __clz(S - 1) : 0;
    const int xx = tid & ((1 << sh) - 1), r0 = tid >> sh, rstep = RG_THREADS >> sh;
    const bool live = xx < S;
    int k[RG_KPAD], cx = 0, kn = 0;
    const int xlo = tap_range(bw, OW, left, RG_MAXT).xmin;
    const TapRange last = tap_range(bw, OW, left + S - 1, RG_MAXT);
    const int seglen = last.xmin + last.n - xlo;
#pragma unroll
    for (int q = 0; q < RG_KPAD; ++q) k[q] = 0;
    if (live) {
        const TapRange r = tap_range(bw, OW, left + xx, RG_MAXT);
        const double ww = tap_sum(r);
#pragma unroll
        for (int q = 0; q < RG_MAXT; ++q) if (q < r.n) { k[q] = tap_coef(r, ww, q); small = small && fits24(k[q]); }
        cx = r.xmin - xlo;
        kn = r.n;
    }
    const int segpad = (seglen + 30) & ~15, vpi = segpad >> 4;
    if (segpad > RG_MAXSEG) return;                         // cannot happen inside the entry's limits; uniform, before any barrier
    const int rows_per_group = max((RG_STG_BYTES - 16) / (segpad * C), 1);
    const int CS = C * S, cap = RG_TMP_BYTES / CS;
    const long plane = (long)H * W;
    const bool m24 = __syncthreads_and(small) != 0;         // also the barrier behind the vertical table
    // staging: the next power of two lanes per segment, so that no index needs a division
    const int vsh = vpi > 1 ? 32 - __clz(vpi - 1) : 0;
    const int vq = tid & ((1 << vsh) - 1), vit0 = tid >> vsh, vstep = RG_THREADS >> vsh;

    int have = 0;                                           // source rows [.., have) of the crop have been filtered
    for (int r = 0; r < nband;) {
        // the chunk: as many rows as the ring holds at once
        const int lo = tvmin[r];
        int nr = 1, hi = lo + tvn[r];
        while (r + nr < nband && nr < RG_CHUNK && tvmin[r + nr] + tvn[r + nr] - lo <= cap) {
            hi = max(hi, tvmin[r + nr] + tvn[r + nr]);
            ++nr;
        }
        // horizontal pass over the crop's rows [max(have, lo), hi), a group at a time
        for (int y0 = max(have, lo); y0 < hi; y0 += rows_per_group) {
            const int nit = min(rows_per_group, hi - y0) * C;          // staged (row, channel) segments
            for (int it = vit0; it < nit; it += vstep) {
                int yy, c;
                split_item(it, C, yy, c);
                const int q = vq;
                const long g = base + c * plane + (long)(bi + y0 + yy) * W + bj + xlo;
                const int shift = (int)(g & 15);
                if (q * 16 < shift + seglen) {
                    const long ga = g - shift + q * 16;
                    uint4 val;
                    if (ga + 16 <= a.data_bytes) {
                        val = *reinterpret_cast<const uint4*>(a.data + ga);
                    } else {                                // the last vector of the buffer: byte by byte, zeros past the end
                        unsigned char t[16];
#pragma unroll
                        for (int e = 0; e < 16; ++e) t[e] = ga + e < a.data_bytes ? a.data[ga + e] : (unsigned char)0;
                        val = *reinterpret_cast<const uint4*>(t);
                    }
                    *reinterpret_cast<uint4*>(stg + it * segpad + q * 16) = val;
                }
            }
            __syncthreads();
            if (live) {
                const int slot0 = y0 % cap;
                auto hpass = [&](auto m) {
                    constexpr bool M24 = decltype(m)::value;
                    for (int it = r0; it < nit; it += rstep) {
                        int yy, c;
                        split_item(it, C, yy, c);
                        const long g = base + c * plane + (long)(bi + y0 + yy) * W + bj + xlo;
                        const unsigned char* row = stg + it * segpad + (int)(g & 15) + cx;
                        int acc = 1 << (AUG_PREC - 1);
#pragma unroll
                        for (int q = 0; q < RG_KPAD; q += 4) {
                            if (q < kn) {
                                const int b0 = row[q], b1 = row[q + 1], b2 = row[q + 2], b3 = row[q + 3];
                                acc += mulc<M24>(b0, k[q]) + mulc<M24>(b1, k[q + 1]) + mulc<M24>(b2, k[q + 2]) + mulc<M24>(b3, k[q + 3]);
                            }
                        }
                        const int slot = slot0 + yy < cap ? slot0 + yy : slot0 + yy - cap;     // a group has at most cap rows
                        tmp[slot * CS + c * S + xx] = clip8(acc);
                    }
                };
                if (m24) hpass(std::true_type{});
                else hpass(std::false_type{});
            }
            __syncthreads();
        }
        have = max(have, hi);
        // vertical pass of the chunk
        if (live) {
            for (int it = r0; it < nr * C; it += rstep) {
                int rr, c;
                split_item(it, C, rr, c);
                const int n = tvn[r + rr];
                const int* kv = tvk[r + rr];
                int slot = tvmin[r + rr] % cap;
                int acc = 1 << (AUG_PREC - 1);
                if (m24) {
                    for (int q = 0; q < n; ++q) {
                        acc += __mul24((int)tmp[slot * CS + c * S + xx], kv[q]);
                        if (++slot == cap) slot = 0;
                    }
                } else {
                    for (int q = 0; q < n; ++q) {
                        acc += (int)tmp[slot * CS + c * S + xx] * kv[q];
                        if (++slot == cap) slot = 0;
                    }
                }
                const unsigned char v = clip8(acc);
                if (a.mode == RG_CROP1) a.scratch[(((long)b * C + c) * S + band0 + r + rr) * S + xx] = v;
                else res[(c * RG_CHUNK + rr) * S + xx] = v;
            }
        }
        __syncthreads();
        // the output stage: flip, ToTensor, Normalize, erase (keyed as augment.hip's emit_output keys it)
        if (a.mode != RG_CROP1) {
            float* o = a.out + (long)b * C * S * S;
            unsigned char* o8 = a.out_u8 ? a.out_u8 + (long)b * C * S * S : nullptr;
            const uint32_t uidx = (uint32_t)idx;
            if ((S & 3) == 0) {
                const int q4 = S >> 2;
                for (int g = tid; g < C * nr * q4; g += RG_THREADS) {
                    const int xg = g % q4, t2 = g / q4, rr = t2 % nr, c = t2 / nr;
                    const int y = band0 + r + rr, x = 4 * xg, e4 = (c * S + y) * q4 + xg;
                    const unsigned char* line = res + (c * RG_CHUNK + rr) * S;
                    const float m = a.mean[c], sd = a.stdv[c];
                    unsigned char lv[4];
                    float v[4];
#pragma unroll
                    for (int t = 0; t < 4; ++t) { lv[t] = line[flip ? S - 1 - (x + t) : x + t]; v[t] = normalized(lv[t], m, sd); }
                    if (y >= et && y < et + eh && x + 3 >= el && x < el + ew) {
                        float nz[4];
                        noise4((uint32_t)e4, uidx, a.epoch, a.k0, a.k1, nz);
#pragma unroll
                        for (int t = 0; t < 4; ++t) if (x + t >= el && x + t < el + ew) v[t] = nz[t];
                    }
                    f32x4 vv = {v[0], v[1], v[2], v[3]};
                    *reinterpret_cast<f32x4*>(o + e4 * 4) = vv;
                    if (o8) *reinterpret_cast<uchar4*>(o8 + e4 * 4) = make_uchar4(lv[0], lv[1], lv[2], lv[3]);
                }
            } else {
                for (int g = tid; g < C * nr * S; g += RG_THREADS) {
                    const int x = g % S, t2 = g / S, rr = t2 % nr, c = t2 / nr;
                    const int y = band0 + r + rr, e = (c * S + y) * S + x;
                    const unsigned char lv = res[(c * RG_CHUNK + rr) * S + (flip ? S - 1 - x : x)];
                    float v = normalized(lv, a.mean[c], a.stdv[c]);
                    if (y >= et && y < et + eh && x >= el && x < el + ew) {
                        float nz[4];
                        noise4((uint32_t)(e >> 2), uidx, a.epoch, a.k0, a.k1, nz);
                        v = nz[e & 3];
                    }
                    o[e] = v;
                    if (o8) o8[e] = lv;
                }
            }
            __syncthreads();
        }
        r += nr;
    }
}

}  // namespace vsom

extern "C" {

size_t vsom_augment_ragged_scratch_bytes(int B, int C, int S) {
    if (B <= 0 || C <= 0 || S <= 0) return 0;
    return ((size_t)B * C * S * S + 255) / 256 * 256;
}

int vsom_augment_plan_ragged(const int64_t* index, const int32_t* shapes, long N, int B, int S, double scale0, double scale1,
                             double log_ratio0, double log_ratio1, int two_stage, double scale2_0, double scale2_1,
                             double log_ratio2_0, double log_ratio2_1, double flip_p, double erase_p, uint64_t seed, int epoch,
                             int32_t* params, vsom_stream_t stream) {
    VSOM_REQUIRE(index && shapes && params, VSOM_EINVAL, "augment_plan_ragged: null pointer");
    VSOM_REQUIRE(N > 0 && B > 0 && S > 0 && epoch >= 0, VSOM_EINVAL, "augment_plan_ragged: bad sizes (N=%ld B=%d S=%d epoch=%d)", N, B,
                 S, epoch);
    VSOM_REQUIRE(S <= vsom::RG_MAXS && N < (1L << 31), VSOM_EUNSUPPORTED, "augment_plan_ragged: S=%d (at most 224), N=%ld (below 2^31)",
                 S, N);
    VSOM_REQUIRE(scale0 > 0 && scale0 <= scale1 && log_ratio0 <= log_ratio1, VSOM_EINVAL,
                 "augment_plan_ragged: bad scale / ratio range");
    VSOM_REQUIRE(!two_stage || (scale2_0 > 0 && scale2_0 <= scale2_1 && log_ratio2_0 <= log_ratio2_1), VSOM_EINVAL,
                 "augment_plan_ragged: bad scale / ratio range of the second crop");
    VSOM_REQUIRE(flip_p >= 0 && flip_p <= 1 && erase_p >= 0 && erase_p <= 1, VSOM_EINVAL,
                 "augment_plan_ragged: probability outside [0, 1]");
    VSOM_REQUIRE(vsom::aligned16(params) && ((uintptr_t)shapes & 3) == 0, VSOM_EALIGN,
                 "augment_plan_ragged: params must be 16-byte aligned");
    const vsom::BoxDraw d1 = {scale0, scale1, log_ratio0, log_ratio1}, d2 = {scale2_0, scale2_1, log_ratio2_0, log_ratio2_1};
    VSOM_LAUNCH(vsom::augment_plan_ragged_kernel, dim3(vsom::cdiv(B, 256)), dim3(256), 0, stream, index, shapes, N, B, S, d1, d2,
                two_stage, flip_p, erase_p, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)epoch, params);
    return vsom::launch_status("augment_plan_ragged_kernel");
}

int vsom_augment_batch_ragged(const unsigned char* data, size_t data_bytes, const int64_t* offsets, const int32_t* shapes, long N,
                              int C, int max_h, int max_w, const int64_t* index, const int32_t* params, int B, int S, int R,
                              const float* mean, const float* std, uint64_t seed, int epoch, void* scratch, size_t scratch_bytes,
                              float* out, unsigned char* out_u8, vsom_stream_t stream) {
    VSOM_REQUIRE(data && offsets && shapes && index && mean && std && out, VSOM_EINVAL, "augment_batch_ragged: null pointer");
    VSOM_REQUIRE(N > 0 && B > 0 && S > 0 && max_h > 0 && max_w > 0 && epoch >= 0, VSOM_EINVAL,
                 "augment_batch_ragged: bad sizes (N=%ld B=%d S=%d max_h=%d max_w=%d epoch=%d)", N, B, S, max_h, max_w, epoch);
    VSOM_REQUIRE(C == 1 || C == 3, VSOM_EUNSUPPORTED, "augment_batch_ragged: %d channels (1 or 3)", C);
    VSOM_REQUIRE(data_bytes >= (size_t)C && data_bytes < ((size_t)1 << 62), VSOM_EINVAL,
                 "augment_batch_ragged: a data buffer of %zu bytes holds no image", data_bytes);
    VSOM_REQUIRE(S <= vsom::RG_MAXS && N < (1L << 31), VSOM_EUNSUPPORTED, "augment_batch_ragged: S=%d (at most 224), N=%ld (below 2^31)",
                 S, N);
    VSOM_REQUIRE(max_h <= vsom::RG_MAXDIM && max_w <= vsom::RG_MAXDIM, VSOM_EUNSUPPORTED,
                 "augment_batch_ragged: declared bounds %d x %d (at most 2048 a side)", max_h, max_w);
    const int side = max_h > max_w ? max_h : max_w;
    if (params) {
        VSOM_REQUIRE(R == S, VSOM_EINVAL, "augment_batch_ragged: training resizes to S (R=%d, S=%d)", R, S);
        VSOM_REQUIRE(side <= vsom::RG_SHRINK * S, VSOM_EUNSUPPORTED, "augment_batch_ragged: %d -> %d shrinks by more than 8", side, S);
        VSOM_REQUIRE(scratch && scratch_bytes >= (size_t)B * C * S * S, VSOM_EWORKSPACE,
                     "augment_batch_ragged: training needs vsom_augment_ragged_scratch_bytes(B, C, S) of scratch");
    } else {
        VSOM_REQUIRE(R >= S, VSOM_EINVAL, "augment_batch_ragged: a resize to R=%d holds no S=%d window", R, S);
        VSOM_REQUIRE(R <= vsom::RG_MAXR, VSOM_EUNSUPPORTED, "augment_batch_ragged: R=%d (at most 256)", R);
        VSOM_REQUIRE(side <= vsom::RG_SHRINK * R, VSOM_EUNSUPPORTED, "augment_batch_ragged: %d -> %d shrinks by more than 8", side, R);
    }
    VSOM_REQUIRE(vsom::aligned16(data) && vsom::aligned16(out) && (!params || vsom::aligned16(params)) &&
                     (!params || vsom::aligned16(scratch)) && ((uintptr_t)out_u8 & 3) == 0 && ((uintptr_t)offsets & 7) == 0 &&
                     ((uintptr_t)shapes & 3) == 0,
                 VSOM_EALIGN, "augment_batch_ragged: data, out, params and scratch must be 16-byte aligned");
    vsom::RaggedArgs a = {data, (long)data_bytes, offsets, shapes, N, C, max_h, max_w, index, params, S, R, vsom::RG_EVAL,
                          mean, std, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)epoch, (unsigned char*)scratch, out, out_u8};
    const dim3 grid(B, vsom::cdiv(S, vsom::RG_BAND));
    if (!params) {
        VSOM_LAUNCH(vsom::ragged_pass_kernel, grid, dim3(vsom::RG_THREADS), 0, stream, a);
        return vsom::launch_status("ragged_pass_kernel (evaluation)");
    }
    a.mode = vsom::RG_CROP1;
    VSOM_LAUNCH(vsom::ragged_pass_kernel, grid, dim3(vsom::RG_THREADS), 0, stream, a);
    const int rc = vsom::hip_status(hipGetLastError(), "ragged_pass_kernel (crop 1)");
    if (rc != VSOM_OK) return rc;
    a.mode = vsom::RG_CROP2;
    a.data = (const unsigned char*)scratch;
    a.data_bytes = (long)B * C * S * S;
    VSOM_LAUNCH(vsom::ragged_pass_kernel, grid, dim3(vsom::RG_THREADS), 0, stream, a);
    return vsom::launch_status("ragged_pass_kernel (crop 2)");
}

}  // extern "C"
