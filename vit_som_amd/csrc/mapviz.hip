// The pictures of the map (tools/evaluation.py:153-265): decoder output -> images and an 8-bit mosaic of the map grid
// (visualize_decoded_prototypes), and the last label that lands on each map cell (visualize_label_heatmap).
// Elementwise and reduction kernels: one pass over data the decoder has just written.
#include "common.h"

namespace vsom {

__device__ __forceinline__ unsigned char mosaic_level(float t) {
    t = fminf(fmaxf(t, 0.f), 1.f);                         // a NaN becomes 0
    return (unsigned char)floorf(fmaf(255.f, t, 0.5f));
}

// One workgroup per prototype image.  The image's decoder output is ONE contiguous span of n * pd floats (the rows behind
// its CLS row), element e = patch (hp, wp), then (py, px, c) inside the patch: pixel (hp p + py, wp p + px), channel c.
template <bool VEC>
__global__ __launch_bounds__(256) void proto_mosaic_kernel(const float* __restrict__ pred, int n, int g, int p, int C,
                                                           float* __restrict__ images, unsigned char* __restrict__ canvas,
                                                           int k0, int cols, int rows, int gap) {
    __shared__ float red[8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pd = p * p * C, S = g * p, pc = p * C;
    const int span = n * pd;
    const long k = (long)k0 + blockIdx.x;
    const float* src = pred + ((long)blockIdx.x * (n + 1) + 1) * pd;

    float lo = 0.f, scale = 1.f;
    if (canvas && C == 1) {                                // imshow(cmap='gray'): the image's own range
        float mn = INFINITY, mx = -INFINITY;
        if (VEC) {
            for (int e = tid * 4; e < span; e += 1024) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(src + e);
                mn = fminf(fminf(mn, v.x), fminf(v.y, fminf(v.z, v.w)));
                mx = fmaxf(fmaxf(mx, v.x), fmaxf(v.y, fmaxf(v.z, v.w)));
            }
        } else {
            for (int e = tid; e < span; e += 256) {
                mn = fminf(mn, src[e]);
                mx = fmaxf(mx, src[e]);
            }
        }
        mx = wave_max(mx);
        mn = -wave_max(-mn);
        if (lane == 0) { red[wave] = mn; red[4 + wave] = mx; }
        __syncthreads();
        mn = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
        mx = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
        lo = mn;
        scale = mx - mn;                                   // 0 for a constant image: every pixel 0
    }

    const int cell_r = (int)(k / cols), cell_c = (int)(k % cols);
    const long Wc = (long)cols * S + (long)(cols - 1) * gap;
    unsigned char* cell = canvas ? canvas + (((long)cell_r * (S + gap)) * Wc + (long)cell_c * (S + gap)) * 3 : nullptr;
    float* img = images ? images + k * C * S * S : nullptr;

    auto put = [&](int e, float v) {
        const int j = e / pd, r = e - j * pd;
        const int py = r / pc, r2 = r - py * pc;
        const int px = r2 / C, c = r2 - px * C;
        const int y = (j / g) * p + py, x = (j % g) * p + px;
        if (img) img[((long)c * S + y) * S + x] = v;
        if (cell) {
            unsigned char* px3 = cell + ((long)y * Wc + x) * 3;
            if (C == 1) {
                const unsigned char q = scale > 0.f ? mosaic_level((v - lo) / scale) : (unsigned char)0;
                px3[0] = q; px3[1] = q; px3[2] = q;
            } else {
                px3[c] = mosaic_level(v);
            }
        }
    };
    if (VEC) {
        for (int e = tid * 4; e < span; e += 1024) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(src + e);
            put(e, v.x); put(e + 1, v.y); put(e + 2, v.z); put(e + 3, v.w);
        }
    } else {
        for (int e = tid; e < span; e += 256) put(e, src[e]);
    }

    if (cell && gap > 0) {                                 // the white strips right of and below the cell (none at the edge)
        const int gr = cell_r < rows - 1 ? gap : 0, gc = cell_c < cols - 1 ? gap : 0;
        const int w = S + gc, total = (S + gr) * w;
        for (int i = tid; i < total; i += 256) {
            const int y = i / w, x = i - y * w;
            if (y < S && x < S) continue;
            unsigned char* px3 = cell + ((long)y * Wc + x) * 3;
            px3[0] = 255; px3[1] = 255; px3[2] = 255;
        }
    }
}

// cells[bmu[i]] = max(cells[bmu[i]], (first + i + 1) << 32 | label[i]): the sample with the highest ordinal wins, whatever
// the order the atomics land in (the reference's in-order `heatmap[divmod(bmu)] = label`, evaluation.py:256-258).
__global__ __launch_bounds__(256) void last_label_kernel(const int64_t* __restrict__ bmu, const int64_t* __restrict__ label,
                                                         long n, long first, int K, unsigned long long* __restrict__ cells,
                                                         int* __restrict__ bad) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int64_t b = bmu[i], y = label[i];
        if (b < 0 || b >= K || y < 0 || y > 0x7fffffffLL) { atomicAdd(bad, 1); continue; }
        atomicMax(cells + b, ((unsigned long long)(first + i + 1) << 32) | (unsigned long long)y);
    }
}

static inline int grid_1d(long n, int block, int cap) {
    const long b = (n + block - 1) / block;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

}  // namespace vsom

extern "C" {

int vsom_proto_mosaic(const float* pred, int chunk, int n, int p, int C, float* images, unsigned char* canvas, int k0, int K,
                      int rows, int cols, int gap, vsom_stream_t stream) {
    VSOM_REQUIRE(pred && (images || canvas), VSOM_EINVAL, "proto_mosaic: null pointer");
    VSOM_REQUIRE(chunk > 0 && n > 0 && p > 0 && K > 0 && k0 >= 0 && (long)k0 + chunk <= K, VSOM_EINVAL,
                 "proto_mosaic: bad sizes (chunk=%d n=%d p=%d k0=%d K=%d)", chunk, n, p, k0, K);
    VSOM_REQUIRE(C == 1 || C == 3, VSOM_EUNSUPPORTED, "proto_mosaic: %d channels (1 or 3 are drawn)", C);
    int g = 0;
    while ((long)g * g < n) ++g;
    VSOM_REQUIRE((long)g * g == n, VSOM_EINVAL, "proto_mosaic: n=%d patches do not form a square", n);
    VSOM_REQUIRE(rows > 0 && cols > 0 && (long)rows * cols == K, VSOM_EINVAL, "proto_mosaic: map %d x %d does not hold K=%d cells",
                 rows, cols, K);
    VSOM_REQUIRE(gap >= 0, VSOM_EINVAL, "proto_mosaic: negative gap");
    const long S = (long)g * p, span = (long)n * p * p * C;
    VSOM_REQUIRE(span < (1L << 30) && (cols * S + (long)(cols - 1) * gap) * 3 < (1L << 31), VSOM_EUNSUPPORTED,
                 "proto_mosaic: image or canvas row too large");
    const bool vec = (p * p * C) % 4 == 0 && vsom::aligned16(pred);
    if (vec) {
        VSOM_LAUNCH(vsom::proto_mosaic_kernel<true>, dim3(chunk), dim3(256), 0, stream, pred, n, g, p, C, images, canvas, k0, cols,
                    rows, gap);
    } else {
        VSOM_LAUNCH(vsom::proto_mosaic_kernel<false>, dim3(chunk), dim3(256), 0, stream, pred, n, g, p, C, images, canvas, k0, cols,
                    rows, gap);
    }
    return vsom::launch_status("proto_mosaic_kernel");
}

int vsom_last_label(const int64_t* bmu, const int64_t* label, long n, long first_ordinal, int K, unsigned long long* cells,
                    int* out_of_range, vsom_stream_t stream) {
    VSOM_REQUIRE(bmu && label && cells && out_of_range, VSOM_EINVAL, "last_label: null pointer");
    VSOM_REQUIRE(n >= 0 && K > 0 && first_ordinal >= 0, VSOM_EINVAL, "last_label: bad sizes");
    VSOM_REQUIRE(first_ordinal + n < (1L << 31), VSOM_EUNSUPPORTED, "last_label: sample ordinals must stay below 2^31");
    if (n == 0) return VSOM_OK;
    VSOM_LAUNCH(vsom::last_label_kernel, dim3(vsom::grid_1d(n, 256, 2048)), dim3(256), 0, stream, bmu, label, n, first_ordinal, K,
                cells, out_of_range);
    return vsom::launch_status("last_label_kernel");
}

}  // extern "C"
