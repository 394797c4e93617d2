// Single-query multi-head attention: one query row per (image, head) against all N keys of that image -- the CLS row of
// a classifier's last encoder block, the only row forward_features reads.  fp32 FMAs throughout.
//
//   q  [B, E]          E = H hd, head h in columns [h hd, (h+1) hd)
//   kv [B N, 2E]       K in columns [0, E), V in [E, 2E) (the qkv Linear's K/V row slice, same head interleave)
//   fwd: s_j = hd^-0.5 q.k_j, o = softmax(s) V, lse = log sum_j exp(s_j)
//   bwd: p_j = exp(s_j - lse), D = do.o, ds_j = p_j (do.v_j - D)
//        dq = hd^-0.5 sum_j ds_j k_j, dk_j = hd^-0.5 ds_j q, dv_j = p_j do
//
// One workgroup of 256 threads per (image, head).  A key is handled by hd/4 consecutive lanes (four channels each, one
// float4 load of K and one of V), so a wave covers 256/hd keys per pass and the workgroup 1024/hd.  The dot products
// are reduced across those lanes by xor shuffles (every lane ends with the same bits).  The forward keeps an online
// softmax (running max, sum, output) per key group in registers: one pass over K and V, any N.  The groups meet in
// LDS and are combined in group order.  The backward writes each key's dK / dV row slice from the group that owns
// the key (rank-1 updates: no atomics), and dq from per-group partials combined in group order.  Bitwise reproducible.
// The kernel is bound by reading K and V once (twice the bytes in the backward: it also writes dK / dV).
#include "common.h"

#pragma clang fp contract(off)

namespace vsom {
namespace {

constexpr int Q1_THREADS = 256;

template <int HD>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = 1; o < HD / 4; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float dot4(const float4& a, const float4& b) {
    return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)));
}

template <int HD>
__global__ __launch_bounds__(Q1_THREADS) void attention_q1_fwd_kernel(const float* __restrict__ q, const float* __restrict__ kv,
                                                                      float* __restrict__ o, float* __restrict__ lse, int N,
                                                                      int H, float scale) {
    constexpr int LPK = HD / 4;                      // lanes per key
    constexpr int G = Q1_THREADS / LPK;              // key groups per workgroup
    __shared__ float s_m[G], s_l[G];
    __shared__ float s_o[G * HD];
    const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
    const int E = H * HD;
    const int lane = threadIdx.x % LPK, grp = threadIdx.x / LPK;
    const float4 qv = *reinterpret_cast<const float4*>(q + (long)b * E + h * HD + lane * 4);
    const float* kbase = kv + (long)b * N * (2 * E) + h * HD + lane * 4;
    float m = -INFINITY, l = 0.f;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = grp; j < N; j += G) {
        const float* row = kbase + (long)j * (2 * E);
        const float4 kk = *reinterpret_cast<const float4*>(row);
        const float4 vv = *reinterpret_cast<const float4*>(row + E);
        const float s = group_sum<HD>(dot4(qv, kk)) * scale;
        const float mn = fmaxf(m, s);
        const float corr = expf(m - mn), p = expf(s - mn);
        l = fmaf(l, corr, p);
        acc.x = fmaf(acc.x, corr, p * vv.x);
        acc.y = fmaf(acc.y, corr, p * vv.y);
        acc.z = fmaf(acc.z, corr, p * vv.z);
        acc.w = fmaf(acc.w, corr, p * vv.w);
        m = mn;
    }
    if (lane == 0) {
        s_m[grp] = m;
        s_l[grp] = l;
    }
    *reinterpret_cast<float4*>(&s_o[grp * HD + lane * 4]) = acc;
    __syncthreads();
    if (threadIdx.x < HD) {
        const int d = threadIdx.x;
        float M = -INFINITY;
        for (int g = 0; g < G; ++g) M = fmaxf(M, s_m[g]);
        float L = 0.f, O = 0.f;
        for (int g = 0; g < G; ++g) {
            const float w = expf(s_m[g] - M);        // groups that saw no key: m = -inf, w = 0
            L = fmaf(s_l[g], w, L);
            O = fmaf(s_o[g * HD + d], w, O);
        }
        o[(long)b * E + h * HD + d] = O / L;
        if (d == 0) lse[bh] = M + logf(L);
    }
}

template <int HD>
__global__ __launch_bounds__(Q1_THREADS) void attention_q1_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ o,
                                                                      const float* __restrict__ lse, const float* __restrict__ q,
                                                                      const float* __restrict__ kv, float* __restrict__ dq,
                                                                      float* __restrict__ dkv, int N, int H, float scale) {
    constexpr int LPK = HD / 4;
    constexpr int G = Q1_THREADS / LPK;
    __shared__ float s_dq[G * HD];
    const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
    const int E = H * HD;
    const int lane = threadIdx.x % LPK, grp = threadIdx.x / LPK;
    const long qoff = (long)b * E + h * HD + lane * 4;
    const float4 qv = *reinterpret_cast<const float4*>(q + qoff);
    const float4 dov = *reinterpret_cast<const float4*>(dout + qoff);
    const float4 ov = *reinterpret_cast<const float4*>(o + qoff);
    const float D = group_sum<HD>(dot4(dov, ov));
    const float L = lse[bh];
    const long rbase = (long)b * N * (2 * E) + h * HD + lane * 4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = grp; j < N; j += G) {
        const long r = rbase + (long)j * (2 * E);
        const float4 kk = *reinterpret_cast<const float4*>(kv + r);
        const float4 vv = *reinterpret_cast<const float4*>(kv + r + E);
        const float s = group_sum<HD>(dot4(qv, kk)) * scale;
        const float dp = group_sum<HD>(dot4(dov, vv));
        const float p = expf(s - L);
        const float ds = p * (dp - D);
        const float dss = ds * scale;
        acc.x = fmaf(ds, kk.x, acc.x);
        acc.y = fmaf(ds, kk.y, acc.y);
        acc.z = fmaf(ds, kk.z, acc.z);
        acc.w = fmaf(ds, kk.w, acc.w);
        *reinterpret_cast<float4*>(dkv + r) = make_float4(dss * qv.x, dss * qv.y, dss * qv.z, dss * qv.w);
        *reinterpret_cast<float4*>(dkv + r + E) = make_float4(p * dov.x, p * dov.y, p * dov.z, p * dov.w);
    }
    *reinterpret_cast<float4*>(&s_dq[grp * HD + lane * 4]) = acc;
    __syncthreads();
    if (threadIdx.x < HD) {
        const int d = threadIdx.x;
        float a = 0.f;
        for (int g = 0; g < G; ++g) a += s_dq[g * HD + d];
        dq[(long)b * E + h * HD + d] = a * scale;
    }
}

// dst[r, :cols] += src[r, :cols] (row strides in floats)
__global__ __launch_bounds__(256) void rows_add_kernel(const float* __restrict__ src, long lds, float* __restrict__ dst, long ldd,
                                                       int rows, int cols) {
    const long n = (long)rows * cols;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long r = i / cols, c = i - r * cols;
        dst[r * ldd + c] += src[r * lds + c];
    }
}

int q1_check(int B, int N, int H, int hd, const char* what) {
    VSOM_REQUIRE(B > 0 && N > 0 && H > 0, VSOM_EINVAL, "%s: non-positive shape (B=%d N=%d H=%d)", what, B, N, H);
    VSOM_REQUIRE(hd == 8 || hd == 16 || hd == 32 || hd == 64, VSOM_EINVAL, "%s: head size %d not in {8, 16, 32, 64}", what, hd);
    VSOM_REQUIRE((long)B * H <= 0x7fffffffL && (long)B * N * 2 * H * hd < (1L << 40), VSOM_EINVAL, "%s: shape too large", what);
    return VSOM_OK;
}

}  // namespace
}  // namespace vsom

using namespace vsom;

extern "C" {

int vsom_attention_q1_fwd(const float* q, const float* kv, float* o, float* lse, int B, int N, int H, int hd,
                          vsom_stream_t stream) {
    VSOM_REQUIRE(q && kv && o && lse, VSOM_EINVAL, "attention_q1_fwd: null pointer");
    int st = q1_check(B, N, H, hd, "attention_q1_fwd");
    if (st != VSOM_OK) return st;
    VSOM_REQUIRE(aligned16(q) && aligned16(kv) && aligned16(o), VSOM_EALIGN, "attention_q1_fwd: q / kv / o not 16-byte aligned");
    const float scale = 1.0f / sqrtf((float)hd);
    const dim3 grid(B * H), block(Q1_THREADS);
    switch (hd) {
        case 8: VSOM_LAUNCH(attention_q1_fwd_kernel<8>, grid, block, 0, stream, q, kv, o, lse, N, H, scale); break;
        case 16: VSOM_LAUNCH(attention_q1_fwd_kernel<16>, grid, block, 0, stream, q, kv, o, lse, N, H, scale); break;
        case 32: VSOM_LAUNCH(attention_q1_fwd_kernel<32>, grid, block, 0, stream, q, kv, o, lse, N, H, scale); break;
        default: VSOM_LAUNCH(attention_q1_fwd_kernel<64>, grid, block, 0, stream, q, kv, o, lse, N, H, scale); break;
    }
    return launch_status("attention_q1_fwd_kernel");
}

int vsom_attention_q1_bwd(const float* dout, const float* o, const float* lse, const float* q, const float* kv, float* dq,
                          float* dkv, int B, int N, int H, int hd, vsom_stream_t stream) {
    VSOM_REQUIRE(dout && o && lse && q && kv && dq && dkv, VSOM_EINVAL, "attention_q1_bwd: null pointer");
    int st = q1_check(B, N, H, hd, "attention_q1_bwd");
    if (st != VSOM_OK) return st;
    VSOM_REQUIRE(aligned16(dout) && aligned16(o) && aligned16(q) && aligned16(kv) && aligned16(dkv), VSOM_EALIGN,
                 "attention_q1_bwd: dout / o / q / kv / dkv not 16-byte aligned");
    const float scale = 1.0f / sqrtf((float)hd);
    const dim3 grid(B * H), block(Q1_THREADS);
    switch (hd) {
        case 8: VSOM_LAUNCH(attention_q1_bwd_kernel<8>, grid, block, 0, stream, dout, o, lse, q, kv, dq, dkv, N, H, scale); break;
        case 16: VSOM_LAUNCH(attention_q1_bwd_kernel<16>, grid, block, 0, stream, dout, o, lse, q, kv, dq, dkv, N, H, scale); break;
        case 32: VSOM_LAUNCH(attention_q1_bwd_kernel<32>, grid, block, 0, stream, dout, o, lse, q, kv, dq, dkv, N, H, scale); break;
        default: VSOM_LAUNCH(attention_q1_bwd_kernel<64>, grid, block, 0, stream, dout, o, lse, q, kv, dq, dkv, N, H, scale); break;
    }
    return launch_status("attention_q1_bwd_kernel");
}

int vsom_rows_add(const float* src, long lds, float* dst, long ldd, int rows, int cols, vsom_stream_t stream) {
    VSOM_REQUIRE(src && dst && rows > 0 && cols > 0 && lds >= cols && ldd >= cols, VSOM_EINVAL, "rows_add: bad arguments");
    const long n = (long)rows * cols;
    const int grid = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
    VSOM_LAUNCH(rows_add_kernel, dim3(grid), dim3(256), 0, stream, src, lds, dst, ldd, rows, cols);
    return launch_status("rows_add_kernel");
}

}  // extern "C"
