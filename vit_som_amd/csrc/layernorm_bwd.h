// LayerNorm backward, per-row body of the 16-lanes-per-row layout (16 lanes per row, NCH float4 chunks per lane: chunk j
// of lane `sub` = columns 4 (sub + 16 j) ..): shared by layernorm_bwd_v4_kernel (layernorm.hip) and the LayerNorm-backward
// epilogue of the input-gradient GEMM (gemm_x6.h, EPI_LN_BWD), so that both write the same dX bits.
#pragma once
#include "common.h"

namespace vsom {

__device__ __forceinline__ float group16_sum(float v) {
    v += __shfl_xor(v, 8, 64); v += __shfl_xor(v, 4, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 1, 64);
    return v;
}

// o = rstd * (g - mean(g) - xhat * mean(g * xhat)), g = dY * gamma, xhat = (x - mean) * rstd; dg += dY * xhat, db += dY.
// Masked chunks come in as d = 0, xv = mu (xhat = 0, g = 0).  Contraction is off and every fused multiply-add is spelled out
// (the ones hipcc formed in the original kernel body), so that the bits do not depend on the kernel this is inlined into.
template <int NCH>
__device__ __forceinline__ void ln_bwd_row(const f32x4 (&d)[NCH], const f32x4 (&xv)[NCH], float mu, float rs,
                                           const f32x4 (&gam)[NCH], float inv_n, f32x4 (&o)[NCH], f32x4 (&dg)[NCH],
                                           f32x4 (&db)[NCH]) {
#pragma clang fp contract(off)
    f32x4 xh[NCH], g[NCH];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            xh[j][e] = (xv[j][e] - mu) * rs;
            g[j][e] = d[j][e] * gam[j][e];
            s1 += g[j][e];
            s2 = fmaf(g[j][e], xh[j][e], s2);
            dg[j][e] = fmaf(d[j][e], xh[j][e], dg[j][e]);
            db[j][e] += d[j][e];
        }
    }
    s1 = group16_sum(s1) * inv_n;
    s2 = group16_sum(s2) * inv_n;
#pragma unroll
    for (int j = 0; j < NCH; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) o[j][e] = rs * fmaf(-xh[j][e], s2, g[j][e] - s1);
}

// o += the residual gradient, rounded on its own (never contracted into the product above)
__device__ __forceinline__ void ln_bwd_add_resid(f32x4& o, const f32x4& rr) {
#pragma clang fp contract(off)
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] += rr[e];
}

}  // namespace vsom
