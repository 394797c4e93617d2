// Rows against parameter rows: the hot loop of kmeans_assign_kernel (kmeans.hip: rows against centres) and of
// gmm_estep_kernel (gmm.hip: rows against means and precisions).
//
// A workgroup of THREADS threads takes THREADS / 64 * RB rows at a time: wave w owns RB of them, lane l the VEC-wide column
// pieces l*VEC + 64*VEC*m.  The parameters are staged through LDS in tiles [plane][KC][dt], so each value read from LDS
// feeds RB rows, and every (row, parameter row) pair has one accumulator in registers.  What a piece contributes, and in
// which type it is summed, is the caller's Term:
//
//   struct Term {
//       static constexpr int PLANES;                        // parameter arrays [K][D] (centres: 1; means, precisions: 2)
//       typedef ... Acc;                                    // accumulator type
//       static Acc term(T x, const T (&prm)[PLANES]);       // one piece, T = Vec<VEC>::T, for VEC = 4 and VEC = 1
//   };
//
// A lane adds its pieces in column order; the sum over the 64 lanes, and whatever follows it, is the caller's.
#pragma once
#include "common.h"

namespace vsom {

template <int VEC>
struct Vec;
template <>
struct Vec<4> {
    typedef f32x4 T;
    static __device__ __forceinline__ T load(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
    static __device__ __forceinline__ T load_nt(const float* p) { return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p)); }
    static __device__ __forceinline__ void store(float* p, T v) { *reinterpret_cast<f32x4*>(p) = v; }
    static __device__ __forceinline__ T zero() { return f32x4{0.f, 0.f, 0.f, 0.f}; }
};
template <>
struct Vec<1> {
    typedef float T;
    static __device__ __forceinline__ T load(const float* p) { return *p; }
    static __device__ __forceinline__ T load_nt(const float* p) { return __builtin_nontemporal_load(p); }
    static __device__ __forceinline__ void store(float* p, T v) { *p = v; }
    static __device__ __forceinline__ T zero() { return 0.f; }
};

// tile width: the largest multiple of 64*VEC with planes*KC*dt floats in lds_bytes, not wider than D needs
inline int row_tile_width(int lds_bytes, int planes, int KC, int VEC, int D) {
    const int unit = 64 * VEC;
    const int dt = (lds_bytes / (planes * KC * 4)) / unit * unit;
    const int need = cdiv(D, unit) * unit;
    return dt < need ? dt : need;
}

// acc[r][j] += sum over the lane's pieces of Term::term(row rw + r, parameter row j0 + j), for all D columns in tiles of
// dt.  stage: fill the LDS tiles first (parameter rows past kc and columns past the tile's end as zeros); a caller whose
// parameters all fit one tile stages them on its first call only.  Rows from r1 on are read as zeros.  The caller zeroes
// acc: zeroed here, the accumulators do not stay in the registers the caller's reduction reads them from.
template <int THREADS, int RB, int KC, int VEC, class Term>
__device__ __forceinline__ void row_tile_pass(const float* X, long ldx, long rw, long r1, int D,
                                              const float* const (&prm)[Term::PLANES], int j0, int kc, float* lds, int dt,
                                              bool stage, typename Term::Acc (&acc)[RB][KC]) {
    typedef Vec<VEC> V;
    typedef typename V::T vT;
    constexpr int PLANES = Term::PLANES;
    const int tid = threadIdx.x, lane = tid & 63;
    const int ntiles = (D + dt - 1) / dt;
    for (int t = 0; t < ntiles; ++t) {
        const int d0 = t * dt, dn = min(dt, D - d0);
        if (stage) {
            __syncthreads();
            for (int e = tid * VEC; e < KC * dt; e += THREADS * VEC) {
                const int j = e / dt, d = e - j * dt;
                vT v[PLANES];
#pragma unroll
                for (int q = 0; q < PLANES; ++q) v[q] = V::zero();
                if (j < kc && d < dn) {
#pragma unroll
                    for (int q = 0; q < PLANES; ++q) v[q] = V::load(prm[q] + (size_t)(j0 + j) * D + d0 + d);
                }
#pragma unroll
                for (int q = 0; q < PLANES; ++q) V::store(lds + (size_t)q * KC * dt + e, v[q]);
            }
            __syncthreads();
        }
        for (int d = lane * VEC; d < dn; d += 64 * VEC) {
            vT xv[RB];
#pragma unroll
            for (int r = 0; r < RB; ++r) xv[r] = (rw + r < r1) ? V::load(X + (rw + r) * ldx + d0 + d) : V::zero();
#pragma unroll
            for (int j = 0; j < KC; ++j) {
                vT pv[PLANES];
#pragma unroll
                for (int q = 0; q < PLANES; ++q) pv[q] = V::load(lds + (size_t)q * KC * dt + j * dt + d);
#pragma unroll
                for (int r = 0; r < RB; ++r) acc[r][j] += Term::term(xv[r], pv);
            }
        }
    }
}

// Launch KERNEL(p) with lds bytes of dynamic LDS; the first launch of each KERNEL raises its limit to max_lds.
template <class P, void (*KERNEL)(P)>
int row_tile_launch(const P& p, int grid, int threads, size_t lds, int max_lds, const char* name, hipStream_t stream) {
    static const int attr_rc = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL),
                                                        hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
    VSOM_REQUIRE(attr_rc == 0, VSOM_EUNSUPPORTED, "%s: cannot reserve %d bytes of LDS", name, max_lds);
    launch_or_record([=]() { hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(threads), lds, stream, p); }, name);
    return launch_status(name);
}

}  // namespace vsom
