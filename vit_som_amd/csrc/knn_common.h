// What the exact k-nearest-neighbour kernels share: vsom_umap_knn (umap.hip: a set among itself) and vsom_knn_query
// (knn.hip: queries in a bank, streamed).  This header IS the contract both keep:
//   - the 128 x 64 tile of dot products on the f32 matrix cores, every (row, row) pair summed over D in one fixed order
//     that depends neither on where the two rows fall in a tile nor on the sizes of the two sets;
//   - the squared norms summed in that same order, so identical rows are at distance exactly 0;
//   - the distance from (dot, norm, norm);
//   - the strict (distance, index) total order of the lists and the order-independent insertion.
#pragma once
#include "gemm_f32.h"

namespace vsom {
namespace {

constexpr int KNN_BM = 128;                  // rows per workgroup (4 waves x 32)
constexpr int KNN_BN = 64;                   // columns per tile (two 32 x 32 accumulators per wave)
constexpr int KNN_THREADS = 256;
constexpr int KNN_MAX_K = 64;                // one list entry per lane
constexpr int KNN_TARGET_BLOCKS = 2048;      // workgroups wanted per launch (8 per CU): the column chunking stops there
constexpr int KNN_MERGE_ROWS = 4;            // rows per merge workgroup (one wave each)

inline size_t align256(size_t b) { return (b + 255) & ~size_t(255); }

// Squared row norms in the order in which the MFMA loop of knn_tile_dots sums a row's products with itself:
// in groups of 8, k = kb + s then kb + 4 + s for s = 0..3 (lane half h feeds k = kb + 4h + s to MFMA step s; the
// instruction is bitwise fma(a_k1 b_k1, fma(a_k0 b_k0, c))).  So sq[i] is <x_i, x_i> of the contraction bit for bit,
// and the euclidean distance between two identical rows is exactly 0.
__global__ __launch_bounds__(256) void knn_sqnorm_kernel(const float* __restrict__ X, long ldx, long N, int D,
                                                        float* __restrict__ sq) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float* x = X + i * ldx;
    float s = 0.f;
    for (int kb = 0; kb < D; kb += 8) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float a0 = kb + j < D ? x[kb + j] : 0.f;
            const float a1 = kb + 4 + j < D ? x[kb + 4 + j] : 0.f;
            s = fmaf(a0, a0, s);
            s = fmaf(a1, a1, s);
        }
    }
    sq[i] = s;
}

// Strict total order of the lists: (distance, index) lexicographic.  I is int (row of this launch) or int64_t (global ordinal).
template <class I>
__device__ __forceinline__ bool knn_less(float d0, I i0, float d1, I i1) { return d0 < d1 || (d0 == d1 && i0 < i1); }

// Insert the wave's candidates (lane l offers (cd, ci)) into a row's sorted list (lane j < k holds entry j), lowest
// lane first.  The result is the k smallest of list and candidates in (distance, index) order: it does not depend on
// the order of insertion, hence neither on the tiling nor on the chunking.
template <class I>
__device__ __forceinline__ void knn_insert(float& ld, I& li, float cd, I ci, int k, int lane) {
    const float kd = __shfl(ld, k - 1, 64);
    const I ki = __shfl(li, k - 1, 64);
    unsigned long long mask = __ballot(knn_less(cd, ci, kd, ki));
    while (mask) {
        const int s = __builtin_ctzll(mask);
        mask &= mask - 1;
        const float xd = __shfl(cd, s, 64);
        const I xi = __shfl(ci, s, 64);
        const int pos = __popcll(__ballot(lane < k && knn_less(ld, li, xd, xi)));
        const float ud = __shfl_up(ld, 1, 64);
        const I ui = __shfl_up(li, 1, 64);
        if (pos < k) {
            if (lane > pos) { ld = ud; li = ui; }
            else if (lane == pos) { ld = xd; li = xi; }
        }
    }
}

// Distance from the dot product and the two squared norms (umap-learn's definitions; cosine of a zero row: 0 against
// another zero row, 1 against any other row).
__device__ __forceinline__ float knn_distance(float dot, float si, float sj, int metric) {
    if (metric == VSOM_DIST_EUCLIDEAN) return sqrtf(fmaxf(si + sj - 2.f * dot, 0.f));
    if (si == 0.f && sj == 0.f) return 0.f;
    if (si == 0.f || sj == 0.f) return 1.f;
    if (dot == si && dot == sj) return 0.f;                          // identical rows
    return fmaxf(1.f - dot / (sqrtf(si) * sqrtf(sj)), 0.f);
}

// One operand of the contraction: rows [rows, D] with row stride ld.
struct KnnOperand {
    const float* base;
    long ld;
    int rows;
    unsigned bytes;     // FAST path: extent for the bounds-checked buffer loads
    int vec;            // generic path: 16-byte loads legal
};

// The operand staging of one workgroup: the row offsets of its 128 A rows are computed once, those of a 64-row B tile
// once per tile (FAST path only; the generic path indexes from the pointers).
template <bool FAST>
struct KnnStage {
    StageRegs<KNN_BM> sa;
    StageRegs<KNN_BN> sb;
    __amdgpu_buffer_rsrc_t rsA, rsB;
    OffKC<KNN_BM> oa;
    OffKC<KNN_BN> ob;
};
template <bool FAST>
__device__ __forceinline__ void knn_stage_init(KnnStage<FAST>& st, const KnnOperand& A, int bm0, const KnnOperand& B, int t) {
    if constexpr (FAST) {
        st.rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(A.base), 0, (int)A.bytes, 0x00020000);
        st.rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(B.base), 0, (int)B.bytes, 0x00020000);
        init_kc<KNN_BM>(st.oa, A.ld, bm0, A.rows, t);
    }
}

// acc[j] <- the 128 x 64 block <A[bm0 + .], B[bn0 + .]> over K on the f32 matrix cores: wave w owns rows 32w..32w+31,
// acc[j] columns 32j..32j+31 (register v of acc[j]: row (v & 3) + 8 (v >> 2) + 4h, column 32j + r).  Operand tiles are
// staged global -> registers -> LDS as in gemm_f32_kernel (lds: (128 + 64) * 36 floats).  Every pair's products are
// summed k-tile by k-tile, 8-group by 8-group, step s = 0..3 with k = kb + s before kb + 4 + s inside the instruction:
// one order for every pair.  Rows outside either operand and k >= K contribute exact zeros.  All waves must call it;
// the caller synchronises before the next call overwrites the LDS tiles.
template <bool FAST>
__device__ __forceinline__ void knn_tile_dots(KnnStage<FAST>& st, const KnnOperand& A, int bm0, const KnnOperand& B, int bn0,
                                              int K, float* lds, int t, f32x16 (&acc)[2]) {
    constexpr int BM = KNN_BM, BN = KNN_BN;
    float* As = lds;
    float* Bs = lds + BM * 36;
    const int lane = t & 63, wave = t >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wm0 = wave * 32;
    const int ktiles = (K + 31) >> 5;
    if constexpr (FAST) init_kc<BN>(st.ob, B.ld, bn0, B.rows, t);
    auto gload = [&](int kt) {
        const int k0 = kt << 5;
        if constexpr (FAST) {
            load_kc_fast<BM>(st.sa, st.rsA, st.oa, k0, K, t);
            load_kc_fast<BN>(st.sb, st.rsB, st.ob, k0, K, t);
        } else {
            load_kc<BM>(st.sa, A.base, A.ld, bm0, A.rows, k0, K, A.vec, t);
            load_kc<BN>(st.sb, B.base, B.ld, bn0, B.rows, k0, K, B.vec, t);
        }
    };
    auto lstore = [&]() {
        store_kc<BM>(st.sa, As, t);
        store_kc<BN>(st.sb, Bs, t);
    };
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[j][v] = 0.f;
    auto mfma_tile = [&]() {
#pragma unroll
        for (int kb = 0; kb < 32; kb += 8) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(As + (wm0 + r) * 36 + kb + 4 * h);
            f32x4 b[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = *reinterpret_cast<const f32x4*>(Bs + (j * 32 + r) * 36 + kb + 4 * h);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[j][s], acc[j], 0, 0, 0);
        }
    };
    gload(0);
    lstore();
    __syncthreads();
    for (int kt = 0; kt + 1 < ktiles; ++kt) {
        gload(kt + 1);
        __builtin_amdgcn_sched_barrier(0);
        mfma_tile();
        __syncthreads();
        lstore();
        __syncthreads();
    }
    mfma_tile();
}

}  // namespace
}  // namespace vsom
