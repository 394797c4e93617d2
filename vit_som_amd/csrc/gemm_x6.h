// fp32-accurate GEMM on the bf16 matrix cores: "split-bf16" (3 pieces per operand, 6 products).
//
// An fp32 value has a 24-bit significand; bf16 keeps fp32's exponent range and 8 significand
// bits.  Truncating to bf16 three times,
//     a1 = trunc16(a),  a2 = trunc16(a - a1),  a3 = a - a1 - a2
// gives a = a1 + a2 + a3 EXACTLY (8 + 8 + 8 bits; both subtractions are exact in fp32), each
// piece a bf16 number, |a2| < 2^-7 |a|, |a3| < 2^-15 |a|.  A product a*b is the 9 terms ai*bj;
// every ai*bj is exact in the MFMA's fp32 accumulator (8x8 -> 16 significand bits).  The six
// terms with i + j <= 4 are accumulated on v_mfma_f32_32x32x16_bf16, smallest first; the three
// dropped terms are below 2^-22 |a b| together, i.e. the size of the fp32 rounding an fmaf chain
// commits at every step anyway.  Measured against fp64 on the qkv GEMM of the step: relative
// error 1.3e-7 here vs 1.9e-7 for the v_mfma_f32_32x32x2_f32 engine.  The MFMA time per k drops
// from 32 to 12 cycles per 32x32 tile; range and denormal behaviour are fp32's (no scaling).
//
// Layouts, per operand: k-contiguous (both: "NT", Y = X W^T; the Linear input-gradient GEMM uses a
// transposed weight copy so that it is NT too) or k-strided (both: "TN", dW = dY^T X, reduction
// over the token rows; B only: "NN", the SOM input gradient coef W).  For a k-strided operand a
// thread loads a 4(k) x 4(cols) block, transposes it in registers and writes the same
// k-contiguous bf16 planes, so the MFMA loop is shared.
// Tiles 128 x 64 x 32 (4 waves of 32 x 64) or 64 x 64 x 32 (2 x 2 waves of 32 x 32), register-staged like
// gemm_f32.h; the split happens between the global load and the LDS store (4 and / 4 sub / 3
// perm per pair of elements).  LDS holds three bf16 planes per operand, rows of 32 bf16 (64 B) with an
// XOR chunk swizzle (x6_chunk_off: conflict-free reads AND stores).  Fragment layout of the 32x32x16
// MFMA: lane (r = l & 31, h = l >> 5) supplies A[row r][k = 8h + j] and B[k = 8h + j][col r],
// j = 0..7 -- one 16-byte LDS read per plane per 16-k step; the accumulator layout equals the
// fp32 MFMA's, so the epilogues are shared.
// One definition each, used by gemm_x6_body, gemm_x6_tn_kernel (gemm_x6_tn.h) and bmu_x3_kernel (bmu_x3.hip): the MFMA
// order (x6_products) and the k-loop with its LDS stages and sched_barriers (X6_KLOOP).
#pragma once
#include "gemm_f32.h"
#include "layernorm_bwd.h"

namespace vsom {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef unsigned v4u32 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned x6_bits(float x) { return __builtin_bit_cast(unsigned, x); }
__device__ __forceinline__ float x6_float(unsigned x) { return __builtin_bit_cast(float, x); }

// 4 floats -> 3 planes of 4 bf16 (8 bytes per plane), element e at bytes 2e..2e+1
__device__ __forceinline__ void x6_split(f32x4 v, uint2& p1, uint2& p2, uint2& p3) {
    const unsigned HI = 0xffff0000u, SEL = 0x07060302u;      // perm: high halves of (S1, S0) -> (lo, hi)
    float r[4], s[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        r[e] = v[e] - x6_float(x6_bits(v[e]) & HI);
        s[e] = r[e] - x6_float(x6_bits(r[e]) & HI);
    }
    p1.x = __builtin_amdgcn_perm(x6_bits(v[1]), x6_bits(v[0]), SEL); p1.y = __builtin_amdgcn_perm(x6_bits(v[3]), x6_bits(v[2]), SEL);
    p2.x = __builtin_amdgcn_perm(x6_bits(r[1]), x6_bits(r[0]), SEL); p2.y = __builtin_amdgcn_perm(x6_bits(r[3]), x6_bits(r[2]), SEL);
    p3.x = __builtin_amdgcn_perm(x6_bits(s[1]), x6_bits(s[0]), SEL); p3.y = __builtin_amdgcn_perm(x6_bits(s[3]), x6_bits(s[2]), SEL);
}

// 4 floats -> TWO planes of 4 bf16 (round to nearest even, v_cvt_pk_bf16_f32): a = a1 + a2 + r with |a2| <= 2^-9 |a|,
// |r| <= 2^-17 |a|.  Three products a2 b1 + a1 b2 + a1 b1 then carry |error| <= 3 * 2^-16 |a||b| per term in the worst case
// (random signs: ~2^-18 on a long sum): the BMU contraction (bmu_x3.hip) and the weight-gradient GEMM (gemm_x6_tn.h).
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
__device__ __forceinline__ void x3_split(f32x4 v, uint2& p1, uint2& p2) {
    const bf16x2_t a01 = {(__bf16)v[0], (__bf16)v[1]}, a23 = {(__bf16)v[2], (__bf16)v[3]};
    const unsigned u01 = __builtin_bit_cast(unsigned, a01), u23 = __builtin_bit_cast(unsigned, a23);
    const float r0 = v[0] - x6_float(u01 << 16), r1 = v[1] - x6_float(u01 & 0xffff0000u);
    const float r2 = v[2] - x6_float(u23 << 16), r3 = v[3] - x6_float(u23 & 0xffff0000u);
    const bf16x2_t b01 = {(__bf16)r0, (__bf16)r1}, b23 = {(__bf16)r2, (__bf16)r3};
    p1.x = u01; p1.y = u23;
    p2.x = __builtin_bit_cast(unsigned, b01); p2.y = __builtin_bit_cast(unsigned, b23);
}

// LDS plane image: [row][64 B] = 32 bf16 of one k-tile, no padding; the 16-byte chunk c (8 consecutive k) of row R sits
// at chunk position c ^ ((R >> 2) & 3).  With that XOR both access patterns are bank-conflict-free: the fragment reads
// (ds_read_b128, lane = row: its 16-lane groups hit 16 different 16-byte slots of the 256-byte bank row) AND the staging
// stores (ds_write_b64, 8 lanes per row: a 16-lane group covers two whole rows = 128 contiguous bytes).  The padded
// [row][80 B] image of round 1 was conflict-free for the reads only -- every store was 2-way (SQ_LDS_BANK_CONFLICT = a
// third of the LDS cycles of the kernel).
constexpr int X6_RS = 64;        // bytes per plane row
__device__ __forceinline__ int x6_chunk_off(int row, int chunk) { return row * X6_RS + ((chunk ^ ((row >> 2) & 3)) << 4); }
// byte offset of the 8-byte piece kq (4 consecutive k, kq = 0..7) of row `row`
__device__ __forceinline__ int x6_piece_off(int row, int kq) { return x6_chunk_off(row, kq >> 1) + ((kq & 1) << 3); }

template <int ROWS, int NPL = 3, int NT = 256>
__device__ __forceinline__ void x6_store(const StageRegs<ROWS, NT>& s, char* planes, int t) {
    constexpr int PL = ROWS * X6_RS;
#pragma unroll
    for (int p = 0; p < ROWS * 8 / NT; ++p) {
        uint2 p1, p2, p3;
        if constexpr (NPL == 3) x6_split(s.v[p], p1, p2, p3); else x3_split(s.v[p], p1, p2);
        char* dst = planes + x6_piece_off(p * (NT / 8) + (t >> 3), t & 7);
        *reinterpret_cast<uint2*>(dst) = p1;
        *reinterpret_cast<uint2*>(dst + PL) = p2;
        if constexpr (NPL == 3) *reinterpret_cast<uint2*>(dst + 2 * PL) = p3;
    }
}

// ---- k-strided ("TN") staging: a task = 4 consecutive reduction rows x 4 consecutive columns.
// Lane order inside a task group is k-group fastest (kg = t % 8, column quad = t / 8): a wave's
// load touches 8 rows x 128 contiguous bytes, and its 8-byte LDS writes are conflict-free.
struct X6Blk { f32x4 v[4]; };
__device__ __forceinline__ void x6_load_ks(X6Blk& b, __amdgpu_buffer_rsrc_t rsrc, unsigned colbytes, unsigned ld4, int k0,
                                           int K, int kg, int seg, int stride, int off0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = k0 + 4 * kg + i;
        const unsigned row = seg ? (unsigned)((k / seg) * stride + off0 + (k % seg)) : (unsigned)k;
        b.v[i] = bload4(rsrc, (k < K && colbytes != OOB) ? row * ld4 + colbytes : OOB);
    }
}
template <int NPL = 3>
__device__ __forceinline__ void x6_store_ks(const X6Blk& b, char* planes, int plane_bytes, int mq, int kg) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const f32x4 col = {b.v[0][e], b.v[1][e], b.v[2][e], b.v[3][e]};      // 4 consecutive k of column 4mq+e
        uint2 p1, p2, p3;
        if constexpr (NPL == 3) x6_split(col, p1, p2, p3); else x3_split(col, p1, p2);
        char* dst = planes + x6_piece_off(4 * mq + e, kg);
        *reinterpret_cast<uint2*>(dst) = p1;
        *reinterpret_cast<uint2*>(dst + plane_bytes) = p2;
        if constexpr (NPL == 3) *reinterpret_cast<uint2*>(dst + 2 * plane_bytes) = p3;
    }
}

// The MFMA order of the split-bf16 engine, written only here: acc += a * b over the NPL planes, smallest terms first
// (NPL = 3: the six products with i + j <= 4; NPL = 2: a2 b1 + a1 b2 + a1 b1).  The wide tile forms (gemm_x6_ln_wide_kernel,
// gemm_x6_tn_kernel<..., STAGES = 2>) are bitwise their narrow forms and bmu_x3_planes_kernel's slabs bitwise
// bmu_x3_kernel's only because every kernel sums each output element in this order.
template <int NPL>
__device__ __forceinline__ void x6_products(f32x16& acc, const bf16x8 (&a)[NPL], const bf16x8 (&b)[NPL]) {
    f32x16 c = acc;
    if constexpr (NPL == 3) {
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], c, 0, 0, 0);   // 2^-16 terms
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], c, 0, 0, 0);
    }
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], c, 0, 0, 0);       // 2^-8 (2^-9) terms
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], c, 0, 0, 0);       // leading term
    acc = c;
}

// The k-loop of the split-bf16 kernels over k-tiles [kt_begin, kt_end): gload(kt) loads k-tile kt into the staging
// registers, lstore(so) splits them into the LDS stage at byte offset so, mfma_tile(so) multiplies that stage.
// STAGES = 1: one LDS stage (so = 0), two barriers per k-tile; the next k-tile's loads are in flight under the MFMAs.
// STAGES = 2: two stages ST bytes apart, one barrier per k-tile: k-tile kt + 1 goes to the other stage while kt is
// multiplied; the stage written was last read before the previous barrier.  Past the range the last k-tile is re-read
// (never stored), so the body stays branch-free.
// The steady-state body is branch-free and the last k-tile is peeled: with a conditional prefetch inside, hipcc carries the
// accumulators through VGPRs and copies all of them AGPR -> VGPR -> AGPR on every iteration.  The sched_barriers keep the
// loads first, then the whole MFMA phase, and only then the split (left alone, hipcc interleaves load -> vmcnt(0) -> split
// into the MFMAs).
// A macro, not a function template taking the three lambdas: hipcc optimises such a function on its own before inlining
// it, and the kernels then come out rescheduled (gemm_x6_body's, the two-stage ones with other instruction counts).  As
// a macro the loop is the kernel's own code and every kernel compiles to the instructions of its former hand-written loop.
#define X6_KLOOP(STAGES, ST, kt_begin, kt_end, gload, lstore, mfma_tile)                                                    \
    do {                                                                                                                    \
        static_assert((STAGES) == 1 || (STAGES) == 2, "one or two LDS stages");                                            \
        if constexpr ((STAGES) == 1) {                                                                                      \
            if ((kt_begin) < (kt_end)) {                                                                                    \
                gload(kt_begin);                                                                                            \
                lstore(0);                                                                                                  \
            }                                                                                                               \
            __syncthreads();                                                                                                \
            for (int kt_ = (kt_begin); kt_ + 1 < (kt_end); ++kt_) {                                                         \
                gload(kt_ + 1);                                                                                             \
                __builtin_amdgcn_sched_barrier(0);                                                                          \
                mfma_tile(0);                                                                                               \
                __builtin_amdgcn_sched_barrier(0);                                                                          \
                __syncthreads();                                                                                            \
                lstore(0);                                                                                                  \
                __syncthreads();                                                                                            \
            }                                                                                                               \
            if ((kt_begin) < (kt_end)) mfma_tile(0);                                                                        \
        } else {                                                                                                            \
            if ((kt_begin) < (kt_end)) {                                                                                    \
                gload(kt_begin);                                                                                            \
                lstore(0);                                                                                                  \
                if ((kt_begin) + 1 < (kt_end)) gload((kt_begin) + 1);                                                       \
            }                                                                                                               \
            __syncthreads();                                                                                                \
            int so_ = 0;                                                                                                    \
            for (int kt_ = (kt_begin); kt_ + 1 < (kt_end); ++kt_) {                                                         \
                lstore((ST) - so_);                                                                                         \
                gload(kt_ + 2 < (kt_end) ? kt_ + 2 : kt_ + 1);                                                              \
                __builtin_amdgcn_sched_barrier(0);                                                                          \
                mfma_tile(so_);                                                                                             \
                __builtin_amdgcn_sched_barrier(0);                                                                          \
                __syncthreads();                                                                                            \
                so_ = (ST) - so_;                                                                                           \
            }                                                                                                               \
            if ((kt_begin) < (kt_end)) mfma_tile(so_);                                                                      \
        }                                                                                                                   \
    } while (0)

// ---- EPI_LN_BWD: the LayerNorm backward of whole output rows (one column tile, BN = the LayerNorm's width).  After the k-loop
// the operand LDS is dead: the accumulators pass through it 8 rows per wave row at a time (register v of a 32x32 accumulator
// holds row (v & 3) + 8 (v >> 2) + 4 h, so pass q = registers 4q..4q+3 = rows 8q..8q+7), restaged into the layout of
// layernorm_bwd_v4_kernel (16 lanes per row, float4 chunk sub + 16 j), and ln_bwd_row runs on them: dX carries the bits of
// the GEMM + layernorm_bwd pair.  The dY tile never reaches memory.  Each tile writes one dgamma / dbeta partial
// part[tile][2][N]: column sums over its rows in a fixed order (per lane in pass order, then the 16 row groups in order).
// The 192-row form runs this once per 64-row group of 256 threads (t = thread index inside the group, lds = the group's
// own LDS region, bm0 = its first row, tile = its 64-row block index); a group wholly past M writes nothing.
template <int WN, int WAVES_M, int WAVES_N, int LDS_BYTES>
__device__ __forceinline__ void x6_ln_bwd_epilogue(const GemmP& g, const f32x16 (&acc)[1][WN], char* lds, int bm0, int wm0,
                                                   int wn0, int r, int h, int tile, int t) {
    constexpr int BN = WAVES_N * WN * 32;
    constexpr int cols = BN;                 // the host launches this epilogue with N == BN only
    constexpr int NCH = (BN + 63) / 64;
    constexpr int LROW = BN + 8;             // floats per staged row: the two lane halves (rows 4 apart) 32 banks apart
    constexpr int PROWS = WAVES_M * 8;       // rows per pass
    constexpr int ITER = PROWS / 16;         // 16 row groups of 16 lanes
    static_assert(PROWS % 16 == 0 && PROWS * LROW * 4 <= LDS_BYTES && 16 * 2 * BN * 4 <= LDS_BYTES, "LN epilogue does not fit");
    float* st = reinterpret_cast<float*>(lds);
    const int sub = t & 15, rg = t >> 4;
    const float inv_n = 1.0f / (float)cols;
    // bounds-checked buffer accesses (32-bit offsets; rows past M read 0 and drop their stores -- d = 0 there)
    const unsigned rbytes = (unsigned)g.M * cols * 4u;
    const __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g.ln_x), 0, (int)rbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsR = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g.ln_resid), 0, (int)rbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsD = __builtin_amdgcn_make_buffer_rsrc(g.C, 0, (int)rbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsM = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g.ln_mean), 0, g.M * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsS = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g.ln_rstd), 0, g.M * 4, 0x00020000);
    const bool has_resid = g.ln_resid != nullptr;
    f32x4 gam[NCH], dg[NCH], db[NCH];
    bool cv[NCH];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        cv[j] = 4 * (sub + 16 * j) < cols;
        gam[j] = cv[j] ? reinterpret_cast<const f32x4*>(g.ln_gamma)[sub + 16 * j] : f32x4{0.f, 0.f, 0.f, 0.f};
        dg[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        db[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const int wr = wm0 >> 5;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        // every global load of the pass before its first store (see gemm_epilogue)
        bool ok[ITER];
        unsigned off[ITER][NCH];
        float mu[ITER], rs[ITER];
        f32x4 xv[ITER][NCH], rr[ITER][NCH];
#pragma unroll
        for (int i = 0; i < ITER; ++i) {
            const int lr = 16 * i + rg;
            const int row = bm0 + (lr >> 3) * 32 + 8 * q + (lr & 7);
            ok[i] = row < g.M;
#pragma unroll
            for (int j = 0; j < NCH; ++j)       // OOB itself, never OOB + something: that wraps round into row 0
                off[i][j] = (ok[i] && cv[j]) ? (unsigned)row * (cols * 4u) + 16u * (sub + 16 * j) : OOB;
            const unsigned roff = ok[i] ? (unsigned)row * 4u : OOB;
            mu[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsM, (int)roff, 0, 0));
            rs[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsS, (int)roff, 0, 0));
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                xv[i][j] = bload4(rsX, off[i][j]);
                rr[i][j] = has_resid ? bload4(rsR, off[i][j]) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
        __syncthreads();                      // q = 0: the last k-tile's operand reads; q > 0: the previous pass's reads
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) st[(wr * 8 + e + 4 * h) * LROW + wn0 + j * 32 + r] = acc[0][j][4 * q + e];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < ITER; ++i) {
            const int lr = 16 * i + rg;
            f32x4 d[NCH], o[NCH];
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                d[j] = (cv[j] && ok[i]) ? *reinterpret_cast<const f32x4*>(st + lr * LROW + 4 * (sub + 16 * j)) : f32x4{0.f, 0.f, 0.f, 0.f};
                if (!cv[j]) xv[i][j] = f32x4{mu[i], mu[i], mu[i], mu[i]};
            }
            ln_bwd_row<NCH>(d, xv[i], mu[i], rs[i], gam, inv_n, o, dg, db);
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                if (has_resid) ln_bwd_add_resid(o[j], rr[i][j]);
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u32, o[j]), rsD, (int)off[i][j], 0, 0);
            }
        }
    }
    __syncthreads();
    float* sh = st;                           // [16 row groups][dgamma | dbeta][cols]
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        if (!cv[j]) continue;
        reinterpret_cast<f32x4*>(sh + (rg * 2 + 0) * cols)[sub + 16 * j] = dg[j];
        reinterpret_cast<f32x4*>(sh + (rg * 2 + 1) * cols)[sub + 16 * j] = db[j];
    }
    __syncthreads();
    if (bm0 >= g.M) return;                   // no barrier below
    for (int c = t; c < 2 * cols; c += 256) {
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) s += sh[q * 2 * cols + c];
        g.ln_part[(long)tile * 2 * cols + c] = s;
    }
}

// NPL = 3: exact three-piece split, six products; NPL = 2: two-piece round-to-nearest split, three products (x3_split above).
// NT threads (WAVES_M * WAVES_N waves; k-strided operands need 256); STAGES: LDS operand stages of X6_KLOOP.  The
// per-element k order and MFMA order (x6_products) do not depend on NT, STAGES or the tile height.
template <bool A_KC, bool B_KC, int WM, int WN, int WAVES_M, int WAVES_N, int EPI, int NPL = 3, int NT = 256, int STAGES = 1>
__device__ __forceinline__ void gemm_x6_body(const GemmP& g) {
    constexpr int BM = WAVES_M * WM * 32;
    constexpr int BN = WAVES_N * WN * 32;
    constexpr int PA = BM * X6_RS, PB = BN * X6_RS;
    constexpr int ST = NPL * (PA + PB);                         // bytes of one operand stage
    static_assert(NT == WAVES_M * WAVES_N * 64 && (NT == 256 || (A_KC && B_KC)), "thread count");
    // EPI_LN_BWD: one LDS region per 64-row group of 256 threads, carved from the dead operand stages
    constexpr int RG = NT / 256;
    constexpr int LN_NEED = EPI == EPI_LN_BWD ? 16 * 2 * BN * 4 : 0;
    constexpr int LDS_BYTES = STAGES * ST > RG * LN_NEED ? STAGES * ST : RG * LN_NEED;
    __shared__ __attribute__((aligned(16))) char lds[LDS_BYTES];
    char* As = lds;
    char* Bs = lds + NPL * PA;

    const int t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wm0 = (wave / WAVES_N) * (WM * 32);
    const int wn0 = (wave % WAVES_N) * (WN * 32);

    // same (split, tile) -> workgroup order as gemm_f32_kernel
    const int tiles_n = (g.N + BN - 1) / BN;
    const int tiles_m = (g.M + BM - 1) / BM;
    const int ntiles = tiles_m * tiles_n;
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int z = lid / ntiles;
    const int rem = lid - z * ntiles;
    const int tm = g.n_major ? rem % tiles_m : rem / tiles_n;
    const int tn = g.n_major ? rem / tiles_m : rem % tiles_n;
    const int bm0 = tm * BM;
    const int bn0 = tn * BN;

    const int ktiles = (g.K + 31) >> 5;
    const int kt_begin = z * g.ktiles_per_split;
    int kt_end = kt_begin + g.ktiles_per_split;
    if (kt_end > ktiles) kt_end = ktiles;

    f32x16 acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[i][j][v] = 0.f;

    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g.A), 0, (int)g.a_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g.B), 0, (int)g.b_bytes, 0x00020000);
    // per-operand staging state: k-contiguous operands use StageRegs / OffKC (all NT threads),
    // k-strided ones the 4x4 task map (A tasks on threads [0, 2 BM), B tasks on [256 - 2 BN, 256))
    StageRegs<A_KC ? BM : 32, NT> sa;
    StageRegs<B_KC ? BN : 32, NT> sb;
    OffKC<A_KC ? BM : 32, NT> oa; OffKC<B_KC ? BN : 32, NT> ob;
    constexpr int TA = 2 * BM, TB0 = 256 - 2 * BN;
    static_assert((A_KC || TA <= 256) && (B_KC || TB0 >= 0), "tile too large for the k-strided task map");
    const bool has_a = !A_KC && t < TA, has_b = !B_KC && t >= TB0;
    const int kga = t & 7, mqa = t >> 3, kgb = (t - TB0) & 7, mqb = (t - TB0) >> 3;
    X6Blk ba, bb;
    unsigned cola = OOB, colb = OOB;
    float cs[4] = {0.f, 0.f, 0.f, 0.f};          // EPI_SLAB bias partial: column sums of A over this thread's k rows
    const bool want_colsum = (EPI == EPI_SLAB) && !A_KC && g.slab_bias != nullptr && bn0 == 0;
    if constexpr (A_KC) init_kc<BM, NT>(oa, g.lda, bm0, g.M, t);
    else if (has_a && bm0 + 4 * mqa < g.M) cola = (unsigned)(bm0 + 4 * mqa) << 2;
    if constexpr (B_KC) init_kc<BN, NT>(ob, g.ldb, bn0, g.N, t);
    else if (has_b && bn0 + 4 * mqb < g.N) colb = (unsigned)(bn0 + 4 * mqb) << 2;
    auto gload = [&](int kt) {
        if constexpr (A_KC) load_kc_fast<BM, NT>(sa, rsA, oa, kt << 5, g.K, t);
        else if (has_a) x6_load_ks(ba, rsA, cola, (unsigned)g.lda << 2, kt << 5, g.K, kga, g.a_seg, g.a_stride, g.a_off);
        if constexpr (B_KC) load_kc_fast<BN, NT>(sb, rsB, ob, kt << 5, g.K, t);
        else if (has_b) x6_load_ks(bb, rsB, colb, (unsigned)g.ldb << 2, kt << 5, g.K, kgb, 0, 0, 0);
    };
    auto lstore = [&](int so) {         // so: byte offset of the LDS stage
        if constexpr (A_KC) {
            x6_store<BM, NPL, NT>(sa, As + so, t);
        } else if (has_a) {
            if (want_colsum) {
#pragma unroll
                for (int e = 0; e < 4; ++e) cs[e] += (ba.v[0][e] + ba.v[1][e]) + (ba.v[2][e] + ba.v[3][e]);
            }
            x6_store_ks<NPL>(ba, As + so, PA, mqa, kga);
        }
        if constexpr (B_KC) x6_store<BN, NPL, NT>(sb, Bs + so, t);
        else if (has_b) x6_store_ks<NPL>(bb, Bs + so, PB, mqb, kgb);
    };

    auto mfma_tile = [&](int so) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 a[WM][NPL], b[WN][NPL];
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int pl = 0; pl < NPL; ++pl)
                    a[i][pl] = *reinterpret_cast<const bf16x8*>(As + so + pl * PA + x6_chunk_off(wm0 + i * 32 + r, 2 * ks + h));
#pragma unroll
            for (int j = 0; j < WN; ++j)
#pragma unroll
                for (int pl = 0; pl < NPL; ++pl)
                    b[j][pl] = *reinterpret_cast<const bf16x8*>(Bs + so + pl * PB + x6_chunk_off(wn0 + j * 32 + r, 2 * ks + h));
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j) x6_products<NPL>(acc[i][j], a[i], b[j]);
        }
    };
    X6_KLOOP(STAGES, ST, kt_begin, kt_end, gload, lstore, mfma_tile);
    if constexpr (EPI == EPI_SLAB && !A_KC) {
        if (want_colsum && has_a) {              // the 8 k-groups of a column quad are 8 consecutive lanes
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = cs[e];
                v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64);
                const int m = bm0 + 4 * mqa + e;
                if (kga == 0 && m < g.M) g.slab_bias[(long)z * g.slab_bias_stride + m] = v;
            }
        }
    }
    if constexpr (EPI == EPI_LN_BWD) {
        static_assert(A_KC && B_KC && WM == 1 && WAVES_M % RG == 0, "EPI_LN_BWD: NT GEMM, one accumulator row per wave");
        // row group gi = threads [256 gi, 256 gi + 256) = wave rows [gi WAVES_M / RG, (gi + 1) WAVES_M / RG)
        constexpr int GM = WAVES_M / RG * 32, RGS = (LDS_BYTES / RG) & ~15;
        const int gi = t >> 8;
        x6_ln_bwd_epilogue<WN, WAVES_M / RG, WAVES_N, RGS>(g, acc, lds + gi * RGS, bm0 + gi * GM, wm0 - gi * GM, wn0, r, h,
                                                           tm * RG + gi, t & 255);
    } else {
        gemm_epilogue<WM, WN, EPI>(g, acc, bm0 + wm0, bn0 + wn0, r, h, z);
    }
}

template <bool A_KC, bool B_KC, int WM, int WN, int WAVES_M, int WAVES_N, int EPI, int NPL = 3>
__global__ __launch_bounds__(256) void gemm_x6_kernel(const GemmP g) {
    gemm_x6_body<A_KC, B_KC, WM, WN, WAVES_M, WAVES_N, EPI, NPL>(g);
}

// The input-gradient GEMM with the LayerNorm backward in its epilogue (EPI_LN_BWD, one column tile of BN = the LayerNorm's
// width), its own kernel so that it can ask for at least two workgroups per CU: 64 x 192 takes 160 VGPRs (three per CU),
// 128 x 96 180 (two).  (128 x 192 would need more than 256: one workgroup per CU, or spills.)
template <int WN, int WAVES_M, int WAVES_N, int NPL>
__global__ __launch_bounds__(256, 2) void gemm_x6_ln_kernel(const GemmP g) {
    gemm_x6_body<true, true, 1, WN, WAVES_M, WAVES_N, EPI_LN_BWD, NPL>(g);
}

// Wide form for the encoder in the three-product mode: 192 x 192 tiles of 12 waves (three 64-row groups of 2 x 2 waves of
// 32 x 96, one workgroup per CU, two operand stages), so the transposed weight is staged and split once per 192 rows
// instead of once per 64.  Each row group runs the epilogue above on its own LDS region and writes the partial of its
// 64-row block: dX and the partials are bitwise those of gemm_x6_ln_kernel<3, 2, 2, NPL>.
template <int WN, int WAVES_M, int WAVES_N, int NPL>
__global__ __launch_bounds__(WAVES_M * WAVES_N * 64) void gemm_x6_ln_wide_kernel(const GemmP g) {
    gemm_x6_body<true, true, 1, WN, WAVES_M, WAVES_N, EPI_LN_BWD, NPL, WAVES_M * WAVES_N * 64, 2>(g);
}

}  // namespace vsom
