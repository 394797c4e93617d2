// GEMM launcher + the nn.Linear-shaped C-ABI entries built on it.
#include "gemm_f32.h"
#include "gemm_x6.h"
#include "gemm_x6_tn.h"

#include <atomic>

#include <stdarg.h>
#include <stdlib.h>

namespace vsom {

static thread_local char g_err[512] = "no error";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
const char* last_error() { return g_err; }

// Arithmetic of the nn.Linear-shaped GEMMs (include/vitsom_hip.h): VSOM_GEMM_F32, VSOM_GEMM_SPLIT_BF16 (exact three-piece
// split, six products everywhere) or VSOM_GEMM_SPLIT_BF16_GRAD3 (default: the same forward; the weight- and input-gradient
// GEMMs of the Linear layers on the two-piece split, three products).
static std::atomic<int> g_gemm_mode{VSOM_GEMM_SPLIT_BF16_GRAD3};
int gemm_mode() { return g_gemm_mode.load(std::memory_order_relaxed); }
int gemm_grad_products() { return gemm_mode() == VSOM_GEMM_SPLIT_BF16_GRAD3 ? 3 : 6; }

// One tile configuration: 128 x 64 (4 waves, each 32 x 64 = two 32x32 accumulators).  Measured
// against 128 x 128 on every GEMM shape of the step (and 4096^3): faster everywhere -- three
// workgroups per CU instead of two and half the epilogue per workgroup.
// ---- the launch plan ("Which kernel runs").
// The kernels a (layout, epilogue) pair has beside the f32 128 x 64 pair that every one has.  gemm_plan() chooses among
// them and dispatch_gemm() instantiates exactly them: a form that is false here is neither planned nor compiled.
struct GemmForms {
    bool x6;            // the split-bf16 engine at 128 x 64, three planes
    bool x6_tile64;     // ... and at 64 x 64 (three planes only)
    bool x6_planes2;    // ... and at 128 x 64 on two planes (three products), for GemmP::products == 3
    bool f32_tile64;    // the f32 engine at 64 x 64
};
static constexpr GemmForms gemm_forms(bool a_kc, bool b_kc, int epi) {
    if (a_kc && b_kc) {                                         // "NT": the slab epilogue (BMU pass) stays exact f32
        const bool x6 = epi != EPI_SLAB;
        return {x6, x6, x6 && (epi == EPI_NONE || epi == EPI_GELU_BWD), false};       // two planes: the input-gradient GEMMs
    }
    if (a_kc) return {epi == EPI_ROWAXPY, false, epi == EPI_ROWAXPY, false};          // "NN": the SOM's gX only
    return {true, true, epi == EPI_ROWAXPY, true};                                    // "TN" (both k-strided)
}
// No plan has two planes under the slab epilogue, so nothing launches this kernel.  It is instantiated to keep the library's
// kernel set (62 in this file) what the bitwise tests and the build time were measured with; retiring it is a change of its own.
template __global__ void gemm_x6_kernel<false, false, 1, 2, 4, 1, EPI_SLAB, 2>(const GemmP);

// 16-byte vector loads run along k for k-contiguous operands and along the tile's columns for k-strided ones
static bool gemm_vec_extents(bool a_kc, bool b_kc, int M, int N, int K) { return (a_kc ? K : M) % 4 == 0 && (b_kc ? K : N) % 4 == 0; }

GemmPlan gemm_plan(bool a_kc, bool b_kc, int epi, int M, int N, int K, bool fast, int mode, int products, int splits) {
    const GemmForms f = gemm_forms(a_kc, b_kc, epi);
    GemmPlan p;
    p.fast = fast;
    p.engine = (f.x6 && fast && mode != VSOM_GEMM_F32) ? GEMM_ENGINE_X6 : GEMM_ENGINE_F32;
    if (!a_kc && !b_kc) {
        // the weight-gradient layout: 64-row tiles when the output height (192 = proj / fc2 rows, 96, ...) would otherwise
        // pad 128-row tiles by >= 10 %
        const double w128 = (double)cdiv(M, 128) * 128, w64 = (double)cdiv(M, 64) * 64;
        p.tile_m = (w128 > 1.10 * w64) ? 64 : 128;
    } else {
        // 64 x 64 only for problems of at most 64 rows.  (Rounds 1-2 chose between the two with a "rounds of 256
        // workgroups" model fitted to each GEMM running ALONE, which sent about half of the step's GEMMs to 64 x 64.
        // Inside the step two kernels share the chip nearly all the time (tools/timeline.py), and there the larger tile
        // wins: every GEMM of this family on 128 x 64 is 0.3 ms per step faster, A/B on one box 11.07-11.14 ->
        // 10.77-10.83 ms; restricting 64 x 64 to launches of < 512 or < 256 large tiles: 10.91 / 10.85.)
        p.tile_m = (f.x6_tile64 && p.engine == GEMM_ENGINE_X6 && M <= 64) ? 64 : 128;
    }
    // the 64 x 64 tile has the three-plane form only, also where three products were asked for
    p.planes = p.engine == GEMM_ENGINE_F32 ? 0 : (f.x6_planes2 && products == 3 && p.tile_m == 128) ? 2 : 3;
    const int ktiles = K > 0 ? cdiv(K, 32) : 1;
    if (splits > ktiles) splits = ktiles;
    if (splits < 1) splits = 1;
    p.ktiles_per_split = cdiv(ktiles, splits);
    p.splits = cdiv(ktiles, p.ktiles_per_split);
    p.tiles = cdiv(M, p.tile_m) * cdiv(N, 64);
    p.grid = p.tiles * p.splits;
    return p;
}

// (engine, tile height, planes, fast) as one switch label
static constexpr int plan_key(int engine, int tile_m, int planes, bool fast) { return ((engine * 2 + (tile_m == 64)) * 4 + planes) * 2 + fast; }

template <bool A_KC, bool B_KC, int EPI>
static int dispatch_gemm(const GemmPlan& p, const GemmP& g, hipStream_t stream) {
    constexpr GemmForms F = gemm_forms(A_KC, B_KC, EPI);
    const dim3 grid(p.grid), block(256);
    switch (plan_key(p.engine, p.tile_m, p.planes, p.fast)) {
        case plan_key(GEMM_ENGINE_F32, 128, 0, false):
            VSOM_LAUNCH((gemm_f32_kernel<A_KC, B_KC, 1, 2, 4, 1, EPI, false>), grid, block, 0, stream, g);
            return launch_status("gemm_f32_kernel");
        case plan_key(GEMM_ENGINE_F32, 128, 0, true):
            VSOM_LAUNCH((gemm_f32_kernel<A_KC, B_KC, 1, 2, 4, 1, EPI, true>), grid, block, 0, stream, g);
            return launch_status("gemm_f32_kernel");
        case plan_key(GEMM_ENGINE_F32, 64, 0, false):
            if constexpr (F.f32_tile64) {
                VSOM_LAUNCH((gemm_f32_kernel<A_KC, B_KC, 1, 1, 2, 2, EPI, false>), grid, block, 0, stream, g);
                return launch_status("gemm_f32_kernel");
            }
            break;
        case plan_key(GEMM_ENGINE_F32, 64, 0, true):
            if constexpr (F.f32_tile64) {
                VSOM_LAUNCH((gemm_f32_kernel<A_KC, B_KC, 1, 1, 2, 2, EPI, true>), grid, block, 0, stream, g);
                return launch_status("gemm_f32_kernel");
            }
            break;
        case plan_key(GEMM_ENGINE_X6, 64, 3, true):
            if constexpr (F.x6_tile64) {
                VSOM_LAUNCH((gemm_x6_kernel<A_KC, B_KC, 1, 1, 2, 2, EPI>), grid, block, 0, stream, g);
                return launch_status("gemm_x6_kernel");
            }
            break;
        case plan_key(GEMM_ENGINE_X6, 128, 3, true):
            if constexpr (F.x6) {
                VSOM_LAUNCH((gemm_x6_kernel<A_KC, B_KC, 1, 2, 4, 1, EPI>), grid, block, 0, stream, g);
                return launch_status("gemm_x6_kernel");
            }
            break;
        case plan_key(GEMM_ENGINE_X6, 128, 2, true):
            if constexpr (F.x6_planes2) {
                VSOM_LAUNCH((gemm_x6_kernel<A_KC, B_KC, 1, 2, 4, 1, EPI, 2>), grid, block, 0, stream, g);
                return launch_status("gemm_x6_kernel");
            }
            break;
    }
    set_error("gemm: plan (engine %d, tile %d x 64, %d planes) has no kernel for layout (%d,%d) epilogue %d", p.engine, p.tile_m,
              p.planes, (int)A_KC, (int)B_KC, EPI);
    return VSOM_EUNSUPPORTED;
}

int launch_gemm(bool a_kc, bool b_kc, int epi, GemmP g, int splits, hipStream_t stream) {
    VSOM_REQUIRE(g.M > 0 && g.N > 0 && g.K > 0, VSOM_EINVAL, "gemm: non-positive shape M=%d N=%d K=%d", g.M, g.N, g.K);
    VSOM_REQUIRE(g.A && g.B, VSOM_EINVAL, "gemm: null operand");
    // 16-byte vector loads need an aligned base and row stride
    g.a_vec = aligned16(g.A) && (g.lda % 4 == 0);
    g.b_vec = aligned16(g.B) && (g.ldb % 4 == 0);
    // extent of each operand in bytes; rows of a k-strided A may be remapped (a_seg)
    const long a_rows = a_kc ? g.M : (g.a_seg ? (long)((g.K - 1) / g.a_seg) * g.a_stride + g.a_off + (g.K - 1) % g.a_seg + 1 : g.K);
    const long a_cols = a_kc ? g.K : g.M;
    const long b_rows = b_kc ? g.N : g.K, b_cols = b_kc ? g.K : g.N;
    const long ab = operand_bytes(a_rows, g.lda, a_cols), bb = operand_bytes(b_rows, g.ldb, b_cols);
    const bool fast = g.a_vec && g.b_vec && gemm_vec_extents(a_kc, b_kc, g.M, g.N, g.K) && ab < 0xFFFF0000L && bb < 0xFFFF0000L;
    g.a_bytes = (unsigned)ab; g.b_bytes = (unsigned)bb;
    g.n_major = bb > ab;        // share the larger operand's panel between neighbouring workgroups

    const GemmPlan p = gemm_plan(a_kc, b_kc, epi, g.M, g.N, g.K, fast, gemm_mode(), g.products, splits);
    g.ktiles_per_split = p.ktiles_per_split;

    if (a_kc && b_kc) {
        switch (epi) {
            case EPI_BIAS: return dispatch_gemm<true, true, EPI_BIAS>(p, g, stream);
            case EPI_BIAS_GELU: return dispatch_gemm<true, true, EPI_BIAS_GELU>(p, g, stream);
            case EPI_BIAS_RELU: return dispatch_gemm<true, true, EPI_BIAS_RELU>(p, g, stream);
            case EPI_BIAS_RES: return dispatch_gemm<true, true, EPI_BIAS_RES>(p, g, stream);
            case EPI_SLAB: return dispatch_gemm<true, true, EPI_SLAB>(p, g, stream);
            case EPI_NONE: return dispatch_gemm<true, true, EPI_NONE>(p, g, stream);
            case EPI_GELU_BWD: return dispatch_gemm<true, true, EPI_GELU_BWD>(p, g, stream);
        }
    } else if (a_kc && !b_kc) {
        switch (epi) {
            case EPI_NONE: return dispatch_gemm<true, false, EPI_NONE>(p, g, stream);
            case EPI_GELU_BWD: return dispatch_gemm<true, false, EPI_GELU_BWD>(p, g, stream);
            case EPI_ROWAXPY: return dispatch_gemm<true, false, EPI_ROWAXPY>(p, g, stream);
        }
    } else if (!a_kc && !b_kc) {
        switch (epi) {
            case EPI_SLAB: return dispatch_gemm<false, false, EPI_SLAB>(p, g, stream);
            case EPI_ROWAXPY: return dispatch_gemm<false, false, EPI_ROWAXPY>(p, g, stream);
        }
    }
    set_error("gemm: layout/epilogue combination (%d,%d,%d) not instantiated", (int)a_kc, (int)b_kc, epi);
    return VSOM_EUNSUPPORTED;
}

// ------------------------------------------------------------------ slab reduction
// (the reducer's body lives in gemm_f32.h: the LayerNorm backward batches many of these reductions into one launch)
template <int WAVES, int VEC>
__global__ __launch_bounds__(WAVES * 64) void reduce_slabs_kernel(const float* __restrict__ slabs, long stride,
                                                                  int nslabs, float* __restrict__ out1, long n1,
                                                                  float* __restrict__ out2, long off2, long n2,
                                                                  int nb1, int vec) {
    __shared__ __attribute__((aligned(16))) f32x4 sh[WAVES][64];
    reduce_slabs_body<WAVES, VEC>(sh, (int)blockIdx.x, slabs, stride, nslabs, out1, n1, out2, off2, n2, nb1, vec);
}

int reduce_slabs2_internal(const float* slabs, long stride, int nslabs, float* out1, long n1, float* out2, long off2,
                           long n2, hipStream_t stream) {
    if (n1 <= 0 && n2 <= 0) return VSOM_OK;
    if (!out2) n2 = 0;
    const int vec = aligned16(slabs) && (stride % 4 == 0) && (off2 % 4 == 0);
    if (n1 + n2 <= 4096 && nslabs >= 32) {
        const int nb1 = cdiv(n1, 64), nb2 = n2 > 0 ? cdiv(n2, 64) : 0;
        VSOM_LAUNCH((reduce_slabs_kernel<16, 1>), dim3(nb1 + nb2), dim3(1024), 0, stream, slabs, stride, nslabs, out1,
                           n1, out2, off2, n2, nb1, vec);
    } else {
        const int nb1 = cdiv(n1, 256), nb2 = n2 > 0 ? cdiv(n2, 256) : 0;
        VSOM_LAUNCH((reduce_slabs_kernel<4, 4>), dim3(nb1 + nb2), dim3(256), 0, stream, slabs, stride, nslabs, out1, n1,
                           out2, off2, n2, nb1, vec);
    }
    return launch_status("reduce_slabs_kernel");
}

int reduce_slabs_internal(const float* slabs, long stride, int nslabs, float* out, long n, hipStream_t stream) {
    return reduce_slabs2_internal(slabs, stride, nslabs, out, n, nullptr, 0, 0, stream);
}

// Split count for a reduction-split GEMM (weight gradients over the token rows, the BMU pass over
// L).  Workgroups are resident 3 per CU (register budget of the 128x64 tile), so a launch runs in
// ceil(tiles*s / slots) rounds of ceil(ktiles/s) k-tiles each; pick the s that minimises
// rounds x (k-tiles per workgroup + fixed per-workgroup cost) + the slab-reduction cost.
static int device_cus() {
    static int cus = 0;
    if (!cus) {
        int dev = 0, n = 256;
        if (hipGetDevice(&dev) == hipSuccess) {
            hipDeviceProp_t p;
            if (hipGetDeviceProperties(&p, dev) == hipSuccess && p.multiProcessorCount > 0) n = p.multiProcessorCount;
        }
        cus = n;
    }
    return cus;
}
int choose_splits(int tiles, int ktiles, int max_splits, bool prefer_xcd_multiple) {
    const int slots = 3 * device_cus();
    if (max_splits > ktiles) max_splits = ktiles;
    if (max_splits < 1) max_splits = 1;
    // measured relative MFMA efficiency with 1 / 2 / 3 co-resident workgroups per CU
    static const double eff[4] = {1.0, 0.64, 0.80, 1.0};
    const int per_cu = slots / 3;
    double best = 1e30;
    int best_s = 1;
    for (int s = 1; s <= max_splits; ++s) {
        const int per = cdiv(ktiles, s);
        if (cdiv(ktiles, per) != s) continue;            // only canonical split counts
        const long blocks = (long)tiles * s;
        const long full = blocks / slots;                // rounds with every slot taken
        const long rest = blocks - full * slots;
        const int share = (int)((rest + per_cu - 1) / per_cu);          // 0..3 workgroups per CU in the last round
        const double passes = 3.0 * full + (share ? share / eff[share] : 0.0);
        double cost = passes * (per + 3.5) + 0.003 * tiles * s;         // + slab reduction
        if (prefer_xcd_multiple && s % 8 == 0) cost *= 0.93;             // one reduction slice per XCD: operands fetched once
        if (cost < best) { best = cost; best_s = s; }
    }
    return best_s;
}
// Weight-gradient plan ("Which kernel runs"): the tile of gemm_x6_tn_kernel, or TN_GENERIC where none fits (the
// generic k-strided GEMM of launch_gemm), and the number of reduction splits -- a function of the shape and the switches
// only, so that the workspace query and the launch agree.
enum TnTile : int { TN_GENERIC = 0, TN_192x64 = 1, TN_96x96 = 2, TN_192x192 = 3 };
struct TnPlan {
    int tile;                   // TnTile
    int rows, cols, threads;    // of one workgroup's tile (rows of dW = N, columns = K); 0 for TN_GENERIC
    int splits;
};
// test / measurement hook (vsom_set_wgrad_tiles): 0 = the 192 x 64 tiles only, 1 = 192 x 192 tiles at the split count
// of the 192 x 64 plan (bitwise the same dW and db), 2 = 192 x 192 tiles with their own split count (default)
static std::atomic<int> g_wgrad_tiles{2};
static int splits_for(int tiles, int ktiles, int target) {
    int s = (target + tiles / 2) / tiles;
    if (s > ktiles) s = ktiles;
    if (s < 1) s = 1;
    return cdiv(ktiles, cdiv(ktiles, s));
}
static TnPlan bwd_weight_plan(int M, int N, int K, int mode, int wide) {
    const int ktiles = cdiv(M, 32);
    if (N % 192 == 0 && K % 192 == 0 && wide && mode == VSOM_GEMM_SPLIT_BF16_GRAD3) {
        // 192 x 192: one 112 KB workgroup per CU.  Workgroups for three quarters of the CUs: inside the step the rest serve
        // the backward chain (round 5, in-step A/B on one box: 256 / 192 / 160 / 128 workgroups -> -0.22 / -0.31 / -0.25 /
        // -0.13 ms per step against the 192 x 64 plan; alone 256 is fastest).  Hook 1 keeps the 192 x 64 plan's splits.
        const int splits = wide == 2 ? splits_for((N / 192) * (K / 192), ktiles, 3 * device_cus() / 4)
                                     : splits_for((N / 192) * (K / 64), ktiles, 384);
        return {TN_192x192, 192, 192, 768, splits};
    }
    // 384 workgroups.  Alone the kernel is fastest with two resident workgroups per CU (512), but inside the step, where it
    // shares the chip with the backward chain, fewer and longer reduction ranges win -- and more so since the gradient GEMMs
    // run three products (round 3, lab builds A/B on one box: 768 / 512 / 384 / 320 / 256 / 192 workgroups ->
    // +0.17 / 0 / -0.08...-0.10 / 0 / +0.15 / +0.45 ms per step; rounding the count to a multiple of 8: no difference)
    if (N % 192 == 0 && K % 64 == 0) return {TN_192x64, 192, 64, 256, splits_for((N / 192) * (K / 64), ktiles, 384)};
    if (N % 96 == 0 && K % 96 == 0) return {TN_96x96, 96, 96, 192, splits_for((N / 96) * (K / 96), ktiles, 384)};
    const int tiles = gemm_plan(false, false, EPI_SLAB, N, K, M, true, mode, 0, 1).tiles;
    return {TN_GENERIC, 0, 0, 0, choose_splits(tiles, ktiles, 128)};
}
// The tile kernels exist on the split engine only, load 16 bytes at a time (`vec`: aligned operands below 4 GB) and take a
// row map only in whole k-tiles; otherwise the generic GEMM runs at the plan's split count.
static bool bwd_weight_tiled(const TnPlan& p, int mode, bool vec, int M, int a_seg) {
    return p.tile != TN_GENERIC && mode != VSOM_GEMM_F32 && vec && (a_seg == 0 || (a_seg % 32 == 0 && M % a_seg == 0));
}
static long pad4(long n) { return (n + 3) & ~3L; }

// ---- input-gradient GEMM + LayerNorm backward (EPI_LN_BWD): one column tile spanning the LayerNorm's width (the A row
// panel is read once instead of three / one and a half times), 64 x 192 (2 x 2 waves of 32 x 96) for the encoder and
// 128 x 96 (4 waves of 32 x 96) for the decoder.  128 x 192 (4 waves of 32 x 192) needs more than 256 registers per lane
// with the epilogue: one workgroup per CU, or spills.  192 x 192 (gemm_x6_ln_wide_kernel): the transposed weight is staged
// and split once per 192 rows (round 6); its partials keep the 64-row layout, so the workspace and
// finish_many do not change.
enum LnTile : int { LN_NONE = 0, LN_64x192 = 1, LN_128x96 = 2, LN_192x192 = 3 };
struct LnPlan {
    bool supported;             // vsom_linear_bwd_input_ln_supported
    int tile;                   // LnTile; LN_NONE when K is no fused width
    int rows, threads;          // of one workgroup (its tile is K columns wide)
    int planes;                 // 2 in the three-product mode, else 3
    int parts;                  // row tiles of the dgamma / dbeta partials: 64 rows (K = 192) or 128 (K = 96), whatever the tile
    int grid;
};
// test / measurement hook (vsom_set_ln_tiles): 0 = the 64 x 192 tiles only, 1 = 192 x 192 tiles for the encoder width in
// the three-product mode (default).  Both write the same dX and per-64-row partials, bit for bit.
static std::atomic<int> g_ln_tiles{1};
static LnPlan ln_fused_plan(int M, int N, int K, int mode, int ln_tiles) {
    LnPlan p = {};
    if (M <= 0 || (K != 192 && K != 96)) return p;
    p.planes = mode == VSOM_GEMM_SPLIT_BF16_GRAD3 ? 2 : 3;
    p.parts = cdiv(M, K == 192 ? 64 : 128);
    // the column reduction of the one-call form must be the wide single-pass reducer that finish_many runs (>= 32 slabs)
    p.supported = N > 0 && mode != VSOM_GEMM_F32 && p.parts >= 32;
    if (K == 192 && p.planes == 2 && ln_tiles == 1) { p.tile = LN_192x192; p.rows = 192; p.threads = 768; }
    else if (K == 192) { p.tile = LN_64x192; p.rows = 64; p.threads = 256; }
    else { p.tile = LN_128x96; p.rows = 128; p.threads = 256; }
    p.grid = cdiv(M, p.rows);
    return p;
}

static int linear_bwd_input_ln_launch(const float* dY, long lddy, const float* Wt, int M, int N, int K, const float* X,
                                      const float* mean, const float* rstd, const float* gamma, const float* resid,
                                      float* dX, float* part, size_t part_bytes, const LnPlan& p, hipStream_t stream) {
    VSOM_REQUIRE(dY && Wt && X && mean && rstd && gamma && dX, VSOM_EINVAL, "linear_bwd_input_ln: null pointer");
    VSOM_REQUIRE(M > 0 && N > 0 && lddy >= N, VSOM_EINVAL, "linear_bwd_input_ln: bad shape M=%d N=%d lddy=%ld", M, N, lddy);
    VSOM_REQUIRE(p.supported, VSOM_EUNSUPPORTED,
                 "linear_bwd_input_ln: unsupported (M=%d N=%d K=%d, gemm mode %d)", M, N, K, gemm_mode());
    VSOM_REQUIRE(aligned16(dY) && aligned16(Wt) && aligned16(X) && aligned16(gamma) && aligned16(dX) &&
                 (!resid || aligned16(resid)) && lddy % 4 == 0 && N % 4 == 0, VSOM_EALIGN,
                 "linear_bwd_input_ln: operands must be 16-byte aligned (lddy, N multiples of 4)");
    VSOM_REQUIRE(part && aligned16(part) && part_bytes >= (size_t)p.parts * 2 * (size_t)K * sizeof(float), VSOM_EWORKSPACE,
                 "linear_bwd_input_ln: partial buffer too small or misaligned");
    const long ab = operand_bytes(M, lddy, N), bb = operand_bytes(K, N, N);
    VSOM_REQUIRE(ab < 0xFFFF0000L && (long)M * K * 4 < 0xFFFF0000L, VSOM_EUNSUPPORTED, "linear_bwd_input_ln: operand larger than 4 GB");
    GemmP g = {};
    g.A = dY; g.lda = lddy; g.B = Wt; g.ldb = N; g.C = dX; g.ldc = K;
    g.M = M; g.N = K; g.K = N; g.alpha = 1.f;
    g.ktiles_per_split = cdiv(N, 32);
    g.a_vec = g.b_vec = 1;
    g.a_bytes = (unsigned)ab; g.b_bytes = (unsigned)bb;
    g.products = gemm_grad_products();
    g.ln_x = X; g.ln_mean = mean; g.ln_rstd = rstd; g.ln_gamma = gamma; g.ln_resid = resid; g.ln_part = part;
    const dim3 grid(p.grid), block(p.threads);
    switch (p.tile * 4 + p.planes) {
        case LN_192x192 * 4 + 2:
            VSOM_LAUNCH((gemm_x6_ln_wide_kernel<3, 6, 2, 2>), grid, block, 0, stream, g);
            return launch_status("gemm_x6_ln_wide_kernel");
        case LN_64x192 * 4 + 2:
            VSOM_LAUNCH((gemm_x6_ln_kernel<3, 2, 2, 2>), grid, block, 0, stream, g);
            return launch_status("gemm_x6_ln_kernel");
        case LN_64x192 * 4 + 3:
            VSOM_LAUNCH((gemm_x6_ln_kernel<3, 2, 2, 3>), grid, block, 0, stream, g);
            return launch_status("gemm_x6_ln_kernel");
        case LN_128x96 * 4 + 2:
            VSOM_LAUNCH((gemm_x6_ln_kernel<3, 4, 1, 2>), grid, block, 0, stream, g);
            return launch_status("gemm_x6_ln_kernel");
        case LN_128x96 * 4 + 3:
            VSOM_LAUNCH((gemm_x6_ln_kernel<3, 4, 1, 3>), grid, block, 0, stream, g);
            return launch_status("gemm_x6_ln_kernel");
    }
    set_error("linear_bwd_input_ln: plan (tile %d, %d planes) has no kernel", p.tile, p.planes);
    return VSOM_EUNSUPPORTED;
}


// dW[N,K] = sum_m dY[row(m), n] X[m, k] (+ db = column sums of dY rows); row(m) = optional map
int linear_bwd_weight_impl(const float* dY, long lddy, const float* X, long ldx, float* dW, float* db, int M, int N,
                           int K, int a_seg, int a_stride, int a_off, void* ws, size_t ws_bytes,
                           hipStream_t stream) {
    VSOM_REQUIRE(dY && X && dW, VSOM_EINVAL, "linear_bwd_weight: null pointer");
    VSOM_REQUIRE(lddy >= N && ldx >= K, VSOM_EINVAL, "linear_bwd_weight: leading dimension too small");
    VSOM_REQUIRE(ws && ws_bytes >= vsom_linear_bwd_weight_workspace_bytes(M, N, K), VSOM_EWORKSPACE,
                 "linear_bwd_weight: workspace too small (%zu < %zu)", ws_bytes,
                 vsom_linear_bwd_weight_workspace_bytes(M, N, K));
    VSOM_REQUIRE(aligned16(ws), VSOM_EALIGN, "linear_bwd_weight: workspace must be 16-byte aligned");
    const TnPlan plan = bwd_weight_plan(M, N, K, gemm_mode(), g_wgrad_tiles.load(std::memory_order_relaxed));
    const int splits = plan.splits;
    const long wlen = pad4((long)N * K), blen = pad4(N);
    float* slab = static_cast<float*>(ws);
    const long a_last = a_seg ? (long)((M - 1) / a_seg) * a_stride + a_off + (M - 1) % a_seg : M - 1;
    const long ab = (a_last * lddy + N) * 4, bb = ((long)(M - 1) * ldx + K) * 4;
    const bool vec = aligned16(dY) && aligned16(X) && lddy % 4 == 0 && ldx % 4 == 0 && ab < 0xFFFF0000L && bb < 0xFFFF0000L;
    if (!bwd_weight_tiled(plan, gemm_mode(), vec, M, a_seg)) {
        // GEMM rows = n, cols = k, reduction = m; both operands k-strided
        GemmP g = {};
        g.A = dY; g.lda = lddy; g.B = X; g.ldb = ldx;
        g.M = N; g.N = K; g.K = M;
        g.a_seg = a_seg; g.a_stride = a_stride; g.a_off = a_off;
        g.slab = slab; g.slab_stride = wlen + blen;
        g.slab_bias = db ? slab + wlen : nullptr; g.slab_bias_stride = wlen + blen;
        int rc = launch_gemm(false, false, EPI_SLAB, g, splits, stream);
        if (rc) return rc;
        // launch_gemm may have reduced the split count (canonical form): unused slabs were never written
        const int used = cdiv(cdiv(M, 32), cdiv(cdiv(M, 32), splits));
        return reduce_slabs2_internal(slab, wlen + blen, used, dW, (long)N * K, db, wlen, db ? N : 0, stream);
    }
    TnP t = {};
    t.dY = dY; t.X = X; t.ldy = lddy; t.ldx = ldx; t.T = M; t.NO = N; t.KI = K;
    t.ktiles_per_split = cdiv(cdiv(M, 32), splits);
    t.a_seg = a_seg; t.a_stride = a_stride; t.a_off = a_off;
    t.slab = slab; t.slab_stride = wlen + blen;
    t.slab_bias = db ? slab + wlen : nullptr; t.slab_bias_stride = wlen + blen;
    t.a_bytes = (unsigned)ab; t.b_bytes = (unsigned)bb;
    const dim3 grid((N / plan.rows) * (K / plan.cols) * splits), block(plan.threads);
    const int planes = gemm_grad_products() == 3 ? 2 : 3;
    switch (plan.tile * 4 + planes) {
        case TN_192x192 * 4 + 2: VSOM_LAUNCH((gemm_x6_tn_kernel<3, 1, 2, 6, 2, 2>), grid, block, 0, stream, t); break;
        case TN_192x64 * 4 + 2: VSOM_LAUNCH((gemm_x6_tn_kernel<3, 1, 2, 2, 2>), grid, block, 0, stream, t); break;
        case TN_192x64 * 4 + 3: VSOM_LAUNCH((gemm_x6_tn_kernel<3, 1, 2, 2, 3>), grid, block, 0, stream, t); break;
        case TN_96x96 * 4 + 2: VSOM_LAUNCH((gemm_x6_tn_kernel<3, 1, 1, 3, 2>), grid, block, 0, stream, t); break;
        case TN_96x96 * 4 + 3: VSOM_LAUNCH((gemm_x6_tn_kernel<3, 1, 1, 3, 3>), grid, block, 0, stream, t); break;
        default:
            set_error("linear_bwd_weight: plan (tile %d, %d planes) has no kernel", plan.tile, planes);
            return VSOM_EUNSUPPORTED;
    }
    const int rc = launch_status("gemm_x6_tn_kernel");
    if (rc) return rc;
    return reduce_slabs2_internal(slab, wlen + blen, splits, dW, (long)N * K, db, wlen, db ? N : 0, stream);
}

}  // namespace vsom

using namespace vsom;

extern "C" {

int vsom_version(void) { return VSOM_VERSION; }
const char* vsom_last_error_string(void) { return vsom::last_error(); }

int vsom_reduce_slabs(const float* slabs, long stride, int nslabs, float* out, long n, vsom_stream_t stream) {
    VSOM_REQUIRE(slabs && out && nslabs > 0 && n >= 0, VSOM_EINVAL, "reduce_slabs: bad arguments");
    return reduce_slabs_internal(slabs, stride, nslabs, out, n, stream);
}

int vsom_linear_fwd(const float* X, long ldx, const float* W, const float* bias, float* Y, long ldy, int M,
                    int N, int K, vsom_stream_t stream) {
    VSOM_REQUIRE(X && W && Y, VSOM_EINVAL, "linear_fwd: null pointer");
    VSOM_REQUIRE(ldx >= K && ldy >= N, VSOM_EINVAL, "linear_fwd: leading dimension too small");
    GemmP g = {};
    g.A = X; g.lda = ldx; g.B = W; g.ldb = K; g.C = Y; g.ldc = ldy;
    g.M = M; g.N = N; g.K = K; g.bias = bias;
    return launch_gemm(true, true, EPI_BIAS, g, 1, stream);
}

int vsom_linear_gelu_fwd(const float* X, long ldx, const float* W, const float* bias, float* Ygrad, float* Yact,
                         int M, int N, int K, vsom_stream_t stream) {
    float* Ypre = Ygrad;
    VSOM_REQUIRE(X && W && Ypre && Yact, VSOM_EINVAL, "linear_gelu_fwd: null pointer");
    VSOM_REQUIRE(ldx >= K, VSOM_EINVAL, "linear_gelu_fwd: leading dimension too small");
    GemmP g = {};
    g.A = X; g.lda = ldx; g.B = W; g.ldb = K; g.C = Ypre; g.ldc = N; g.C2 = Yact; g.ldc2 = N;
    g.M = M; g.N = N; g.K = K; g.bias = bias;
    return launch_gemm(true, true, EPI_BIAS_GELU, g, 1, stream);
}

int vsom_linear_relu_fwd(const float* X, long ldx, const float* W, const float* bias, float* Ygrad, float* Yact,
                         int M, int N, int K, vsom_stream_t stream) {
    VSOM_REQUIRE(X && W && Ygrad && Yact, VSOM_EINVAL, "linear_relu_fwd: null pointer");
    VSOM_REQUIRE(ldx >= K, VSOM_EINVAL, "linear_relu_fwd: leading dimension too small");
    GemmP g = {};
    g.A = X; g.lda = ldx; g.B = W; g.ldb = K; g.C = Ygrad; g.ldc = N; g.C2 = Yact; g.ldc2 = N;
    g.M = M; g.N = N; g.K = K; g.bias = bias;
    return launch_gemm(true, true, EPI_BIAS_RELU, g, 1, stream);
}

int vsom_linear_residual_fwd(const float* X, long ldx, const float* W, const float* bias, const float* R,
                             long ldr, int r_mod, float* Y, long ldy, int M, int N, int K,
                             vsom_stream_t stream) {
    VSOM_REQUIRE(X && W && R && Y, VSOM_EINVAL, "linear_residual_fwd: null pointer");
    VSOM_REQUIRE(ldx >= K && ldy >= N && ldr >= N && r_mod > 0, VSOM_EINVAL, "linear_residual_fwd: bad leading dimension / r_mod");
    GemmP g = {};
    g.A = X; g.lda = ldx; g.B = W; g.ldb = K; g.C = Y; g.ldc = ldy;
    g.M = M; g.N = N; g.K = K; g.bias = bias; g.R = R; g.ldr = ldr; g.r_mod = r_mod; g.r_off = 0;
    return launch_gemm(true, true, EPI_BIAS_RES, g, 1, stream);
}

int vsom_linear_bwd_input(const float* dY, long lddy, const float* W, float* dX, long lddx, int M, int N, int K,
                          int accumulate, const float* gelu_grad, vsom_stream_t stream) {
    const float* gelu_pre = gelu_grad;
    VSOM_REQUIRE(dY && W && dX, VSOM_EINVAL, "linear_bwd_input: null pointer");
    VSOM_REQUIRE(lddy >= N && lddx >= K, VSOM_EINVAL, "linear_bwd_input: leading dimension too small");
    // dX[M,K] = dY[M,N] * W[N,K]: reduction over N; W is "k-strided" (rows are reduction indices)
    GemmP g = {};
    g.A = dY; g.lda = lddy; g.B = W; g.ldb = K; g.C = dX; g.ldc = lddx;
    g.M = M; g.N = K; g.K = N; g.alpha = 1.f; g.accumulate = accumulate;
    if (gelu_pre) {
        g.R = gelu_pre; g.ldr = K;
        return launch_gemm(true, false, EPI_GELU_BWD, g, 1, stream);
    }
    return launch_gemm(true, false, EPI_NONE, g, 1, stream);
}

int vsom_linear_bwd_input_t(const float* dY, long lddy, const float* Wt, float* dX, long lddx, int M, int N, int K,
                            int accumulate, const float* gelu_grad, vsom_stream_t stream) {
    VSOM_REQUIRE(dY && Wt && dX, VSOM_EINVAL, "linear_bwd_input_t: null pointer");
    VSOM_REQUIRE(lddy >= N && lddx >= K, VSOM_EINVAL, "linear_bwd_input_t: leading dimension too small");
    // dX[M,K] = dY[M,N] * Wt[K,N]^T: both operands contiguous along the reduction (N)
    GemmP g = {};
    g.A = dY; g.lda = lddy; g.B = Wt; g.ldb = N; g.C = dX; g.ldc = lddx;
    g.M = M; g.N = K; g.K = N; g.alpha = 1.f; g.accumulate = accumulate;
    g.products = gemm_grad_products();
    if (gelu_grad) {
        g.R = gelu_grad; g.ldr = K;
        return launch_gemm(true, true, EPI_GELU_BWD, g, 1, stream);
    }
    return launch_gemm(true, true, EPI_NONE, g, 1, stream);
}

static LnPlan ln_fused_plan_now(int M, int N, int K) {
    return ln_fused_plan(M, N, K, gemm_mode(), g_ln_tiles.load(std::memory_order_relaxed));
}

int vsom_linear_bwd_input_ln_supported(int M, int N, int K) { return ln_fused_plan_now(M, N, K).supported; }

size_t vsom_linear_bwd_input_ln_partial_bytes(int M, int K) {
    return (size_t)ln_fused_plan_now(M, 1, K).parts * 2 * (size_t)K * sizeof(float);       // whatever N, mode and hook
}

int vsom_linear_bwd_input_ln(const float* dY, long lddy, const float* Wt, int M, int N, int K, const float* X,
                             const float* mean, const float* rstd, const float* gamma, const float* resid, float* dX,
                             float* dgamma, float* dbeta, void* ws, size_t ws_bytes, vsom_stream_t stream) {
    VSOM_REQUIRE(dgamma && dbeta, VSOM_EINVAL, "linear_bwd_input_ln: null pointer");
    float* part = static_cast<float*>(ws);
    const LnPlan p = ln_fused_plan_now(M, N, K);
    const int rc = linear_bwd_input_ln_launch(dY, lddy, Wt, M, N, K, X, mean, rstd, gamma, resid, dX, part, ws_bytes, p, stream);
    if (rc) return rc;
    // same reducer, arguments and order as vsom_layernorm_bwd_finish_many on this job
    return reduce_slabs2_internal(part, 2L * K, p.parts, dgamma, K, dbeta, K, K, stream);
}

int vsom_linear_bwd_input_ln_partial(const float* dY, long lddy, const float* Wt, int M, int N, int K, const float* X,
                                     const float* mean, const float* rstd, const float* gamma, const float* resid,
                                     float* dX, void* part, size_t part_bytes, vsom_stream_t stream) {
    return linear_bwd_input_ln_launch(dY, lddy, Wt, M, N, K, X, mean, rstd, gamma, resid, dX, static_cast<float*>(part),
                                      part_bytes, ln_fused_plan_now(M, N, K), stream);
}

int vsom_set_gemm_mode(int mode) {
    VSOM_REQUIRE(mode == VSOM_GEMM_F32 || mode == VSOM_GEMM_SPLIT_BF16 || mode == VSOM_GEMM_SPLIT_BF16_GRAD3, VSOM_EINVAL,
                 "set_gemm_mode: unknown mode %d", mode);
    g_gemm_mode.store(mode, std::memory_order_relaxed);
    return VSOM_OK;
}
int vsom_get_gemm_mode(void) { return gemm_mode(); }

int vsom_set_ln_tiles(int mode) {
    VSOM_REQUIRE(mode == 0 || mode == 1, VSOM_EINVAL, "set_ln_tiles: unknown mode %d", mode);
    g_ln_tiles.store(mode, std::memory_order_relaxed);
    return VSOM_OK;
}

int vsom_set_wgrad_tiles(int mode) {
    VSOM_REQUIRE(mode >= 0 && mode <= 2, VSOM_EINVAL, "set_wgrad_tiles: unknown mode %d", mode);
    g_wgrad_tiles.store(mode, std::memory_order_relaxed);
    return VSOM_OK;
}

// The (layout, epilogue, GEMM shape, products, splits) of each entry point that is one launch_gemm call.
static int describe_gemm(bool a_kc, bool b_kc, int epi, int M, int N, int K, bool vec, int products, int splits, char* out,
                         size_t out_bytes) {
    const bool fast = vec && gemm_vec_extents(a_kc, b_kc, M, N, K);
    const GemmPlan p = gemm_plan(a_kc, b_kc, epi, M, N, K, fast, gemm_mode(), products, splits);
    const int n = snprintf(out, out_bytes, "engine=%s tile=%dx64 planes=%d fast=%d threads=256 splits=%d workgroups=%d",
                           p.engine == GEMM_ENGINE_X6 ? "x6" : "f32", p.tile_m, p.planes, (int)p.fast, p.splits, p.grid);
    VSOM_REQUIRE(n > 0 && (size_t)n < out_bytes, VSOM_EINVAL, "describe_plan: buffer too small");
    return VSOM_OK;
}

int vsom_describe_plan(int op, int M, int N, int K, int flags, char* out, size_t out_bytes) {
    VSOM_REQUIRE(out && out_bytes > 0, VSOM_EINVAL, "describe_plan: null buffer");
    out[0] = 0;
    VSOM_REQUIRE(M > 0 && N > 0 && K > 0, VSOM_EINVAL, "describe_plan: non-positive shape %d %d %d", M, N, K);
    const bool vec = flags & 1;
    const int g3 = gemm_grad_products();
    int n = 0;
    switch (op) {
        case VSOM_PLAN_LINEAR_FWD: return describe_gemm(true, true, EPI_BIAS, M, N, K, vec, 0, 1, out, out_bytes);
        case VSOM_PLAN_LINEAR_GELU_FWD: return describe_gemm(true, true, EPI_BIAS_GELU, M, N, K, vec, 0, 1, out, out_bytes);
        case VSOM_PLAN_LINEAR_RELU_FWD: return describe_gemm(true, true, EPI_BIAS_RELU, M, N, K, vec, 0, 1, out, out_bytes);
        case VSOM_PLAN_LINEAR_RESIDUAL_FWD: return describe_gemm(true, true, EPI_BIAS_RES, M, N, K, vec, 0, 1, out, out_bytes);
        // dX[M,K] = dY[M,N] W: the reduction runs over N
        case VSOM_PLAN_LINEAR_BWD_INPUT: return describe_gemm(true, false, EPI_NONE, M, K, N, vec, 0, 1, out, out_bytes);
        case VSOM_PLAN_LINEAR_BWD_INPUT_GELU: return describe_gemm(true, false, EPI_GELU_BWD, M, K, N, vec, 0, 1, out, out_bytes);
        case VSOM_PLAN_LINEAR_BWD_INPUT_T: return describe_gemm(true, true, EPI_NONE, M, K, N, vec, g3, 1, out, out_bytes);
        case VSOM_PLAN_LINEAR_BWD_INPUT_T_GELU: return describe_gemm(true, true, EPI_GELU_BWD, M, K, N, vec, g3, 1, out, out_bytes);
        // (B, K, L): gW[K,L] reduces over the batch, gX[B,L] over the prototypes, the dots [B,K] over L
        case VSOM_PLAN_SOM_BWD_GW: return describe_gemm(false, false, EPI_ROWAXPY, N, K, M, vec, g3, 1, out, out_bytes);
        case VSOM_PLAN_SOM_BWD_GX: return describe_gemm(true, false, EPI_ROWAXPY, M, K, N, vec, g3, 1, out, out_bytes);
        case VSOM_PLAN_BMU_COSINE_DOTS:
        case VSOM_PLAN_BMU_COSINE: {
            const BmuPlan p = bmu_plan(M, N, K, K, vec, op == VSOM_PLAN_BMU_COSINE ? gemm_mode() : VSOM_GEMM_F32, flags & 2);
            if (p.form == VSOM_BMU_EXACT) return describe_gemm(true, true, EPI_SLAB, M, N, K, vec, 0, p.splits, out, out_bytes);
            n = snprintf(out, out_bytes, "engine=%s tile=%dx%d planes=2 fast=1 threads=%d splits=%d workgroups=%d",
                         p.form == VSOM_BMU_X3_PLANES ? "bmu_x3_planes" : "bmu_x3", p.tile_m, p.tile_n, p.threads, p.splits,
                         p.tiles * p.splits);
            break;
        }
        case VSOM_PLAN_LINEAR_BWD_WEIGHT: {
            const TnPlan p = bwd_weight_plan(M, N, K, gemm_mode(), g_wgrad_tiles.load(std::memory_order_relaxed));
            if (!bwd_weight_tiled(p, gemm_mode(), vec, M, 0))
                return describe_gemm(false, false, EPI_SLAB, N, K, M, vec, 0, p.splits, out, out_bytes);
            n = snprintf(out, out_bytes, "engine=x6_tn tile=%dx%d planes=%d fast=1 threads=%d splits=%d workgroups=%d", p.rows, p.cols,
                         g3 == 3 ? 2 : 3, p.threads, p.splits, (N / p.rows) * (K / p.cols) * p.splits);
            break;
        }
        case VSOM_PLAN_LINEAR_BWD_INPUT_LN: {
            const LnPlan p = ln_fused_plan_now(M, N, K);
            VSOM_REQUIRE(p.supported && vec, VSOM_EUNSUPPORTED, "describe_plan: linear_bwd_input_ln does not take M=%d N=%d K=%d", M, N, K);
            n = snprintf(out, out_bytes, "engine=x6_ln tile=%dx%d planes=%d fast=1 threads=%d splits=1 workgroups=%d", p.rows, K, p.planes,
                         p.threads, p.grid);
            break;
        }
        case VSOM_PLAN_ATTENTION_BWD: {
            static const char* const form[] = {"attn_two_launch", "attn_fused", "attn_shared", "attn_shared_bf16x3"};
            const int plan = attn_bwd_plan_now(M, K);
            VSOM_REQUIRE(plan >= 0, VSOM_EUNSUPPORTED, "describe_plan: attention head dim %d not supported", K);
            n = snprintf(out, out_bytes, "engine=%s tile=16x16 planes=%d fast=1 threads=%d splits=1 workgroups=%d", form[plan],
                         plan == 3 ? 2 : 0, attn_bwd_threads(M), N);
            break;
        }
        default:
            set_error("describe_plan: unknown op %d", op);
            return VSOM_EINVAL;
    }
    VSOM_REQUIRE(n > 0 && (size_t)n < out_bytes, VSOM_EINVAL, "describe_plan: buffer too small");
    return VSOM_OK;
}

size_t vsom_linear_bwd_weight_workspace_bytes(int M, int N, int K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    const int s = bwd_weight_plan(M, N, K, gemm_mode(), g_wgrad_tiles.load(std::memory_order_relaxed)).splits;
    return (size_t)s * (size_t)(pad4((long)N * K) + pad4(N)) * sizeof(float);
}

int vsom_linear_bwd_weight(const float* dY, long lddy, const float* X, long ldx, float* dW, float* db, int M,
                           int N, int K, void* ws, size_t ws_bytes, vsom_stream_t stream) {
    return linear_bwd_weight_impl(dY, lddy, X, ldx, dW, db, M, N, K, 0, 0, 0, ws, ws_bytes, stream);
}

}  // extern "C"
