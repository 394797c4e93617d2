// Kohonen's batch map on the device (SOMLayer.fit_batch; no counterpart in the reference): one epoch at radius sigma is
//
//   vsom_som_batch_accumulate   n_c = #{i : bmu_i = c},  S_c = sum over those rows of x_i (* inv_norm_i), fp64
//   vsom_som_batch_update       W_k = sum_c h(k,c) S_c / sum_c h(k,c) n_c,  h(k,c) = exp(-(d2(k,c) - m_k) / (2 sigma^2))
//                               over the units with hits, m_k = the smallest d2(k,c) among them (reasons: DESIGN.md section 4)
//
// ACCUMULATE.  Every (unit, column) is ONE fp64 chain over the unit's rows in ascending row index: the rows of a unit are
// a run of `order`, the stable sort of the BMUs the caller passes in.  A chain cannot be split without changing its bits,
// so the parallelism of the ADDS is columns x units; the LOADS of a long unit's rows are spread over the four waves of a
// workgroup (16-byte path, bs_accumulate_vec_kernel), since a few units hold most rows while the radius is wide.  No
// floating-point atomics; the result does not depend on how the rows were cut into calls (accumulate = 1 continues the
// chain from what `sums` holds) and equals np.add.at in fp64 bit for bit (the product of two f32 values is exact in fp64,
// so a contraction of the product into an fma changes nothing).
// UPDATE.  The numerator is a [K x K] . [K x D] contraction on the exact-f32 matrix cores (v_mfma_f32_32x32x2_f32).  The A
// tile is GENERATED from the grid positions while it is stored to LDS (no [K, K] matrix in memory): the exponent is formed
// in fp64 -- d2 and m_k are close and large for a unit far from every hit, in f32 their difference loses the digits the
// Gaussian needs -- rounded once to f32 and given to the hardware exp2.  S is rounded to f32 as its tile is loaded.  The
// reduction over c runs in ascending k-tiles inside one workgroup, in segments of 128 units whose sums are added in
// order: one fixed order, bitwise reproducible.  m_k, the denominators and the hit units' positions come from a small
// fp64 pre-pass.
#include "gemm_f32.h"

#include <math.h>

namespace vsom {
namespace {

constexpr int ACC_UNROLL = 8;                // element-wise path: gathered rows a thread keeps in flight
constexpr int AV_COLS = 256, AV_PER_WAVE = 16, AV_ROWS = 4 * AV_PER_WAVE;      // 16-byte path: the LDS tile of a batch
constexpr int AV_LONG_SEGMENT = 256;         // 16-byte path: a unit with more rows goes to the cooperative kernel
constexpr int BS_MAX_UNITS = 65535;          // the unit is a grid coordinate
constexpr int UP_BM = 128, UP_BN = 128;      // update tile: 4 waves x (32 rows x 128 columns)
constexpr int UP_ALD = 36, UP_BLD = 36;      // both LDS tiles are [row or column][k], 32 k-values in a pitch of 36 floats
static_assert(f32_tile_floats<true, 1>() == UP_ALD && UP_BLD == UP_ALD, "mfma_tile reads the k-contiguous tile image of gemm_f32.h");
constexpr int UP_SEG_KTILES = 4;            // k-tiles of 32 units per first-level sum

// --------------------------------------------------------------------------------------------------- accumulate
// seg[c] = the first position of `order` whose row has a BMU >= c (c = 0 .. K): unit c owns order[seg[c] .. seg[c + 1]).
// A row index outside [0, N) counts as a key beyond every unit.  Threads below N also check their BMU and order entry.
__global__ __launch_bounds__(256) void bs_segments_kernel(const int64_t* __restrict__ bmu, const int64_t* __restrict__ order, long N,
                                                          int K, int64_t* __restrict__ seg, int* __restrict__ bad) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < N) {
        const int64_t b = bmu[i], o = order[i];
        if (b < 0 || b >= K || o < 0 || o >= N) atomicAdd(bad, 1);
    }
    if (i <= K) {
        long lo = 0, hi = N;
        while (lo < hi) {
            const long mid = lo + ((hi - lo) >> 1);
            const int64_t o = order[mid];
            const int64_t key = (o >= 0 && o < N) ? bmu[o] : INT64_MAX;
            if (key < i) lo = mid + 1;
            else hi = mid;
        }
        seg[i] = lo;
    }
}

// Units with at most `most` rows (all of them on the element-wise path): a wave owns 64 x W columns of one unit, a thread W
// columns and 8 gathered rows in flight.  Tens of thousands of short segments keep the device full this way.
template <bool VEC>
__global__ __launch_bounds__(64) void bs_accumulate_kernel(const float* __restrict__ X, long ldx, long N, int D,
                                                          const int64_t* __restrict__ order, const float* __restrict__ inv_norm,
                                                          const int64_t* __restrict__ seg, double* __restrict__ sums,
                                                          int64_t* __restrict__ counts, int accumulate, long most) {
    constexpr int W = VEC ? 4 : 1;
    const int c = blockIdx.y;
    const long j0 = seg[c], j1 = seg[c + 1];
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[c] = (accumulate ? counts[c] : 0) + (j1 - j0);
    if (j1 - j0 > most) return;                              // bs_accumulate_vec_kernel's
    const int col = (blockIdx.x * 64 + threadIdx.x) * W;
    if (col >= D) return;
    double* out = sums + (long)c * D + col;
    double acc[W];
#pragma unroll
    for (int e = 0; e < W; ++e) acc[e] = accumulate ? out[e] : 0.0;

    auto load = [&](long j, float (&v)[W], float& s) {
        const int64_t row = order[j];
        const bool ok = row >= 0 && row < N;                 // flagged by bs_segments_kernel; never dereferenced
        s = 0.f;
#pragma unroll
        for (int e = 0; e < W; ++e) v[e] = 0.f;
        if (ok) {
            const float* p = X + row * ldx + col;
            if constexpr (VEC) {
                const f32x4 q = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = q[e];
            } else {
                v[0] = *p;
            }
            s = inv_norm ? inv_norm[row] : 1.f;
        }
        return ok;
    };
    long j = j0;
    for (; j + ACC_UNROLL <= j1; j += ACC_UNROLL) {
        float v[ACC_UNROLL][W], s[ACC_UNROLL];
        bool ok[ACC_UNROLL];
#pragma unroll
        for (int u = 0; u < ACC_UNROLL; ++u) ok[u] = load(j + u, v[u], s[u]);
#pragma unroll
        for (int u = 0; u < ACC_UNROLL; ++u)
            if (ok[u]) {
#pragma unroll
                for (int e = 0; e < W; ++e) acc[e] += (double)v[u][e] * (double)s[u];
            }
    }
    for (; j < j1; ++j) {
        float v[W], s;
        if (load(j, v, s)) {
#pragma unroll
            for (int e = 0; e < W; ++e) acc[e] += (double)v[e] * (double)s;
        }
    }
#pragma unroll
    for (int e = 0; e < W; ++e) out[e] = acc[e];
}

// Units with more than `most` rows on the 16-byte path.  The chain of a (unit, column) is serial, but the LOADS need not
// be: early epochs put thousands of rows into a few units, and a wave that walks such a segment alone keeps 8 KB in flight
// -- a few hundred waves on the whole device, 0.4 TB/s measured.  Here a workgroup of four waves owns 256 columns of one
// unit; all of them gather rows as float4 (wave w the rows w, w + 4, ... of a batch of 64, sixteen loads in flight per
// lane) into an LDS tile, then every thread adds the batch's rows, in ascending order, into the one column it owns.  The
// next batch's loads are in flight under the adds.
__global__ __launch_bounds__(256) void bs_accumulate_vec_kernel(const float* __restrict__ X, long ldx, long N, int D,
                                                               const int64_t* __restrict__ order, const float* __restrict__ inv_norm,
                                                               const int64_t* __restrict__ seg, double* __restrict__ sums,
                                                               int accumulate, long most) {
    __shared__ __attribute__((aligned(16))) float tile[AV_ROWS][AV_COLS];
    __shared__ float scl[AV_ROWS];
    __shared__ int okf[AV_ROWS];
    const int c = blockIdx.y, t = threadIdx.x, lane = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const long j0 = seg[c], j1 = seg[c + 1];
    if (j1 - j0 <= most) return;                             // bs_accumulate_kernel's (it also writes every count)
    const int lcol = blockIdx.x * AV_COLS + lane * 4;         // the four columns this lane loads (D % 4 == 0)
    const int col = blockIdx.x * AV_COLS + t;                // the column this thread sums
    double* out = sums + (long)c * D + col;
    double acc = (col < D && accumulate) ? *out : 0.0;

    f32x4 v[AV_PER_WAVE];
    float s[AV_PER_WAVE];
    bool ok[AV_PER_WAVE];
    auto gather = [&](long jb) {
#pragma unroll
        for (int u = 0; u < AV_PER_WAVE; ++u) {
            const long j = jb + u * 4 + w;
            v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            s[u] = 0.f;
            ok[u] = false;
            if (j < j1) {
                const int64_t row = order[j];
                ok[u] = row >= 0 && row < N;                 // flagged by bs_segments_kernel; never dereferenced
                if (ok[u]) {
                    if (lcol < D) v[u] = *reinterpret_cast<const f32x4*>(X + row * ldx + lcol);
                    s[u] = inv_norm ? inv_norm[row] : 1.f;
                }
            }
        }
    };
    if (j0 < j1) gather(j0);
    for (long jb = j0; jb < j1; jb += AV_ROWS) {
#pragma unroll
        for (int u = 0; u < AV_PER_WAVE; ++u) {
            const int r = u * 4 + w;
            *reinterpret_cast<f32x4*>(&tile[r][lane * 4]) = v[u];
            if (lane == 0) { scl[r] = s[u]; okf[r] = ok[u]; }
        }
        __syncthreads();
        if (jb + AV_ROWS < j1) gather(jb + AV_ROWS);
        const int rows = (int)(j1 - jb < AV_ROWS ? j1 - jb : AV_ROWS);
        for (int r = 0; r < rows; ++r)
            if (okf[r]) acc += (double)tile[r][t] * (double)scl[r];
        __syncthreads();
    }
    if (col < D) *out = acc;
}

// --------------------------------------------------------------------------------------------------- update
// part: [mks K | den K | cx K | cy K] doubles.  Workgroup k: m_k = min over the hit units of d2(k, c); mks = m_k s2 with
// s2 = log2(e) / (2 sigma^2), so that h(k, c) = exp2(mks - d2 s2); den_k = sum_c n_c h(k, c): per-thread sums over
// c = t, t + 256, ... in ascending order, then a fixed tree.  cx / cy: the unit's position, cx = +inf for a unit without
// hits -- its d2 is +inf and its h exactly 0 with no branch in the tile generator.  No hit anywhere: mks = 0, den = 0.
__device__ __forceinline__ double grid_d2(double ax, double ay, double bx, double by) {
    const double dx = ax - bx, dy = ay - by;
    return dx * dx + dy * dy;
}

__global__ __launch_bounds__(256) void bs_prepare_kernel(const int64_t* __restrict__ counts, const float* __restrict__ pos, int K,
                                                         double s2, double* __restrict__ part) {
    __shared__ double sh[256];
    const int k = blockIdx.x, t = threadIdx.x;
    const double kx = (double)pos[2 * k], ky = (double)pos[2 * k + 1];
    double m = INFINITY;
    for (int c = t; c < K; c += 256)
        if (counts[c] > 0) m = fmin(m, grid_d2(kx, ky, (double)pos[2 * c], (double)pos[2 * c + 1]));
    sh[t] = m;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) sh[t] = fmin(sh[t], sh[t + o]);
        __syncthreads();
    }
    m = sh[0];
    __syncthreads();
    const bool any = m < INFINITY;
    const double mks = any ? m * s2 : 0.0;
    double den = 0.0;
    for (int c = t; c < K; c += 256) {
        const int64_t n = counts[c];
        if (n > 0) den += (double)n * exp2(fma(-grid_d2(kx, ky, (double)pos[2 * c], (double)pos[2 * c + 1]), s2, mks));
    }
    sh[t] = den;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) sh[t] += sh[t + o];
        __syncthreads();
    }
    if (t == 0) {
        part[k] = mks;
        part[K + k] = sh[0];
        part[2L * K + k] = counts[k] > 0 ? kx : (double)INFINITY;
        part[3L * K + k] = ky;
    }
}

// W_out tile [128 units x 128 columns]; wave w owns the units 32 w .. 32 w + 31.  FAST: D % 4 == 0 and sums 16-byte aligned.
template <bool FAST>
__global__ __launch_bounds__(256, 2) void bs_update_kernel(const double* __restrict__ sums, const int64_t* __restrict__ counts,
                                                        const float* __restrict__ pos, const double* __restrict__ part, int K, int D,
                                                        double s2, float* __restrict__ W_out, long ldw) {
    __shared__ __attribute__((aligned(16))) float As[UP_BM * UP_ALD];
    __shared__ __attribute__((aligned(16))) float Bs[UP_BN * UP_BLD];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wm0 = wave * 32;
    const int tiles_m = (K + UP_BM - 1) / UP_BM;
    // the row tiles of one column panel of S are neighbours in the logical order: they share the panel in one XCD's L2
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int tm = lid % tiles_m, tn = lid / tiles_m;
    const int bm0 = tm * UP_BM, bn0 = tn * UP_BN;
    const int ktiles = (K + 31) >> 5;

    // the generator's unit: row `gm` of the tile, the 16 reduction indices of half `gh`
    // (the half is the same for a whole wave: made a scalar, the hit units' positions come through scalar loads)
    const int gm = t & (UP_BM - 1), gh = __builtin_amdgcn_readfirstlane(t >> 7);
    const int gk = bm0 + gm;
    double kx = 0.0, ky = 0.0, mks = 0.0;
    if (gk < K) { kx = (double)pos[2 * gk]; ky = (double)pos[2 * gk + 1]; mks = part[gk]; }
    const double* cxs = part + 2L * K;
    const double* cys = part + 3L * K;
    auto gen_a = [&](int kt) {
        const int c0 = (kt << 5) + gh * 16;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f32x4 a;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = c0 + q * 4 + e;
                const double cx = c < K ? cxs[c] : (double)INFINITY, cy = c < K ? cys[c] : 0.0;
                a[e] = __builtin_amdgcn_exp2f((float)fma(-grid_d2(kx, ky, cx, cy), s2, mks));
            }
            *reinterpret_cast<f32x4*>(As + gm * UP_ALD + gh * 16 + q * 4) = a;
        }
    };
    // the loader's elements: 4 columns of the rows br, br + 8, br + 16, br + 24 of the k-tile
    const int bc = (t & 31) << 2, br = t >> 5;
    const int col = bn0 + bc;
    double bv[4][4];
    auto load_b = [&](int kt) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int c = (kt << 5) + br + 8 * p;
#pragma unroll
            for (int e = 0; e < 4; ++e) bv[p][e] = 0.0;
            if (c < K && counts[c] > 0) {                    // a unit without hits contributes exactly nothing
                const double* s = sums + (long)c * D + col;
                if constexpr (FAST) {
                    if (col < D) {
                        const double2 lo = *reinterpret_cast<const double2*>(s), hi = *reinterpret_cast<const double2*>(s + 2);
                        bv[p][0] = lo.x; bv[p][1] = lo.y; bv[p][2] = hi.x; bv[p][3] = hi.y;
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (col + e < D) bv[p][e] = s[e];
                }
            }
        }
    };
    auto store_b = [&]() {                                   // transposed: a lane of the MFMA loop reads four k-values at once
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int e = 0; e < 4; ++e) Bs[(bc + e) * UP_BLD + br + 8 * p] = (float)bv[p][e];
    };

    // two-level sum: `acc` takes UP_SEG_KTILES k-tiles (128 units), then goes into `tot` -- a chain of 1 600 f32 additions
    // per output would use up the tolerance a float32 evaluation of the formula sets
    f32x16 acc[4], tot[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int v = 0; v < 16; ++v) { acc[j][v] = 0.f; tot[j][v] = 0.f; }

    load_b(0);
    gen_a(0);
    store_b();
    __syncthreads();
    for (int kt = 0; kt < ktiles; ++kt) {
        const bool more = kt + 1 < ktiles;
        mfma_tile<true, true, UP_BM, UP_BN>(As, Bs, wm0, 0, r, h, reinterpret_cast<f32x16 (&)[1][4]>(acc));
        if ((kt + 1) % UP_SEG_KTILES == 0 || !more) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                tot[j] += acc[j];
#pragma unroll
                for (int v = 0; v < 16; ++v) acc[j][v] = 0.f;
            }
        }
        __syncthreads();
        if (more) {
            load_b(kt + 1);                                  // in flight under the generator's arithmetic
            gen_a(kt + 1);
            store_b();
        }
        __syncthreads();
    }

    // register v of an accumulator is row 4 h + (v & 3) + 8 (v >> 2), column r of its 32 x 32 block
    const double* den = part + K;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int k = bm0 + wm0 + 4 * h + (v & 3) + 8 * (v >> 2);
        if (k >= K) continue;
        const double d = den[k];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = bn0 + j * 32 + r;
            if (n < D) W_out[(long)k * ldw + n] = d > 0.0 ? (float)((double)tot[j][v] / d) : 0.f;
        }
    }
}

// x / max(|x|_2, 1e-12) per row (torch.nn.functional.normalize): the squares summed in fp64, per-thread sums over
// d = t, t + 256, ... in ascending order, then a fixed tree
__global__ __launch_bounds__(256) void bs_row_normalize_kernel(float* __restrict__ W, long ldw, int D) {
    __shared__ double sh[256];
    float* w = W + (long)blockIdx.x * ldw;
    const int t = threadIdx.x;
    double ss = 0.0;
    for (int d = t; d < D; d += 256) ss = fma((double)w[d], (double)w[d], ss);
    sh[t] = ss;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) sh[t] += sh[t + o];
        __syncthreads();
    }
    const float nrm = fmaxf((float)sqrt(sh[0]), 1e-12f);
    for (int d = t; d < D; d += 256) w[d] = w[d] / nrm;
}

}  // namespace
}  // namespace vsom

using namespace vsom;

extern "C" {

long vsom_som_batch_accumulate_parts(int K) { return K >= 1 && K <= BS_MAX_UNITS ? (long)K + 1 : 0; }

int vsom_som_batch_accumulate(const float* X, long ldx, long N, int D, const int64_t* bmu, const int64_t* order,
                              const float* inv_norm, int K, double* sums, int64_t* counts, int accumulate, int* bad, int64_t* seg,
                              long n_seg, vsom_stream_t stream) {
    VSOM_REQUIRE(sums && counts && bad, VSOM_EINVAL, "som_batch_accumulate: null pointer");
    VSOM_REQUIRE(N >= 0 && D >= 1 && K >= 1 && ldx >= D, VSOM_EINVAL, "som_batch_accumulate: bad sizes N=%ld D=%d K=%d ldx=%ld", N, D,
                 K, ldx);
    VSOM_REQUIRE(N == 0 || (X && bmu && order), VSOM_EINVAL, "som_batch_accumulate: null pointer");
    VSOM_REQUIRE(K <= BS_MAX_UNITS, VSOM_EUNSUPPORTED, "som_batch_accumulate: K=%d > %d units", K, BS_MAX_UNITS);
    const long need = vsom_som_batch_accumulate_parts(K);
    VSOM_REQUIRE(seg && n_seg >= need, VSOM_EWORKSPACE, "som_batch_accumulate: segment buffer null or too small (%ld < %ld int64)",
                 n_seg, need);
    const long most = N > K + 1 ? N : K + 1;
    VSOM_LAUNCH(bs_segments_kernel, dim3(cdiv(most, 256)), dim3(256), 0, stream, bmu, order, N, K, seg, bad);
    if (int rc = launch_status("bs_segments_kernel")) return rc;
    const bool vec = D % 4 == 0 && ldx % 4 == 0 && aligned16(X);
    if (!vec) {
        VSOM_LAUNCH((bs_accumulate_kernel<false>), dim3(cdiv(D, 64), K), dim3(64), 0, stream, X, ldx, N, D, order, inv_norm,
                    (const int64_t*)seg, sums, counts, accumulate, N);
        return launch_status("bs_accumulate_kernel");
    }
    // every unit is summed by exactly one of the two kernels, and both walk its rows in the same order: the same bits
    VSOM_LAUNCH((bs_accumulate_kernel<true>), dim3(cdiv(D, 256), K), dim3(64), 0, stream, X, ldx, N, D, order, inv_norm,
                (const int64_t*)seg, sums, counts, accumulate, (long)AV_LONG_SEGMENT);
    if (int rc = launch_status("bs_accumulate_kernel")) return rc;
    if (N <= AV_LONG_SEGMENT) return VSOM_OK;                // no unit can have a long segment
    VSOM_LAUNCH(bs_accumulate_vec_kernel, dim3(cdiv(D, AV_COLS), K), dim3(256), 0, stream, X, ldx, N, D, order, inv_norm,
                (const int64_t*)seg, sums, accumulate, (long)AV_LONG_SEGMENT);
    return launch_status("bs_accumulate_vec_kernel");
}

long vsom_som_batch_update_parts(int K) { return K >= 1 ? 4L * K : 0; }

int vsom_som_batch_update(const double* sums, const int64_t* counts, const float* grid_positions, int K, int D, double sigma,
                          int normalize, float* W_out, long ldw, double* part, long n_part, vsom_stream_t stream) {
    VSOM_REQUIRE(sums && counts && grid_positions && W_out, VSOM_EINVAL, "som_batch_update: null pointer");
    VSOM_REQUIRE(K >= 1 && D >= 1 && ldw >= D, VSOM_EINVAL, "som_batch_update: bad sizes K=%d D=%d ldw=%ld", K, D, ldw);
    VSOM_REQUIRE(isfinite(sigma) && sigma > 0.0, VSOM_EINVAL, "som_batch_update: sigma=%g is not a positive finite radius", sigma);
    const double s2 = 1.4426950408889634 / (2.0 * sigma * sigma);
    VSOM_REQUIRE(isfinite(s2) && s2 > 0.0, VSOM_EINVAL, "som_batch_update: sigma=%g: 1 / (2 sigma^2) is not a positive finite number",
                 sigma);
    const long need = vsom_som_batch_update_parts(K);
    VSOM_REQUIRE(part && n_part >= need, VSOM_EWORKSPACE, "som_batch_update: partial buffer null or too small (%ld < %ld doubles)",
                 n_part, need);
    const long tiles = (long)cdiv(K, UP_BM) * cdiv(D, UP_BN);
    VSOM_REQUIRE(tiles < 0x7fffffffL, VSOM_EUNSUPPORTED, "som_batch_update: %ld output tiles", tiles);
    VSOM_LAUNCH(bs_prepare_kernel, dim3(K), dim3(256), 0, stream, counts, grid_positions, K, s2, part);
    if (int rc = launch_status("bs_prepare_kernel")) return rc;
    if (D % 4 == 0 && aligned16(sums))
        VSOM_LAUNCH((bs_update_kernel<true>), dim3((int)tiles), dim3(256), 0, stream, sums, counts, grid_positions, (const double*)part, K,
                    D, s2, W_out, ldw);
    else
        VSOM_LAUNCH((bs_update_kernel<false>), dim3((int)tiles), dim3(256), 0, stream, sums, counts, grid_positions, (const double*)part,
                    K, D, s2, W_out, ldw);
    if (int rc = launch_status("bs_update_kernel")) return rc;
    if (normalize) {
        VSOM_LAUNCH(bs_row_normalize_kernel, dim3(K), dim3(256), 0, stream, W_out, ldw, D);
        return launch_status("bs_row_normalize_kernel");
    }
    return VSOM_OK;
}

}  // extern "C"
