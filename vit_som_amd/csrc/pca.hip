// Principal component analysis of a row set on the device (vit_som_amd/pca.py; no counterpart in the reference): the
// kernels of a block subspace iteration on the covariance operator of X [N, D].
//
//   vsom_pca_colstats     column mean (fp64 sums, one rounding to f32) and unbiased column variance (fp64, about that
//                         rounded mean), split over the rows, the per-split partials added in split order.
//   vsom_pca_project      Y  = (X - mean) B^T diag(scale)     "NT": both operands k-contiguous, the reduction runs over D
//   vsom_pca_backproject  Zt = Y^T (X - mean)                 "TN": both operands k-strided, the reduction runs over the rows
//   vsom_pca_gram         G = Zt Zt^T and H = B Zt^T in fp64, every entry one fixed-order sum over D.
//   vsom_pca_rotate       Bout = T Zt, T fp64 [l_out, l_in]: fp64 accumulation, one rounding to f32.
//   vsom_pca_reconstruct  Xout = (Y diag(scale)) B + mean.
//
// The two contractions run on the exact-f32 matrix cores and are the shared tile contraction of gemm_f32.h -- its staging
// (F32Stage), its k-loop (F32_KLOOP), its MFMA order (mfma_tile), its LDS images and its slab epilogue: the same code as
// gemm_f32_kernel's, not a copy.  What pca_gemm_kernel adds is the CENTRING ON LOAD: the mean is subtracted from an X tile between the global load and
// the LDS store, never algebraically after the contraction -- latents have column means that are large against their
// spread, and X B^T - 1 (mean^T B^T) cancels in f32.  A tile element outside the matrix (a row >= N, a column >= D, the
// zero an out-of-range buffer load returns) must stay zero AFTER centring: the mean vector a thread subtracts is zero
// outside [0, D), and it is subtracted only from elements whose row is inside the matrix.
// With l <= 256 the output has few tiles, so both contractions split their reduction, write per-split slabs and add them
// in split order (pca_reduce_kernel): no floating-point atomics, every sum has one fixed order, results are bitwise
// reproducible.  The split count is a function of the shape alone, so that the count query and the launch agree on any host.
#include "gemm_f32.h"

namespace vsom {
namespace {

constexpr int PCA_MAX_L = 256;
constexpr int PCA_BM = 128, PCA_BN = 64;     // the 128 x 64 tile of gemm_f32_kernel: 4 waves x (1 x 2) accumulators
constexpr int PCA_TARGET_BLOCKS = 768;       // three co-resident workgroups on each of 256 CUs
constexpr int PCA_MAX_SPLITS = 64;
constexpr int CS_COLS = 64, CS_LANES = 8;    // colstats workgroup: 64 columns x 8 row lanes
constexpr int GRAM_THREADS = 1024, GRAM_WAVES = GRAM_THREADS / 64;
constexpr int CS_MIN_ROWS = 64;              // rows a split owns at least
constexpr int CS_TARGET_BLOCKS = 512;        // two workgroups per CU

struct PcaPlan { int tiles, ktiles, splits, per; };

// which = 0: project (M = N rows, N = l, K = D); 1: backproject (M = l, N = D, K = N rows)
PcaPlan pca_plan(long N, int D, int l, int which) {
    const long M = which ? l : N, Nc = which ? D : l, K = which ? N : D;
    PcaPlan p;
    p.tiles = cdiv(M, PCA_BM) * cdiv(Nc, PCA_BN);
    p.ktiles = cdiv(K, 32);
    int s = PCA_TARGET_BLOCKS / p.tiles;
    if (s > PCA_MAX_SPLITS) s = PCA_MAX_SPLITS;
    if (s > p.ktiles) s = p.ktiles;
    if (s < 1) s = 1;
    const Split ks = even_split(p.ktiles, s);  // every split owns at least one k-tile
    p.per = (int)ks.per;
    p.splits = ks.count;
    return p;
}

struct CsPlan { int col_blocks, splits; long rows_per; };
CsPlan cs_plan(long N, int D) {
    CsPlan p;
    p.col_blocks = cdiv(D, CS_COLS);
    long s = cdiv(CS_TARGET_BLOCKS, p.col_blocks);
    const long most = (N + CS_MIN_ROWS - 1) / CS_MIN_ROWS;
    if (s > most) s = most;
    if (s < 1) s = 1;
    const Split rows = even_split(N, s);
    p.rows_per = rows.per;
    p.splits = rows.count;
    return p;
}

// ---------------------------------------------------------------------------------------------- column statistics
// part[s][c] = sum over the rows of split s of x (SQ = false) or of (x - mean[c])^2 (SQ = true), in fp64: each of the 8
// row lanes walks its rows in ascending order into four interleaved accumulators (four loads in flight instead of one
// dependent chain), combined as (a0 + a1) + (a2 + a3); the lanes are added in lane order.  One fixed order.
template <bool SQ>
__global__ __launch_bounds__(CS_COLS* CS_LANES) void pca_colsum_kernel(const float* __restrict__ X, long ldx, long N, int D,
                                                                       long rows_per, const float* __restrict__ mean,
                                                                       double* __restrict__ part) {
    __shared__ double sh[CS_LANES][CS_COLS];
    const int c = blockIdx.x * CS_COLS + (threadIdx.x % CS_COLS);
    const int lane = threadIdx.x / CS_COLS;
    const long r0 = (long)blockIdx.y * rows_per;
    long r1 = r0 + rows_per;
    if (r1 > N) r1 = N;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (c < D) {
        const double mu = SQ ? (double)mean[c] : 0.0;
        long r = r0 + lane;
        for (; r + 3 * CS_LANES < r1; r += 4 * CS_LANES) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const double v = (double)X[(r + u * CS_LANES) * ldx + c] - mu;
                acc[u] += SQ ? v * v : v;
            }
        }
        for (int u = 0; r < r1; r += CS_LANES, ++u) {
            const double v = (double)X[r * ldx + c] - mu;
            acc[u] += SQ ? v * v : v;
        }
    }
    sh[lane][threadIdx.x % CS_COLS] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    __syncthreads();
    if (lane == 0 && c < D) {
        double t = sh[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < CS_LANES; ++w) t += sh[w][threadIdx.x];
        part[(long)blockIdx.y * D + c] = t;
    }
}

// the partials added in split order; mean: / N, rounded once to f32; var: / (N - 1), fp64
__global__ __launch_bounds__(256) void pca_colfinish_kernel(const double* __restrict__ part, int splits, int D, double div,
                                                            float* __restrict__ mean, double* __restrict__ var) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= D) return;
    double t = 0.0;
    for (int s = 0; s < splits; ++s) t += part[(long)s * D + c];
    t /= div;
    if (mean) mean[c] = (float)t;
    if (var) var[c] = t;
}

// ---------------------------------------------------------------------------------------------- the two contractions
// gemm_f32_kernel<NT ? (A_KC, B_KC) : (!A_KC, !B_KC), 1, 2, 4, 1, EPI_SLAB, FAST> with the centring step between the
// global load and the LDS store: its own are the mean's buffer resource, mean4, centre() in front of lstore, and k_loaded.  NT: A = X (rows = output rows, centred along k = the columns of X), B = the basis.
// TN: A = Y (k-strided; rows of Y are reduction indices), B = X (k-strided, centred along its columns = output columns).
template <bool NT, bool FAST>
__global__ __launch_bounds__(256) void pca_gemm_kernel(const GemmP g, const float* __restrict__ mean) {
    constexpr int BM = PCA_BM, BN = PCA_BN, WM = 1, WN = 2;
    constexpr int A_LDS = f32_tile_floats<NT, BM>();
    __shared__ __attribute__((aligned(16))) float lds[A_LDS + f32_tile_floats<NT, BN>()];
    float* As = lds;
    float* Bs = lds + A_LDS;

    const int t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wm0 = wave * (WM * 32);
    const int wn0 = 0;

    // gemm_f32_kernel's tile and split arithmetic, as text: behind a helper shared with it, every instantiation of both
    // kernels came out rescheduled (same length and registers), and these four are byte for byte their hand-written form
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
    for (int j = 0; j < WN; ++j)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[0][j][v] = 0.f;

    const F32Operand A = {g.A, g.lda, g.M, g.a_bytes, g.a_vec}, B = {g.B, g.ldb, g.N, g.b_bytes, g.b_vec};
    F32Stage<NT, NT, BM, BN, FAST> st;
    st.point(A, B);
    // the mean as a bounds-checked buffer of its own: a load at a column >= D returns the zero the centring needs there
    __amdgpu_buffer_rsrc_t rsM;
    if constexpr (FAST) {
        const int mcols = NT ? g.K : g.N;
        rsM = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(mean), 0, mean ? mcols * 4 : 0, 0x00020000);
    }
    st.rows_a(A, bm0, t);
    st.rows_b(B, bn0, t);
    // the four mean values this thread subtracts: columns c .. c + 3 of X, zero outside [0, D)
    auto mean4 = [&](int c, int ncols) {
        f32x4 m = {0.f, 0.f, 0.f, 0.f};
        if (!mean) return m;
        if constexpr (FAST) {
            m = bload4(rsM, c < ncols ? (unsigned)c << 2 : OOB);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (c + e < ncols) m[e] = mean[c + e];
        }
        return m;
    };
    f32x4 m4 = {0.f, 0.f, 0.f, 0.f};
    int k_loaded = 0;                        // first reduction index of the tile held in sa / sb
    if constexpr (!NT) m4 = mean4(bn0 + ((t % (BN / 4)) << 2), g.N);       // TN: the thread's columns never change

    auto gload = [&](int kt) {
        const int k0 = kt << 5;
        k_loaded = k0;
        st.gload(A, bm0, B, bn0, k0, g.K, t);                              // no reduction-row map: literal zeros
        if constexpr (NT) m4 = mean4(k0 + ((t & 7) << 2), g.K);            // NT: the thread's columns move with the k-tile
    };
    // Centring, between the global load and the LDS store.  Only elements whose ROW is inside the matrix are touched (m4 is
    // already zero at columns outside it): everything else was loaded as zero and stays zero.
    auto centre = [&]() {
        if constexpr (NT) {
#pragma unroll
            for (int p = 0; p < BM / 32; ++p)
                if (bm0 + p * 32 + (t >> 3) < g.M) st.sa.v[p] -= m4;
        } else {
            constexpr int TPR = BN / 4, KPP = 256 / TPR;
#pragma unroll
            for (int p = 0; p < BN / 32; ++p)
                if (k_loaded + p * KPP + t / TPR < g.K) st.sb.v[p] -= m4;
        }
    };
    auto lstore = [&]() {
        centre();
        st.lstore(As, Bs, t);
    };
    auto tile = [&]() { mfma_tile<NT, NT, BM, BN>(As, Bs, wm0, wn0, r, h, acc); };
    F32_KLOOP(false, kt_begin, kt_end, gload, lstore, tile);

    gemm_epilogue<WM, WN, EPI_SLAB>(g, acc, bm0 + wm0, bn0 + wn0, r, h, z);
}

// out[m * ldo + n] = (sum over the slabs, in split order, of slab[s][m * Nc + n]) * scale[n]
__global__ __launch_bounds__(256) void pca_reduce_kernel(const float* __restrict__ slabs, long stride, int nslabs, long M, int Nc,
                                                         const float* __restrict__ scale, float* __restrict__ out, long ldo) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= M * Nc) return;
    const long m = i / Nc;
    const int n = (int)(i - m * Nc);
    float t = slabs[i];
    for (int s = 1; s < nslabs; ++s) t += slabs[(long)s * stride + i];
    if (scale) t *= scale[n];
    out[m * ldo + n] = t;
}

// NT / TN launch over the slabs, then the reduction into out (row stride ldo)
int pca_contract(bool nt, GemmP g, const float* mean, const float* scale, float* out, long ldo, const PcaPlan& p,
                 float* slabs, hipStream_t stream) {
    g.a_vec = aligned16(g.A) && g.lda % 4 == 0;
    g.b_vec = aligned16(g.B) && g.ldb % 4 == 0;
    // 16-byte buffer loads: D % 4 == 0, pointers and strides 16-byte aligned, extents below 4 GB.  A float4 of the k-strided
    // Y (TN) straddles its last column when l % 4 != 0.  It stays inside the row pitch (ldy % 4 == 0) and, in the last row,
    // inside the aligned 16 bytes that hold the row's last element, so Y's extent is counted to the end of that float4;
    // what it reads past column l lands in tile rows >= l, which the epilogue never stores.
    const long a_rows = nt ? g.M : g.K, a_cols = nt ? g.K : (g.a_vec ? (g.M + 3L) / 4 * 4 : g.M);
    const long b_rows = nt ? g.N : g.K, b_cols = nt ? g.K : g.N;
    const long ab = operand_bytes(a_rows, g.lda, a_cols), bb = operand_bytes(b_rows, g.ldb, b_cols);
    const int xcols = nt ? g.K : g.N;                  // D: the width of X, whichever operand it is
    const bool fast = g.a_vec && g.b_vec && xcols % 4 == 0 && (!mean || aligned16(mean)) && ab < 0xFFFF0000L && bb < 0xFFFF0000L;
    g.a_bytes = (unsigned)ab; g.b_bytes = (unsigned)bb;
    g.n_major = bb > ab;
    g.ktiles_per_split = p.per;
    g.slab = slabs;
    g.slab_stride = (long)g.M * g.N;
    const dim3 grid(p.tiles * p.splits), block(256);
    if (nt) {
        if (fast) VSOM_LAUNCH((pca_gemm_kernel<true, true>), grid, block, 0, stream, g, mean);
        else VSOM_LAUNCH((pca_gemm_kernel<true, false>), grid, block, 0, stream, g, mean);
    } else {
        if (fast) VSOM_LAUNCH((pca_gemm_kernel<false, true>), grid, block, 0, stream, g, mean);
        else VSOM_LAUNCH((pca_gemm_kernel<false, false>), grid, block, 0, stream, g, mean);
    }
    const int rc = launch_status("pca_gemm_kernel");
    if (rc) return rc;
    const long n_out = (long)g.M * g.N;
    VSOM_LAUNCH(pca_reduce_kernel, dim3(cdiv(n_out, 256)), dim3(256), 0, stream, (const float*)slabs, g.slab_stride, p.splits,
                (long)g.M, g.N, scale, out, ldo);
    return launch_status("pca_reduce_kernel");
}

// ---------------------------------------------------------------------------------------------- Gram matrices
// A workgroup owns a 4 x 4 patch of G (and of H).  Thread t sums the products at d = t, t + 1024, ... in fp64, the 64 lanes
// of a wave are combined by a butterfly, the sixteen waves in wave order: one fixed order per entry, and G comes out
// symmetric bit for bit (the patch (j, i) adds the same products in the same order).
__global__ __launch_bounds__(GRAM_THREADS) void pca_gram_kernel(const float* __restrict__ Zt, long ldz, const float* __restrict__ B, long ldb,
                                                       int l, int D, double* __restrict__ G, double* __restrict__ H) {
    __shared__ double sh[GRAM_WAVES][32];
    const int i0 = blockIdx.y * 4, j0 = blockIdx.x * 4;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double g[4][4], hh[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) { g[a][b] = 0.0; hh[a][b] = 0.0; }
    for (int d = t; d < D; d += GRAM_THREADS) {
        double zi[4], zj[4], bi[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            zi[a] = i0 + a < l ? (double)Zt[(long)(i0 + a) * ldz + d] : 0.0;
            zj[a] = j0 + a < l ? (double)Zt[(long)(j0 + a) * ldz + d] : 0.0;
            bi[a] = (B && i0 + a < l) ? (double)B[(long)(i0 + a) * ldb + d] : 0.0;
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                g[a][b] = fma(zi[a], zj[b], g[a][b]);
                hh[a][b] = fma(bi[a], zj[b], hh[a][b]);
            }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            g[a][b] = wave_sum_f64(g[a][b]);
            hh[a][b] = wave_sum_f64(hh[a][b]);
            if (lane == 0) { sh[wave][a * 4 + b] = g[a][b]; sh[wave][16 + a * 4 + b] = hh[a][b]; }
        }
    __syncthreads();
    if (t < 32) {
        const int a = (t & 15) >> 2, b = t & 3;
        if (i0 + a < l && j0 + b < l) {
            double v = sh[0][t];
#pragma unroll
            for (int w = 1; w < GRAM_WAVES; ++w) v += sh[w][t];
            if (t < 16) G[(long)(i0 + a) * l + j0 + b] = v;
            else if (H) H[(long)(i0 + a) * l + j0 + b] = v;
        }
    }
}

// Bout[o][d] = sum_i T[o][i] Zt[i][d], i ascending, fp64, rounded once; a thread owns one column d and four rows o
__global__ __launch_bounds__(256) void pca_rotate_kernel(const double* __restrict__ T, int l_out, int l_in, const float* __restrict__ Zt,
                                                         long ldz, int D, float* __restrict__ Bout, long ldo) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    const int o0 = blockIdx.y * 4;
    if (d >= D) return;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < l_in; ++i) {
        const double z = (double)Zt[(long)i * ldz + d];
#pragma unroll
        for (int a = 0; a < 4; ++a)
            if (o0 + a < l_out) acc[a] = fma(T[(long)(o0 + a) * l_in + i], z, acc[a]);
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
        if (o0 + a < l_out) Bout[(long)(o0 + a) * ldo + d] = (float)acc[a];
}

// Xout[m][d] = fma chain over j ascending of (Y[m][j] scale[j]) B[j][d], then + mean[d]; four rows m per workgroup, their
// scaled coordinates in LDS; bound by the output store
__global__ __launch_bounds__(256) void pca_reconstruct_kernel(const float* __restrict__ Y, long ldy, long M, int l,
                                                              const float* __restrict__ scale, const float* __restrict__ B, long ldb,
                                                              int D, const float* __restrict__ mean, float* __restrict__ Xout, long ldo) {
    __shared__ float ys[4][PCA_MAX_L];
    const long m0 = (long)blockIdx.y * 4;
    for (int i = threadIdx.x; i < 4 * l; i += 256) {
        const int a = i / l, j = i - a * l;
        ys[a][j] = m0 + a < M ? Y[(m0 + a) * ldy + j] * (scale ? scale[j] : 1.0f) : 0.f;
    }
    __syncthreads();
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= D) return;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < l; ++j) {
        const float b = B[(long)j * ldb + d];
#pragma unroll
        for (int a = 0; a < 4; ++a) acc[a] = fmaf(ys[a][j], b, acc[a]);
    }
    const float mu = mean ? mean[d] : 0.f;
#pragma unroll
    for (int a = 0; a < 4; ++a)
        if (m0 + a < M) Xout[(m0 + a) * ldo + d] = acc[a] + mu;
}

constexpr long PCA_MAX_ROWS = 0x7fffffffL - 256;       // tile arithmetic is 32-bit

int check_shape(const char* who, long N, int D, int l) {
    VSOM_REQUIRE(N >= 1 && D >= 1 && l >= 1, VSOM_EINVAL, "%s: non-positive size N=%ld D=%d l=%d", who, N, D, l);
    VSOM_REQUIRE(l <= PCA_MAX_L, VSOM_EUNSUPPORTED, "%s: basis width l=%d > %d", who, l, PCA_MAX_L);
    VSOM_REQUIRE(l <= D, VSOM_EUNSUPPORTED, "%s: basis width l=%d > D=%d", who, l, D);
    VSOM_REQUIRE(N >= 2, VSOM_EUNSUPPORTED, "%s: N=%ld < 2 rows", who, N);
    VSOM_REQUIRE(N <= PCA_MAX_ROWS, VSOM_EUNSUPPORTED, "%s: N=%ld > %ld rows", who, N, PCA_MAX_ROWS);
    return VSOM_OK;
}

}  // namespace
}  // namespace vsom

using namespace vsom;

extern "C" {

long vsom_pca_colstats_parts(long N, int D) {
    if (N <= 0 || D <= 0) return 0;
    return (long)cs_plan(N, D).splits * D;
}

int vsom_pca_colstats(const float* X, long ldx, long N, int D, float* mean, double* var, double* part, long n_part,
                      vsom_stream_t stream) {
    VSOM_REQUIRE(X && mean && var, VSOM_EINVAL, "pca_colstats: null pointer");
    VSOM_REQUIRE(N >= 1 && D >= 1 && ldx >= D, VSOM_EINVAL, "pca_colstats: bad sizes N=%ld D=%d ldx=%ld", N, D, ldx);
    VSOM_REQUIRE(N >= 2, VSOM_EUNSUPPORTED, "pca_colstats: N=%ld < 2 rows (the variance divides by N - 1)", N);
    const long need = vsom_pca_colstats_parts(N, D);
    VSOM_REQUIRE(part && n_part >= need, VSOM_EWORKSPACE, "pca_colstats: partial buffer null or too small (%ld < %ld doubles)",
                 n_part, need);
    VSOM_REQUIRE(aligned16(part), VSOM_EALIGN, "pca_colstats: partial buffer not 16-byte aligned");
    const CsPlan p = cs_plan(N, D);
    const dim3 grid(p.col_blocks, p.splits), block(CS_COLS * CS_LANES);
    VSOM_LAUNCH((pca_colsum_kernel<false>), grid, block, 0, stream, X, ldx, N, D, p.rows_per, (const float*)nullptr, part);
    VSOM_LAUNCH(pca_colfinish_kernel, dim3(cdiv(D, 256)), dim3(256), 0, stream, (const double*)part, p.splits, D, (double)N, mean,
                (double*)nullptr);
    VSOM_LAUNCH((pca_colsum_kernel<true>), grid, block, 0, stream, X, ldx, N, D, p.rows_per, (const float*)mean, part);
    VSOM_LAUNCH(pca_colfinish_kernel, dim3(cdiv(D, 256)), dim3(256), 0, stream, (const double*)part, p.splits, D, (double)(N - 1),
                (float*)nullptr, var);
    return launch_status("pca_colstats");
}

long vsom_pca_slabs(long N, int D, int l, int which) {
    if (N <= 0 || D <= 0 || l <= 0 || N > PCA_MAX_ROWS || (which != 0 && which != 1)) return 0;
    const PcaPlan p = pca_plan(N, D, l, which);
    return (long)p.splits * (which ? (long)l * D : N * l);
}

int vsom_pca_project(const float* X, long ldx, long N, int D, const float* mean, const float* B, long ldb, int l,
                     const float* scale, float* Y, long ldy, float* slabs, long n_slabs, vsom_stream_t stream) {
    VSOM_REQUIRE(X && B && Y, VSOM_EINVAL, "pca_project: null pointer");
    if (int rc = check_shape("pca_project", N, D, l)) return rc;
    VSOM_REQUIRE(ldx >= D && ldb >= D && ldy >= l, VSOM_EINVAL, "pca_project: row stride below the row length (ldx=%ld ldb=%ld ldy=%ld)",
                 ldx, ldb, ldy);
    const long need = vsom_pca_slabs(N, D, l, 0);
    VSOM_REQUIRE(slabs && n_slabs >= need, VSOM_EWORKSPACE, "pca_project: slab buffer null or too small (%ld < %ld floats)", n_slabs, need);
    VSOM_REQUIRE(aligned16(slabs), VSOM_EALIGN, "pca_project: slab buffer not 16-byte aligned");
    GemmP g{};
    g.A = X; g.lda = ldx; g.B = B; g.ldb = ldb;
    g.M = (int)N; g.N = l; g.K = D;
    return pca_contract(true, g, mean, scale, Y, ldy, pca_plan(N, D, l, 0), slabs, stream);
}

int vsom_pca_backproject(const float* Y, long ldy, const float* X, long ldx, long N, int D, const float* mean, int l, float* Zt,
                         long ldz, float* slabs, long n_slabs, vsom_stream_t stream) {
    VSOM_REQUIRE(X && Y && Zt, VSOM_EINVAL, "pca_backproject: null pointer");
    if (int rc = check_shape("pca_backproject", N, D, l)) return rc;
    VSOM_REQUIRE(ldx >= D && ldy >= l && ldz >= D, VSOM_EINVAL, "pca_backproject: row stride below the row length (ldx=%ld ldy=%ld ldz=%ld)",
                 ldx, ldy, ldz);
    const long need = vsom_pca_slabs(N, D, l, 1);
    VSOM_REQUIRE(slabs && n_slabs >= need, VSOM_EWORKSPACE, "pca_backproject: slab buffer null or too small (%ld < %ld floats)", n_slabs,
                 need);
    VSOM_REQUIRE(aligned16(slabs), VSOM_EALIGN, "pca_backproject: slab buffer not 16-byte aligned");
    GemmP g{};
    g.A = Y; g.lda = ldy; g.B = X; g.ldb = ldx;
    g.M = l; g.N = D; g.K = (int)N;
    return pca_contract(false, g, mean, nullptr, Zt, ldz, pca_plan(N, D, l, 1), slabs, stream);
}

int vsom_pca_gram(const float* Zt, long ldz, const float* B, long ldb, int l, int D, double* G, double* H, vsom_stream_t stream) {
    VSOM_REQUIRE(Zt && G, VSOM_EINVAL, "pca_gram: null pointer");
    VSOM_REQUIRE((B == nullptr) == (H == nullptr), VSOM_EINVAL, "pca_gram: B and H go together");
    VSOM_REQUIRE(l >= 1 && D >= 1 && ldz >= D && (!B || ldb >= D), VSOM_EINVAL, "pca_gram: bad sizes l=%d D=%d ldz=%ld ldb=%ld", l, D, ldz, ldb);
    VSOM_REQUIRE(l <= PCA_MAX_L, VSOM_EUNSUPPORTED, "pca_gram: basis width l=%d > %d", l, PCA_MAX_L);
    const int nb = cdiv(l, 4);
    VSOM_LAUNCH(pca_gram_kernel, dim3(nb, nb), dim3(GRAM_THREADS), 0, stream, Zt, ldz, B, ldb, l, D, G, H);
    return launch_status("pca_gram_kernel");
}

int vsom_pca_rotate(const double* T, int l_out, int l_in, const float* Zt, long ldz, int D, float* Bout, long ldo,
                    vsom_stream_t stream) {
    VSOM_REQUIRE(T && Zt && Bout, VSOM_EINVAL, "pca_rotate: null pointer");
    VSOM_REQUIRE(l_out >= 1 && l_in >= 1 && D >= 1 && ldz >= D && ldo >= D, VSOM_EINVAL, "pca_rotate: bad sizes l_out=%d l_in=%d D=%d ldz=%ld ldo=%ld",
                 l_out, l_in, D, ldz, ldo);
    VSOM_REQUIRE(l_out <= PCA_MAX_L && l_in <= PCA_MAX_L, VSOM_EUNSUPPORTED, "pca_rotate: width %d x %d > %d", l_out, l_in, PCA_MAX_L);
    // the output rows are written while the input rows are still read by other workgroups
    const float* z_end = Zt + ((long)(l_in - 1) * ldz + D);
    const float* o_end = Bout + ((long)(l_out - 1) * ldo + D);
    VSOM_REQUIRE(o_end <= Zt || z_end <= Bout, VSOM_EINVAL, "pca_rotate: Bout overlaps Zt");
    VSOM_LAUNCH(pca_rotate_kernel, dim3(cdiv(D, 256), cdiv(l_out, 4)), dim3(256), 0, stream, T, l_out, l_in, Zt, ldz, D, Bout, ldo);
    return launch_status("pca_rotate_kernel");
}

int vsom_pca_reconstruct(const float* Y, long ldy, long M, int l, const float* scale, const float* B, long ldb, int D,
                         const float* mean, float* Xout, long ldo, vsom_stream_t stream) {
    VSOM_REQUIRE(Y && B && Xout, VSOM_EINVAL, "pca_reconstruct: null pointer");
    VSOM_REQUIRE(M >= 1 && l >= 1 && D >= 1 && ldy >= l && ldb >= D && ldo >= D, VSOM_EINVAL,
                 "pca_reconstruct: bad sizes M=%ld l=%d D=%d ldy=%ld ldb=%ld ldo=%ld", M, l, D, ldy, ldb, ldo);
    VSOM_REQUIRE(l <= PCA_MAX_L, VSOM_EUNSUPPORTED, "pca_reconstruct: width l=%d > %d", l, PCA_MAX_L);
    VSOM_REQUIRE(M <= 4L * 65535, VSOM_EUNSUPPORTED, "pca_reconstruct: M=%ld > %ld rows per call", M, 4L * 65535);
    VSOM_LAUNCH(pca_reconstruct_kernel, dim3(cdiv(D, 256), cdiv(M, 4)), dim3(256), 0, stream, Y, ldy, M, l, scale, B, ldb, D, mean, Xout, ldo);
    return launch_status("pca_reconstruct_kernel");
}

}  // extern "C"
