// Gaussian mixtures (diag / spherical covariances) for vit_som_amd/gmm.py: the steps of sklearn.mixture.GaussianMixture
// (_gaussian_mixture.py, _base.py) that touch the data, in the DIRECT form ("Gaussian mixtures").
//
//   vsom_gmm_estep        log p_ik = c_k - m_ik / 2 with m_ik = sum_d (x_id - mu_kd)^2 p_kd, the fp64 log-sum-exp over k,
//                         responsibilities, first-argmax labels, per-workgroup sums of log_prob_norm.
//   vsom_gmm_mstep        per-slab nk, S1 = sum_i r_ik (x_id - mu_old_kd), S2 = sum_i r_ik (x_id - mu_old_kd)^2 (fp64).
//   vsom_gmm_params       slabs added in slab order -> means, covariances, precisions, log constants, weights, status record.
//   vsom_gmm_set_params   the tail of vsom_gmm_params alone, from given weights and covariances.
//
// No floating-point atomics anywhere: every sum has one fixed order, so a fit is bitwise reproducible.
#include <float.h>

#include "row_tile.h"

namespace vsom {
namespace {

constexpr int GM_THREADS = 512;              // 8 waves
constexpr int GM_WAVES = GM_THREADS / 64;
constexpr int GM_RB = 4;                     // rows per wave, register-blocked: one LDS parameter read serves 4 rows
constexpr int GM_GROUP = GM_WAVES * GM_RB;   // 32 rows per workgroup step
constexpr int GM_KC = 8;                     // components per register chunk: 4 x 8 fp64 accumulators per lane
constexpr int GM_LDS = 128 * 1024;           // mean tile [KC][dt] + precision tile [KC][dt]; gfx950 has 160 KiB per CU
constexpr int GM_MAX_GROUPS = 256;           // one workgroup per CU
constexpr int GM_MAX_K = 1024;
constexpr size_t GM_SLAB_BUDGET = size_t(128) << 20;
constexpr int GM_MT = 256;                   // M-step and parameter kernels: threads per workgroup
constexpr int GM_MAX_SLABS = 256;
constexpr double GM_LOG_2PI = 1.8378770664093454835606594728112;

// ---- E-step split: a function of N alone
inline int gm_groups(long N) {
    const long need = (N + GM_GROUP - 1) / GM_GROUP;
    return (int)(need < GM_MAX_GROUPS ? need : GM_MAX_GROUPS);
}
inline long gm_estep_parts(long N, int K) { return (long)gm_groups(N) * (2 + (long)GM_GROUP * K); }

// ---- M-step split: row slabs, a function of the shape alone.  One slab holds [K][2][D] + [K] doubles; as many slabs as keep
// about 1024 workgroups in flight, fewer when they would pass 128 MiB (large K * D) or hold under 32 rows each.
inline Split gm_slabs(long N, int D, int K) {
    const size_t per = ((size_t)K * (2 * (size_t)D + 1)) * 8;
    long s = (long)(GM_SLAB_BUDGET / per);
    const long want = (1024 + cdiv(D, GM_MT) - 1) / cdiv(D, GM_MT);
    if (s > want) s = want;
    if (s > GM_MAX_SLABS) s = GM_MAX_SLABS;
    const long need = (N + 31) / 32;
    if (s > need) s = need;
    if (s < 1) s = 1;
    return even_split(N, s);                     // every slab holds rows
}
// scratch of the M-step and of the parameter pass: slabs S1 / S2 [S][K][2][D], nk [S][K], the diag covariances [K][D]
// (what spherical averages), per-component records [K][4]
inline long gm_mstep_parts(long N, int D, int K) {
    return (long)gm_slabs(N, D, K).count * K * (2 * (long)D + 1) + (long)K * D + (long)K * 4;
}
inline long gm_set_parts(int K) { return (long)K * 4; }

// a piece's Mahalanobis terms against planes (means, precisions): the sum over its columns of (x - mu)^2 p in f32, one f32
// chain (a segment of at most 4 columns), widened once for the fp64 sum over pieces
struct Maha {
    static constexpr int PLANES = 2;
    typedef double Acc;
    static __device__ __forceinline__ double term(f32x4 x, const f32x4 (&mp)[2]) {
        const f32x4 e = x - mp[0], pr = mp[1];
        float s = (e.x * e.x) * pr.x;
        s = fmaf(e.y * e.y, pr.y, s);
        s = fmaf(e.z * e.z, pr.z, s);
        return (double)fmaf(e.w * e.w, pr.w, s);
    }
    static __device__ __forceinline__ double term(float x, const float (&mp)[2]) {
        const float e = x - mp[0];
        return (double)((e * e) * mp[1]);
    }
};

struct EstepP {
    const float* X;
    long ldx, N;
    int D, K;
    const float* mu;      // [K][D]
    const float* prec;    // [K][D]
    const double* logc;   // [K]
    float* resp;          // [N][ldr] or null
    long ldr;
    double* lpn;          // [N]
    int64_t* labels;      // [N] or null
    double* part;         // [G] sums of lpn, [G] refused rows, [G][32][K] log p staging
    long rows_per_group;
    int dt, G;
};

// One workgroup's contiguous row range, 32 rows at a time.
//  (1) Mahalanobis terms: row_tile_pass (row_tile.h) with Maha, wave w on rows 4w..4w+3 of the step.  A piece's VEC terms
//      are added in f32 (a segment of at most 4 columns), the pieces of a lane in fp64 in column order, the 64 lanes by a
//      fp64 butterfly (the same value on every lane).  log p_ik = c_k - m_ik / 2 goes to the workgroup's staging rows.
//  (2) per row, by its wave: first argmax, max-shifted fp64 log-sum-exp (lane l takes k = l, l + 64, ..., then the
//      butterfly), resp = exp(log p - log_prob_norm) rounded once to f32.
template <int VEC>
__global__ __launch_bounds__(GM_THREADS) void gmm_estep_kernel(EstepP p) {
    constexpr int KC = GM_KC;
    extern __shared__ __attribute__((aligned(16))) float lds_g[];     // [KC][dt] means, [KC][dt] precisions
    __shared__ double s_sum[GM_WAVES];
    __shared__ int s_bad[GM_WAVES];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int D = p.D, K = p.K;
    const long r0 = (long)blockIdx.x * p.rows_per_group;
    const long r1 = min(p.N, r0 + p.rows_per_group);
    double* stage = p.part + 2 * (size_t)p.G + (size_t)blockIdx.x * GM_GROUP * K;
    const float* const planes[2] = {p.mu, p.prec};
    const int nchunks = (K + KC - 1) / KC;
    const bool resident = nchunks == 1 && D <= p.dt;                 // parameters staged once for the whole range
    double wsum = 0.0;
    int wbad = 0;

    for (long base = r0; base < r1; base += GM_GROUP) {
        const long rw = base + wave * GM_RB;
        for (int ch = 0; ch < nchunks; ++ch) {
            const int j0 = ch * KC, kc = min(KC, K - j0);
            double acc[GM_RB][KC];
#pragma unroll
            for (int r = 0; r < GM_RB; ++r)
#pragma unroll
                for (int j = 0; j < KC; ++j) acc[r][j] = 0.0;
            row_tile_pass<GM_THREADS, GM_RB, KC, VEC, Maha>(p.X, p.ldx, rw, r1, D, planes, j0, kc, lds_g, p.dt,
                                                            !resident || base == r0, acc);
#pragma unroll
            for (int r = 0; r < GM_RB; ++r)
#pragma unroll
                for (int j = 0; j < KC; ++j) {
                    const double s = wave_sum_f64(acc[r][j]);
                    if (lane == 0 && j < kc) stage[(size_t)(wave * GM_RB + r) * K + j0 + j] = p.logc[j0 + j] - 0.5 * s;
                }
        }
        __syncthreads();                                              // the staging rows are written
        for (int r = 0; r < GM_RB; ++r) {
            const long row = rw + r;
            if (row >= r1) break;                                     // wave-uniform
            const double* lp = stage + (size_t)(wave * GM_RB + r) * K;
            double m = -INFINITY;
            int bi = 0x7fffffff;
            for (int k = lane; k < K; k += 64) {
                const double v = lp[k];
                if (v > m) { m = v; bi = k; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double om = __shfl_xor(m, o, 64);
                const int ob = __shfl_xor(bi, o, 64);
                if (om > m || (om == m && ob < bi)) { m = om; bi = ob; }
            }
            double s = 0.0;
            for (int k = lane; k < K; k += 64) s += exp(lp[k] - m);
            s = wave_sum_f64(s);
            const double lse = m + log(s);
            const bool ok = isfinite(lse);
            if (p.resp)
                for (int k = lane; k < K; k += 64) p.resp[row * p.ldr + k] = ok ? (float)exp(lp[k] - lse) : NAN;
            if (lane == 0) {
                p.lpn[row] = ok ? lse : (double)NAN;
                if (p.labels) p.labels[row] = ok ? (int64_t)bi : (int64_t)-1;
            }
            if (ok) wsum += lse; else wbad += 1;
        }
        __syncthreads();                                              // before the next step overwrites the staging rows
    }
    if (lane == 0) { s_sum[wave] = wsum; s_bad[wave] = wbad; }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        int b = 0;
        for (int w = 0; w < GM_WAVES; ++w) { s += s_sum[w]; b += s_bad[w]; }
        p.part[blockIdx.x] = s;
        p.part[p.G + blockIdx.x] = (double)b;
    }
}

// estat[0] = sum_g part[g] in g order (the accepted rows' log_prob_norm), estat[1] = the refused rows
__global__ void gmm_estat_kernel(const double* __restrict__ part, int G, double* __restrict__ estat) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0, b = 0.0;
    for (int g = 0; g < G; ++g) { s += part[g]; b += part[G + g]; }
    estat[0] = s;
    estat[1] = b;
}

// M-step partials.  Workgroup (cb, s): columns 256 cb .. 256 cb + 255 (thread = column), the rows of slab s, the components
// in chunks of 8.  d = x - mu_old, r d and (r d) d are all fp64 (the difference and the first product are exact), summed
// in row order.  Workgroups with cb == 0 also sum nk (thread = component).
__global__ __launch_bounds__(GM_MT) void gmm_mstep_kernel(const float* __restrict__ X, long ldx, long N, int D, int K,
                                                          const float* __restrict__ resp, long ldr,
                                                          const float* __restrict__ mu_old, double* __restrict__ slabs,
                                                          double* __restrict__ nks, long rows_per_slab) {
    constexpr int KC = GM_KC;
    const int col = blockIdx.x * GM_MT + threadIdx.x, s = blockIdx.y;
    const long r0 = (long)s * rows_per_slab, r1 = min(N, r0 + rows_per_slab);
    const bool live = col < D;
    double* slab = slabs + (size_t)s * K * 2 * D;
    for (int k0 = 0; k0 < K; k0 += KC) {
        const int kc = min(KC, K - k0);
        double mu[KC], a1[KC], a2[KC];
#pragma unroll
        for (int j = 0; j < KC; ++j) {
            mu[j] = (live && j < kc) ? (double)mu_old[(size_t)(k0 + j) * D + col] : 0.0;
            a1[j] = 0.0; a2[j] = 0.0;
        }
#pragma unroll 4
        for (long i = r0; i < r1; ++i) {
            const double x = live ? (double)X[i * ldx + col] : 0.0;
            const float* ri = resp + i * ldr + k0;
#pragma unroll
            for (int j = 0; j < KC; ++j) {
                const float r = j < kc ? ri[j] : 0.f;
                const double dd = x - mu[j];
                const double rd = (double)r * dd;
                a1[j] += rd;
                a2[j] = fma(rd, dd, a2[j]);
            }
        }
        if (live) {
#pragma unroll
            for (int j = 0; j < KC; ++j)
                if (j < kc) {
                    slab[((size_t)(k0 + j) * 2) * D + col] = a1[j];
                    slab[((size_t)(k0 + j) * 2 + 1) * D + col] = a2[j];
                }
        }
    }
    if (blockIdx.x == 0)
        for (int k = threadIdx.x; k < K; k += GM_MT) {
            double n = 0.0;
            for (long i = r0; i < r1; ++i) n += (double)resp[i * ldr + k];
            nks[(size_t)s * K + k] = n;
        }
}

// sklearn _estimate_gaussian_parameters / _estimate_gaussian_covariances_diag about the shift mu_old, slabs in slab order:
//   nk = sum_s nk_s + 10 eps,  a = S1 / nk,  mean = mu_old + a,  cov = S2 / nk - a^2 + reg_covar
__global__ __launch_bounds__(GM_MT) void gmm_reduce_kernel(const double* __restrict__ slabs, const double* __restrict__ nks, int S,
                                                           int K, int D, const float* __restrict__ mu_old, double reg_covar,
                                                           float* __restrict__ means, double* __restrict__ covd,
                                                           double* __restrict__ kst) {
    const long kd = (long)K * D;
    for (long e = (long)blockIdx.x * GM_MT + threadIdx.x; e < kd; e += (long)gridDim.x * GM_MT) {
        const int k = (int)(e / D), d = (int)(e - (long)k * D);
        double nk = 0.0, s1 = 0.0, s2 = 0.0;
        for (int s = 0; s < S; ++s) {
            const double* slab = slabs + (size_t)s * K * 2 * D;
            nk += nks[(size_t)s * K + k];
            s1 += slab[((size_t)k * 2) * D + d];
            s2 += slab[((size_t)k * 2 + 1) * D + d];
        }
        nk += 10.0 * DBL_EPSILON;
        const double a = s1 / nk;
        means[e] = (float)((double)mu_old[e] + a);
        covd[e] = s2 / nk - a * a + reg_covar;
        if (d == 0) kst[(size_t)k * 4] = nk;
    }
}

// spherical: cov[k] = the fp64 mean of covd[k][:] in ascending d (tiles through LDS, thread 0 adds)
__global__ __launch_bounds__(GM_MT) void gmm_spherical_kernel(const double* __restrict__ covd, int D, double* __restrict__ cov) {
    __shared__ double tile[2048];
    __shared__ double s_acc;
    const double* row = covd + (size_t)blockIdx.x * D;
    if (threadIdx.x == 0) s_acc = 0.0;
    for (int d0 = 0; d0 < D; d0 += 2048) {
        const int dn = min(2048, D - d0);
        __syncthreads();
        for (int d = threadIdx.x; d < dn; d += GM_MT) tile[d] = row[d0 + d];
        __syncthreads();
        if (threadIdx.x == 0) {
            double s = s_acc;
            for (int d = 0; d < dn; ++d) s += tile[d];
            s_acc = s;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) cov[blockIdx.x] = s_acc / (double)D;
}

// per component: precisions (f32 [K][D], a spherical value repeated), kst[k][1..3] = (sum_d log p_kd / 2, the smallest
// covariance, the covariances that are <= 0 or not finite)
__global__ __launch_bounds__(GM_MT) void gmm_component_kernel(const double* __restrict__ cov, int D, int spherical,
                                                              float* __restrict__ prec, double* __restrict__ kst) {
    __shared__ double sh[GM_MT];
    const int k = blockIdx.x;
    double hl = 0.0, mn = INFINITY, bad = 0.0;
    if (spherical) {
        const double c = cov[k];
        const float q = (float)(1.0 / c);
        for (int d = threadIdx.x; d < D; d += GM_MT) prec[(size_t)k * D + d] = q;
        hl = 0.5 * (double)D * log(1.0 / c);
        mn = c;
        bad = (!(c > 0.0) || !isfinite(c)) ? 1.0 : 0.0;
    } else {
        for (int d = threadIdx.x; d < D; d += GM_MT) {
            const double c = cov[(size_t)k * D + d];
            prec[(size_t)k * D + d] = (float)(1.0 / c);
            const bool b = !(c > 0.0) || !isfinite(c);
            hl += b ? 0.0 : 0.5 * log(1.0 / c);
            mn = (c < mn || c != c) ? c : mn;
            bad += b ? 1.0 : 0.0;
        }
        hl = block_sum_f64<GM_MT>(hl, sh);
        mn = block_min_f64<GM_MT>(mn, sh);
        bad = block_sum_f64<GM_MT>(bad, sh);
    }
    if (threadIdx.x == 0) { kst[(size_t)k * 4 + 1] = hl; kst[(size_t)k * 4 + 2] = mn; kst[(size_t)k * 4 + 3] = bad; }
}

// one workgroup: weights (nk / n_norm, or nk / sum_k nk in ascending k when n_norm == 0, or the given ones), the log
// constants c_k = log w_k + sum_d log p_kd / 2 - D log(2 pi) / 2 and the status record
__global__ __launch_bounds__(GM_MT) void gmm_finish_kernel(const double* __restrict__ kst, int K, int D, long N, long n_norm,
                                                           const double* __restrict__ weights_in, const double* __restrict__ estat,
                                                           double* __restrict__ weights, double* __restrict__ logc,
                                                           double* __restrict__ record) {
    __shared__ double s_tot;
    if (threadIdx.x == 0) {
        double tot = (double)n_norm, mnk = INFINITY, mcov = INFINITY, bad = 0.0;
        if (!weights_in && n_norm == 0) {
            tot = 0.0;
            for (int k = 0; k < K; ++k) tot += kst[(size_t)k * 4];
        }
        for (int k = 0; k < K; ++k) {
            if (!weights_in) mnk = fmin(mnk, kst[(size_t)k * 4]);
            const double c = kst[(size_t)k * 4 + 2];
            mcov = (c < mcov || c != c) ? c : mcov;
            bad += kst[(size_t)k * 4 + 3];
        }
        s_tot = tot;
        record[0] = estat ? estat[0] / (double)N : (double)NAN;
        record[1] = weights_in ? (double)NAN : mnk;
        record[2] = mcov;
        record[3] = bad;
        record[4] = estat ? estat[1] : 0.0;
        record[5] = tot;
        record[6] = 0.0;
        record[7] = 0.0;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += GM_MT) {
        const double w = weights_in ? weights_in[k] : kst[(size_t)k * 4] / s_tot;
        if (!weights_in) weights[k] = w;
        logc[k] = log(w) + kst[(size_t)k * 4 + 1] - 0.5 * (double)D * GM_LOG_2PI;
    }
}

template <int VEC>
int launch_estep(const EstepP& p, hipStream_t stream) {
    return row_tile_launch<EstepP, gmm_estep_kernel<VEC>>(p, p.G, GM_THREADS, (size_t)2 * GM_KC * p.dt * 4, GM_LDS,
                                                          "gmm_estep_kernel", stream);
}

int launch_tail(const double* cov, int D, int K, long N, long n_norm, int spherical, const double* weights_in, const double* estat,
                float* prec, double* weights, double* logc, double* record, double* kst, hipStream_t stream) {
    VSOM_LAUNCH(gmm_component_kernel, dim3(K), dim3(GM_MT), 0, stream, cov, D, spherical, prec, kst);
    VSOM_LAUNCH(gmm_finish_kernel, dim3(1), dim3(GM_MT), 0, stream, (const double*)kst, K, D, N, n_norm, weights_in, estat, weights,
                logc, record);
    return launch_status("gmm_params");
}

}  // namespace
}  // namespace vsom

extern "C" {

long vsom_gmm_parts(long N, int D, int K, int which) {
    using namespace vsom;
    if (N < 1 || D < 1 || K < 1 || K > GM_MAX_K) return 0;
    switch (which) {
        case VSOM_GMM_ESTEP: return gm_estep_parts(N, K);
        case VSOM_GMM_MSTEP: return gm_mstep_parts(N, D, K);
        case VSOM_GMM_SET: return gm_set_parts(K);
        default: return 0;
    }
}

long vsom_gmm_slab_rows(long N, int D, int K) {
    using namespace vsom;
    if (N < 1 || D < 1 || K < 1 || K > GM_MAX_K) return 0;
    return gm_slabs(N, D, K).per;
}

int vsom_gmm_estep(const float* X, long ldx, long N, int D, const float* means, const float* prec, const double* logc, int K,
                   float* resp, long ldr, double* log_prob_norm, int64_t* labels, double* estat, double* part, long n_part,
                   vsom_stream_t stream) {
    using namespace vsom;
    VSOM_REQUIRE(X && means && prec && logc && log_prob_norm && estat, VSOM_EINVAL, "gmm_estep: null pointer");
    VSOM_REQUIRE(N >= 1 && D >= 1 && K >= 1 && ldx >= D && (!resp || ldr >= K), VSOM_EINVAL,
                 "gmm_estep: bad sizes N=%ld D=%d K=%d ldx=%ld ldr=%ld", N, D, K, ldx, ldr);
    VSOM_REQUIRE(K <= GM_MAX_K, VSOM_EUNSUPPORTED, "gmm_estep: K=%d > %d", K, GM_MAX_K);
    VSOM_REQUIRE(part && n_part >= gm_estep_parts(N, K), VSOM_EWORKSPACE, "gmm_estep: part holds %ld doubles < %ld (too small)",
                 part ? n_part : 0L, gm_estep_parts(N, K));
    EstepP p = {};
    p.X = X; p.ldx = ldx; p.N = N; p.D = D; p.K = K; p.mu = means; p.prec = prec; p.logc = logc;
    p.resp = resp; p.ldr = ldr; p.lpn = log_prob_norm; p.labels = labels; p.part = part;
    const Split rows = even_split(N, gm_groups(N));
    p.rows_per_group = rows.per;
    p.G = rows.count;                             // every workgroup gets rows; at most gm_groups(N), so the staging rows fit
    const bool vec = D % 4 == 0 && ldx % 4 == 0 && aligned16(X) && aligned16(means) && aligned16(prec);
    p.dt = row_tile_width(GM_LDS, Maha::PLANES, GM_KC, vec ? 4 : 1, D);
    const int rc = vec ? launch_estep<4>(p, stream) : launch_estep<1>(p, stream);
    if (rc != VSOM_OK) return rc;
    VSOM_LAUNCH(gmm_estat_kernel, dim3(1), dim3(64), 0, stream, (const double*)part, p.G, estat);
    return launch_status("gmm_estat_kernel");
}

int vsom_gmm_mstep(const float* X, long ldx, long N, int D, const float* resp, long ldr, const float* means_old, int K,
                   double* part, long n_part, vsom_stream_t stream) {
    using namespace vsom;
    VSOM_REQUIRE(X && resp && means_old, VSOM_EINVAL, "gmm_mstep: null pointer");
    VSOM_REQUIRE(N >= 1 && D >= 1 && K >= 1 && ldx >= D && ldr >= K, VSOM_EINVAL,
                 "gmm_mstep: bad sizes N=%ld D=%d K=%d ldx=%ld ldr=%ld", N, D, K, ldx, ldr);
    VSOM_REQUIRE(K <= GM_MAX_K, VSOM_EUNSUPPORTED, "gmm_mstep: K=%d > %d", K, GM_MAX_K);
    VSOM_REQUIRE(part && n_part >= gm_mstep_parts(N, D, K), VSOM_EWORKSPACE, "gmm_mstep: part holds %ld doubles < %ld (too small)",
                 part ? n_part : 0L, gm_mstep_parts(N, D, K));
    const Split slabs = gm_slabs(N, D, K);
    double* nks = part + (size_t)slabs.count * K * 2 * D;
    VSOM_LAUNCH(gmm_mstep_kernel, dim3(cdiv(D, GM_MT), slabs.count), dim3(GM_MT), 0, stream, X, ldx, N, D, K, resp, ldr, means_old,
                part, nks, slabs.per);
    return launch_status("gmm_mstep_kernel");
}

int vsom_gmm_params(double* part, long n_part, long N, int D, int K, const float* means_old, double reg_covar, int spherical,
                    long n_norm, const double* estat, float* means, double* cov, float* prec, double* weights, double* logc,
                    double* record, vsom_stream_t stream) {
    using namespace vsom;
    VSOM_REQUIRE(means_old && means && cov && prec && weights && logc && record, VSOM_EINVAL, "gmm_params: null pointer");
    VSOM_REQUIRE(N >= 1 && D >= 1 && K >= 1 && n_norm >= 0, VSOM_EINVAL, "gmm_params: bad sizes N=%ld D=%d K=%d", N, D, K);
    VSOM_REQUIRE(K <= GM_MAX_K, VSOM_EUNSUPPORTED, "gmm_params: K=%d > %d", K, GM_MAX_K);
    VSOM_REQUIRE(means_old != means, VSOM_EINVAL, "gmm_params: means must not alias means_old");
    VSOM_REQUIRE(part && n_part >= gm_mstep_parts(N, D, K), VSOM_EWORKSPACE, "gmm_params: part holds %ld doubles < %ld (too small)",
                 part ? n_part : 0L, gm_mstep_parts(N, D, K));
    const int S = gm_slabs(N, D, K).count;
    const double* nks = part + (size_t)S * K * 2 * D;
    double* covd_scratch = part + (size_t)S * K * (2 * (size_t)D + 1);
    double* kst = covd_scratch + (size_t)K * D;
    double* covd = spherical ? covd_scratch : cov;                    // diag: the reduced covariances are the output
    int blocks = cdiv((long)K * D, GM_MT);
    if (blocks > 4096) blocks = 4096;
    VSOM_LAUNCH(gmm_reduce_kernel, dim3(blocks), dim3(GM_MT), 0, stream, (const double*)part, nks, S, K, D, means_old, reg_covar, means, covd, kst);
    if (spherical) VSOM_LAUNCH(gmm_spherical_kernel, dim3(K), dim3(GM_MT), 0, stream, (const double*)covd, D, cov);
    return launch_tail(cov, D, K, N, n_norm, spherical, nullptr, estat, prec, weights, logc, record, kst, stream);
}

int vsom_gmm_set_params(const double* weights, const double* cov, int D, int K, int spherical, float* prec, double* logc,
                        double* record, double* part, long n_part, vsom_stream_t stream) {
    using namespace vsom;
    VSOM_REQUIRE(weights && cov && prec && logc && record, VSOM_EINVAL, "gmm_set_params: null pointer");
    VSOM_REQUIRE(D >= 1 && K >= 1, VSOM_EINVAL, "gmm_set_params: bad sizes D=%d K=%d", D, K);
    VSOM_REQUIRE(K <= GM_MAX_K, VSOM_EUNSUPPORTED, "gmm_set_params: K=%d > %d", K, GM_MAX_K);
    VSOM_REQUIRE(part && n_part >= gm_set_parts(K), VSOM_EWORKSPACE, "gmm_set_params: part holds %ld doubles < %ld (too small)",
                 part ? n_part : 0L, gm_set_parts(K));
    return launch_tail(cov, D, K, 1, 0, spherical, weights, nullptr, prec, nullptr, logc, record, part, stream);
}

}  // extern "C"
