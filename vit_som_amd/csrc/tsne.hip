// t-SNE (van der Maaten & Hinton 2008) with scikit-learn's TSNE surface and an EXACT repulsion (vit_som_amd/tsne.py states
// the whole algorithm step by step; DESIGN.md section 4 has the error bounds).
//
//   vsom_tsne_affinities   the conditional P of every row from its neighbour distances: sklearn's _binary_search_perplexity
//                          in fp64, one thread per row, rule for rule.
//   vsom_tsne_repulsion    the hot kernel: for every row the all-pairs sums  sum_j q^2 (y_i - y_j)  and  sum_j q,
//                          q = 1 / (1 + |y_i - y_j|^2), tiled through LDS, and the per-row-block sums of q that make up Z.
//   vsom_tsne_step         one iteration from those sums: attraction over the CSR joint P, gradient, gains, momentum, move,
//                          and on request the KL / gradient-norm partials.
//
// An iteration is these last two launches.  No floating-point atomics anywhere and every sum has one fixed order: a fit
// is bitwise reproducible.
#include "common.h"

#include <math.h>

namespace vsom {
namespace {

// ---------------------------------------------------------------- affinities
constexpr int AFF_THREADS = 64;
constexpr int AFF_MAX_K = 63;               // the neighbour search holds 64 entries, the row itself included

struct AffP {
    const float* dist;          // [N][ldk]
    const int64_t* idx;         // [N][ldk] or null
    long ldk, N;
    int k, first, square;
    double log_perplexity;
    double* P;                  // [N][k]
    double* beta;               // [N]
    int* status;
};

// sklearn/manifold/_utils.pyx: both constants are C floats there, promoted to double where they are used.
constexpr float AFF_EPSILON = 1e-8f;
constexpr float AFF_TOLERANCE = 1e-5f;
constexpr int AFF_STEPS = 100;

// One row per thread.  The row's k distances (f32 values, exact) and its k current exponentials live in LDS, [j][thread]
// so that the 64 threads of the wave touch 64 neighbouring words.  No contraction: the sums are the plain sums of the
// scalar loop this restates.
__global__ __launch_bounds__(AFF_THREADS) void tsne_affinities_kernel(const AffP p) {
#pragma clang fp contract(off)
    __shared__ float d[AFF_MAX_K * AFF_THREADS];
    __shared__ double e[AFF_MAX_K * AFF_THREADS];
    const int tid = threadIdx.x;
    const long i = (long)blockIdx.x * AFF_THREADS + tid;
    if (i >= p.N) return;                                   // no barrier below: every thread works on its own LDS column
    const int k = p.k;
    bool bad = false;
    for (int j = 0; j < k; ++j) {
        const float v = p.dist[i * p.ldk + p.first + j];
        const float s = p.square ? v * v : v;
        if (!(v >= 0.f) || !(s < INFINITY)) bad = true;     // NaN, negative, infinite, or a square that overflows
        if (p.idx && p.idx[i * p.ldk + p.first + j] < 0) bad = true;
        d[j * AFF_THREADS + tid] = s;
    }
    if (bad) {
        atomicAdd(p.status, 1);
        return;
    }
    double beta = 1.0, beta_min = -INFINITY, beta_max = INFINITY, sum_p = 0.0;
    for (int l = 0; l < AFF_STEPS; ++l) {
        sum_p = 0.0;
        for (int j = 0; j < k; ++j) {
            const double v = exp((double)(-d[j * AFF_THREADS + tid]) * beta);
            e[j * AFF_THREADS + tid] = v;
            sum_p += v;
        }
        if (sum_p == 0.0) sum_p = (double)AFF_EPSILON;
        double sum_dp = 0.0;
        for (int j = 0; j < k; ++j) sum_dp += (double)d[j * AFF_THREADS + tid] * (e[j * AFF_THREADS + tid] / sum_p);
        const double diff = (log(sum_p) + beta * sum_dp) - p.log_perplexity;
        if (fabs(diff) <= (double)AFF_TOLERANCE || l == AFF_STEPS - 1) break;   // P and beta go together: the last evaluated
        if (diff > 0.0) {
            beta_min = beta;
            beta = (beta_max == INFINITY) ? beta * 2.0 : (beta + beta_max) / 2.0;
        } else {
            beta_max = beta;
            beta = (beta_min == -INFINITY) ? beta / 2.0 : (beta + beta_min) / 2.0;
        }
    }
    for (int j = 0; j < k; ++j) p.P[i * k + j] = e[j * AFF_THREADS + tid] / sum_p;
    p.beta[i] = beta;
}

// ---------------------------------------------------------------- repulsion
constexpr int REP_ROWS = 64;                // rows of a workgroup: one per lane
constexpr int REP_WAVES = 16;               // column groups of a workgroup: one per wave
constexpr int REP_THREADS = REP_ROWS * REP_WAVES;
constexpr int REP_CHUNK = 64;               // columns whose terms are added in f32 before the sum moves to fp64
constexpr int REP_TILE = REP_WAVES * REP_CHUNK;

// The terms of one chunk of 64 columns for the lane's row, added in f32 in ascending column order.  Every lane reads the
// same column: the LDS reads are broadcasts.  CHECKED: the chunk holds the diagonal or runs past N; the pair (i, i) is
// excluded by index and a column past N adds nothing.  v_rcp_f32 (1 ulp).
template <bool CHECKED>
__device__ __forceinline__ void rep_chunk(const float2* cols, float yx, float yy, long i, long c0, long N, float& fx, float& fy,
                                          float& sq) {
#pragma unroll 8
    for (int jj = 0; jj < REP_CHUNK; ++jj) {
        const float2 yj = cols[jj];
        const float dx = yx - yj.x, dy = yy - yj.y;
        float q = __builtin_amdgcn_rcpf(1.f + fmaf(dx, dx, dy * dy));
        if (CHECKED) {
            const long j = c0 + jj;
            if (j == i || j >= N) q = 0.f;
        }
        const float q2 = q * q;
        sq += q;
        fx = fmaf(q2, dx, fx);
        fy = fmaf(q2, dy, fy);
    }
}

// Workgroup b owns rows [64 b, 64 b + 64), lane = row; its 16 waves share the columns: of every tile of 1024 columns
// staged in LDS, wave w takes chunk w.  A chunk's sums run in f32, a wave adds its chunks in fp64 in ascending order, and
// wave 0 adds the 16 waves' sums in ascending wave order.  zpart[b] = the fp64 sum of the block's 64 row sums of q in
// ascending row order.  The tile is double-buffered, so one barrier a tile is enough: a wave that stores tile t + 1 has
// passed the barrier of tile t, which every wave reaches only after it has finished reading tile t - 1.
__global__ __launch_bounds__(REP_THREADS) void tsne_repulsion_kernel(const float* Y, long N, double* rep, double* sumq,
                                                                      double* zpart) {
    __shared__ float2 tile[2][REP_TILE];
    __shared__ double red[REP_WAVES][3][REP_ROWS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long row0 = (long)blockIdx.x * REP_ROWS, i = row0 + lane;
    const bool valid = i < N;
    const float2* Y2 = reinterpret_cast<const float2*>(Y);
    const float2 zero = make_float2(0.f, 0.f);
    const float2 yi = valid ? Y2[i] : zero;
    double FX = 0.0, FY = 0.0, SQ = 0.0;
    const long ntiles = (N + REP_TILE - 1) / REP_TILE;
    float2 nxt = tid < N ? Y2[tid] : zero;
    for (long t = 0; t < ntiles; ++t) {
        tile[t & 1][tid] = nxt;
        const long col = (t + 1) * REP_TILE + tid;
        nxt = col < N ? Y2[col] : zero;                      // past the last tile: col >= N
        __syncthreads();
        const long c0 = t * REP_TILE + (long)w * REP_CHUNK;
        if (c0 < N) {
            float fx = 0.f, fy = 0.f, sq = 0.f;
            const float2* cols = &tile[t & 1][w * REP_CHUNK];
            if (c0 == row0 || c0 + REP_CHUNK > N) rep_chunk<true>(cols, yi.x, yi.y, i, c0, N, fx, fy, sq);
            else rep_chunk<false>(cols, yi.x, yi.y, i, c0, N, fx, fy, sq);
            FX += (double)fx;
            FY += (double)fy;
            SQ += (double)sq;
        }
    }
    red[w][0][lane] = FX;
    red[w][1][lane] = FY;
    red[w][2][lane] = SQ;
    __syncthreads();
    if (w == 0) {
        double s[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            s[c] = red[0][c][lane];
            for (int v = 1; v < REP_WAVES; ++v) s[c] += red[v][c][lane];
        }
        if (valid) {
            rep[2 * i] = s[0];
            rep[2 * i + 1] = s[1];
            sumq[i] = s[2];
        }
        red[0][2][lane] = valid ? s[2] : 0.0;
    }
    __syncthreads();
    if (tid == 0) {
        double z = 0.0;
        for (int l = 0; l < REP_ROWS; ++l) z += red[0][2][l];
        zpart[blockIdx.x] = z;
    }
}

// ---------------------------------------------------------------- step
constexpr int STEP_THREADS = 256;
constexpr int STEP_LANES = 16;              // lanes that share one row's edges
constexpr int STEP_ROWS = STEP_THREADS / STEP_LANES;
constexpr double MACHINE_EPSILON = 2.220446049250313e-16;       // sklearn's clamp inside the KL's logarithm

struct StepP {
    const int64_t* indptr;      // [N + 1]
    const int64_t* indices;     // [nnz]
    const double* data;         // [nnz] joint P, unexaggerated
    const float* Yin;           // [N][2]
    float* Yout;
    float* update;              // [N][2] in / out
    float* gains;               // [N][2] in / out
    const double* rep;          // [N][2]
    const double* zpart;
    double* part;               // [2 blocks]: KL, |grad|^2
    long N, n_z;
    double exaggeration, momentum, lr;
    int record;
};

__device__ __forceinline__ double group_sum_f64(double v) {        // over the 16 lanes of a row: a fixed butterfly
#pragma unroll
    for (int o = STEP_LANES / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, STEP_LANES);
    return v;
}

// Z first, the same bits in every workgroup: lane l of wave 0 adds segment l of zpart in ascending order, thread 0 adds the
// 64 segment sums in ascending order.  Then 16 lanes a row: lane l takes the row's edges l, l + 16, ... in fp64 (the
// differences of two f32 are exact there), the 16 sums meet in a butterfly, and lane 0 makes the move.
__global__ __launch_bounds__(STEP_THREADS) void tsne_step_kernel(const StepP p) {
#pragma clang fp contract(off)
    __shared__ double zs[64];
    __shared__ double Zsh;
    __shared__ double rec[2][STEP_ROWS];
    const int tid = threadIdx.x;
    if (tid < 64) {
        const long seg = (p.n_z + 63) / 64;
        const long b = (long)tid * seg, e = b + seg < p.n_z ? b + seg : p.n_z;
        double s = 0.0;
        for (long c = b; c < e; ++c) s += p.zpart[c];
        zs[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        double z = 0.0;
        for (int l = 0; l < 64; ++l) z += zs[l];
        Zsh = z;
    }
    __syncthreads();
    const double Z = Zsh;
    const int g = tid / STEP_LANES, l = tid % STEP_LANES;
    const long r = (long)blockIdx.x * STEP_ROWS + g;
    const bool valid = r < p.N;
    double ax = 0.0, ay = 0.0, kl = 0.0;
    float yx = 0.f, yy = 0.f;
    if (valid) {
        yx = p.Yin[2 * r];
        yy = p.Yin[2 * r + 1];
        const long e1 = p.indptr[r + 1];
        for (long e = p.indptr[r] + l; e < e1; e += STEP_LANES) {
            const long j = p.indices[e];
            if (j < 0 || j >= p.N) continue;                 // never dereferenced; the host builds the graph
            const double pe = p.exaggeration * p.data[e];
            const double dx = (double)yx - (double)p.Yin[2 * j], dy = (double)yy - (double)p.Yin[2 * j + 1];
            const double q = 1.0 / (1.0 + (dx * dx + dy * dy));
            const double pq = pe * q;
            ax += pq * dx;
            ay += pq * dy;
            if (p.record) kl += pe * log(fmax(pe, MACHINE_EPSILON) / fmax(q / Z, MACHINE_EPSILON));
        }
    }
    ax = group_sum_f64(ax);
    ay = group_sum_f64(ay);
    if (p.record) kl = group_sum_f64(kl);
    double g2 = 0.0;
    if (valid && l == 0) {
        const double grad[2] = {4.0 * (ax - p.rep[2 * r] / Z), 4.0 * (ay - p.rep[2 * r + 1] / Z)};
        const float y[2] = {yx, yy};
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const float u = p.update[2 * r + c];
            float gn = p.gains[2 * r + c];
            gn = ((double)u * grad[c] < 0.0) ? gn + 0.2f : gn * 0.8f;
            gn = fmaxf(gn, 0.01f);
            const float un = (float)(p.momentum * (double)u - (p.lr * (double)gn) * grad[c]);
            p.gains[2 * r + c] = gn;
            p.update[2 * r + c] = un;
            p.Yout[2 * r + c] = y[c] + un;
            g2 += grad[c] * grad[c];
        }
    }
    if (!p.record) return;
    if (l == 0) {
        rec[0][g] = valid ? kl : 0.0;
        rec[1][g] = g2;
    }
    __syncthreads();
    if (tid == 0) {
        double a = 0.0, b = 0.0;
        for (int v = 0; v < STEP_ROWS; ++v) { a += rec[0][v]; b += rec[1][v]; }
        p.part[2 * (long)blockIdx.x] = a;
        p.part[2 * (long)blockIdx.x + 1] = b;
    }
}

}  // namespace
}  // namespace vsom

extern "C" {

int vsom_tsne_affinities(const float* knn_dist, const int64_t* knn_idx, long ldk, long N, int k_eff, int first, int square,
                         double perplexity, double* P, double* beta, int32_t* status, vsom_stream_t stream) {
    using namespace vsom;
    VSOM_REQUIRE(knn_dist && P && beta && status, VSOM_EINVAL, "tsne_affinities: null pointer");
    VSOM_REQUIRE(N >= 1 && N <= 0x7fffffffL - AFF_THREADS && first >= 0 && k_eff >= 1 && ldk >= (long)first + k_eff, VSOM_EINVAL,
                 "tsne_affinities: bad sizes N=%ld k_eff=%d first=%d ldk=%ld", N, k_eff, first, ldk);
    VSOM_REQUIRE(k_eff <= AFF_MAX_K, VSOM_EUNSUPPORTED, "tsne_affinities: k_eff=%d > %d", k_eff, AFF_MAX_K);
    VSOM_REQUIRE(perplexity > 0.0 && perplexity < INFINITY, VSOM_EINVAL, "tsne_affinities: perplexity=%g", perplexity);
    AffP p = {};
    p.dist = knn_dist; p.idx = knn_idx; p.ldk = ldk; p.N = N; p.k = k_eff; p.first = first; p.square = square != 0;
    p.log_perplexity = log((double)(float)perplexity);      // sklearn takes the perplexity as a C float
    p.P = P; p.beta = beta; p.status = status;
    VSOM_LAUNCH(tsne_affinities_kernel, dim3(cdiv(N, AFF_THREADS)), dim3(AFF_THREADS), 0, stream, p);
    return launch_status("tsne_affinities");
}

long vsom_tsne_repulsion_parts(long N) {
    if (N < 1) return 0;
    return (N + vsom::REP_ROWS - 1) / vsom::REP_ROWS;
}

int vsom_tsne_repulsion(const float* Y, long N, double* rep, double* sumq, double* zpart, long n_zpart, vsom_stream_t stream) {
    using namespace vsom;
    VSOM_REQUIRE(Y && rep && sumq, VSOM_EINVAL, "tsne_repulsion: null pointer");
    VSOM_REQUIRE(N >= 1, VSOM_EINVAL, "tsne_repulsion: bad size N=%ld", N);
    VSOM_REQUIRE(N < 0x7fffffffL, VSOM_EUNSUPPORTED, "tsne_repulsion: N=%ld >= 2^31 - 1", N);
    VSOM_REQUIRE(aligned16(Y), VSOM_EALIGN, "tsne_repulsion: Y must be 16-byte aligned");
    VSOM_REQUIRE(zpart && n_zpart >= vsom_tsne_repulsion_parts(N), VSOM_EWORKSPACE,
                 "tsne_repulsion: zpart of %ld doubles is too small, < %ld (or null)", n_zpart, vsom_tsne_repulsion_parts(N));
    VSOM_LAUNCH(tsne_repulsion_kernel, dim3((unsigned)vsom_tsne_repulsion_parts(N)), dim3(REP_THREADS), 0, stream, Y, N, rep, sumq,
                zpart);
    return launch_status("tsne_repulsion");
}

long vsom_tsne_step_parts(long N) {
    if (N < 1) return 0;
    return 2 * ((N + vsom::STEP_ROWS - 1) / vsom::STEP_ROWS);
}

int vsom_tsne_step(const int64_t* indptr, const int64_t* indices, const double* data, const float* Y_in, float* Y_out,
                   float* update, float* gains, long N, const double* rep, const double* zpart, long n_zpart, double exaggeration,
                   double momentum, double learning_rate, int record, double* part, long n_part, vsom_stream_t stream) {
    using namespace vsom;
    VSOM_REQUIRE(indptr && indices && data && Y_in && Y_out && update && gains && rep, VSOM_EINVAL, "tsne_step: null pointer");
    VSOM_REQUIRE(N >= 1, VSOM_EINVAL, "tsne_step: bad size N=%ld", N);
    VSOM_REQUIRE(N < 0x7fffffffL, VSOM_EUNSUPPORTED, "tsne_step: N=%ld >= 2^31 - 1", N);
    VSOM_REQUIRE(Y_in != Y_out, VSOM_EINVAL, "tsne_step: Y_out must not alias Y_in");
    VSOM_REQUIRE(zpart && n_zpart >= vsom_tsne_repulsion_parts(N), VSOM_EWORKSPACE,
                 "tsne_step: zpart of %ld doubles is too small, < %ld (or null)", n_zpart, vsom_tsne_repulsion_parts(N));
    VSOM_REQUIRE(part && n_part >= vsom_tsne_step_parts(N), VSOM_EWORKSPACE,
                 "tsne_step: part of %ld doubles is too small, < %ld (or null)", n_part, vsom_tsne_step_parts(N));
    StepP p = {};
    p.indptr = indptr; p.indices = indices; p.data = data; p.Yin = Y_in; p.Yout = Y_out; p.update = update; p.gains = gains;
    p.rep = rep; p.zpart = zpart; p.part = part; p.N = N; p.n_z = vsom_tsne_repulsion_parts(N);
    p.exaggeration = exaggeration; p.momentum = momentum; p.lr = learning_rate; p.record = record != 0;
    VSOM_LAUNCH(tsne_step_kernel, dim3((unsigned)(vsom_tsne_step_parts(N) / 2)), dim3(STEP_THREADS), 0, stream, p);
    return launch_status("tsne_step");
}

}  // extern "C"
