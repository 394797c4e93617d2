// UMAP for visualize_umap_progression (tools/evaluation.py:267-323): the step of umap-learn's fit that runs once per
// epoch (vit_som_amd/umap.py states the whole algorithm step by step).  The other step that touches the data, the
// exact kNN graph (vsom_umap_knn), is the self mode of the search in knn.hip.
//
//   vsom_umap_epoch        one synchronous epoch of optimize_layout_euclidean: one thread per vertex, walking its CSR row.
//   vsom_umap_neg_sample   the negative-sample hash the epoch evaluates, for the host.
//   vsom_umap_transform_layout   transform(): every epoch of every new point in one launch, one thread per point, against
//                          the fixed training embedding (move_other=False), each term applied at once.
//
// No floating-point atomics anywhere and every sum has one fixed order: a fit and a transform are bitwise reproducible.
#include "common.h"

namespace vsom {
namespace {

constexpr int EPOCH_THREADS = 256;

// The negative-sample hash (include/vitsom_hip.h): two splitmix64 rounds over (seed, edge) and (epoch, p).
__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ uint64_t umap_neg_hash(uint64_t seed, int epoch, long edge, long p) {
    return splitmix64(splitmix64(seed ^ (uint64_t)edge) ^ (((uint64_t)(uint32_t)epoch << 32) | (uint64_t)(uint32_t)p));
}

// ---------------------------------------------------------------- layout epoch
struct EpochP {
    const int64_t* indptr;      // [N + 1]
    const int64_t* indices;     // [nnz]
    const double* eps;          // epochs_per_sample
    double* next;               // epoch_of_next_sample
    const double* eps_neg;      // epochs_per_negative_sample
    double* next_neg;           // epoch_of_next_negative_sample
    const float* Yin;           // [N][DIM] epoch-start embedding
    float* Yout;
    long N;
    float a, b, gamma, alpha;
    int epoch;
    uint64_t seed;
};

__device__ __forceinline__ float clip4(float x) { return fminf(fmaxf(x, -4.f), 4.f); }

// One epoch for vertex v (one thread): every term reads the epoch-start embedding and the terms are summed in CSR
// order -- each sampled edge's attraction twice (its own and the one the reverse edge moves v by), then its negative
// samples -- and y_v' = y_v + alpha * sum.  No contraction, so that the fp64 schedule state is the plain sums the
// host restates.
template <int DIM>
__global__ __launch_bounds__(EPOCH_THREADS) void umap_epoch_kernel(const EpochP p) {
#pragma clang fp contract(off)
    const long v = (long)blockIdx.x * EPOCH_THREADS + threadIdx.x;
    if (v >= p.N) return;
    const double n = (double)p.epoch;
    float yv[DIM], acc[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d) { yv[d] = p.Yin[v * DIM + d]; acc[d] = 0.f; }
    const float two_ab = 2.f * p.a * p.b, two_gb = 2.f * p.gamma * p.b;
    for (long e = p.indptr[v]; e < p.indptr[v + 1]; ++e) {
        const double nx = p.next[e];
        if (nx > n) continue;
        const long u = p.indices[e];
        float yo[DIM], d2 = 0.f;
#pragma unroll
        for (int d = 0; d < DIM; ++d) { yo[d] = p.Yin[u * DIM + d]; const float df = yv[d] - yo[d]; d2 += df * df; }
        float coef = 0.f;
        if (d2 > 0.f) coef = (-two_ab * powf(d2, p.b - 1.f)) / (p.a * powf(d2, p.b) + 1.f);
#pragma unroll
        for (int d = 0; d < DIM; ++d) {
            const float g = clip4(coef * (yv[d] - yo[d]));
            acc[d] += g;
            acc[d] += g;
        }
        p.next[e] = nx + p.eps[e];
        const double nn = p.next_neg[e], en = p.eps_neg[e];
        const long n_neg = (long)floor((n - nn) / en);
        for (long q = 0; q < n_neg; ++q) {
            const long s = (long)(umap_neg_hash(p.seed, p.epoch, e, q) % (uint64_t)p.N);
            float ys[DIM];
            d2 = 0.f;
#pragma unroll
            for (int d = 0; d < DIM; ++d) { ys[d] = p.Yin[s * DIM + d]; const float df = yv[d] - ys[d]; d2 += df * df; }
            if (!(d2 > 0.f)) continue;            // s == v is skipped; any other coincident sample adds 0
            coef = two_gb / ((0.001f + d2) * (p.a * powf(d2, p.b) + 1.f));
#pragma unroll
            for (int d = 0; d < DIM; ++d) acc[d] += clip4(coef * (yv[d] - ys[d]));
        }
        p.next_neg[e] = nn + (double)n_neg * en;
    }
#pragma unroll
    for (int d = 0; d < DIM; ++d) p.Yout[v * DIM + d] = yv[d] + p.alpha * acc[d];
}

// ---------------------------------------------------------------- transform layout
constexpr int TRANSFORM_THREADS = 64;       // one wave per workgroup: 1600 prototypes are still 25 workgroups
constexpr int TRANSFORM_MAX_K = 64;         // one bit per edge in the thread's live mask

struct TransformP {
    const int64_t* idx;         // [M][k] ordinals of training rows
    const double* weights;      // [M][k]
    const double* eps;          // [M][k] epochs_per_sample, +inf = pruned
    const float* Ytrain;        // [N][DIM], read only
    float* Y;                   // [M][DIM] in / out
    double* next;               // [k][M] epoch_of_next_sample
    double* next_neg;           // [k][M] epoch_of_next_negative_sample
    int* status;
    long M, N;
    int k, n_epochs, epoch_begin, epoch_end;
    float a, b, gamma;
    double initial_alpha, rate;
    uint64_t seed;
};

// All epochs [epoch_begin, epoch_end) of new point i (one thread), its position in registers: the point is attracted to
// and repelled by training rows only, which never move, so no thread reads what another writes.  Every term is applied at
// once, in the order (epoch, edge j, attraction, negative samples p), as umap-learn's loop applies them.  The schedule
// state is [k][M] so that the wave's 64 threads read 64 neighbouring doubles.  No contraction: the fp64 state is the
// plain sums the host restates.
template <int DIM>
__global__ __launch_bounds__(TRANSFORM_THREADS) void umap_transform_kernel(const TransformP p) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * TRANSFORM_THREADS + threadIdx.x;
    if (i >= p.M) return;
    const int k = p.k;
    const bool first = p.epoch_begin == 0;
    // an edge the thread will not follow: ordinal outside [0, N), weight NaN or negative, eps NaN or <= 0
    uint64_t live = 0;
    int refused = 0;
    double init[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d) init[d] = 0.0;
    for (int j = 0; j < k; ++j) {
        const long e = i * k + j;
        const int64_t u = p.idx[e];
        const double w = p.weights[e], ep = p.eps[e];
        const bool ok = u >= 0 && u < p.N && w >= 0.0 && ep > 0.0;
        if (!ok) ++refused;
        else if (ep < INFINITY) live |= 1ull << j;
        if (first) {
            if (ok) {
#pragma unroll
                for (int d = 0; d < DIM; ++d) init[d] += w * (double)p.Ytrain[u * DIM + d];
            }
            p.next[(long)j * p.M + i] = ok ? ep : (double)INFINITY;
            p.next_neg[(long)j * p.M + i] = ok ? ep / p.rate : (double)INFINITY;
        }
    }
    if (refused) atomicAdd(&p.status[0], refused);
    float y[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d) y[d] = first ? (float)init[d] : p.Y[i * DIM + d];

    const float two_ab = 2.f * p.a * p.b, two_gb = 2.f * p.gamma * p.b;
    for (int n = p.epoch_begin; n < p.epoch_end; ++n) {
        const double nd = (double)n;
        const float alpha = (float)(n == 0 ? p.initial_alpha : p.initial_alpha * (1.0 - (double)(n - 1) / (double)p.n_epochs));
        for (uint64_t m = live; m; m &= m - 1) {
            const int j = __ffsll((unsigned long long)m) - 1;
            const long s_at = (long)j * p.M + i;
            const double nx = p.next[s_at];
            if (nx > nd) continue;
            const long e = i * k + j;
            const long u = p.idx[e];
            float df[DIM], d2 = 0.f;
#pragma unroll
            for (int d = 0; d < DIM; ++d) { df[d] = y[d] - p.Ytrain[u * DIM + d]; d2 += df[d] * df[d]; }
            float coef = 0.f;
            if (d2 > 0.f) coef = (-two_ab * powf(d2, p.b - 1.f)) / (p.a * powf(d2, p.b) + 1.f);
#pragma unroll
            for (int d = 0; d < DIM; ++d) y[d] += alpha * clip4(coef * df[d]);
            const double ep = p.eps[e];
            p.next[s_at] = nx + ep;
            const double nn = p.next_neg[s_at], en = ep / p.rate;
            const long n_neg = (long)floor((nd - nn) / en);
            for (long q = 0; q < n_neg; ++q) {
                const long s = (long)(umap_neg_hash(p.seed, n, e, q) % (uint64_t)p.N);
                d2 = 0.f;
#pragma unroll
                for (int d = 0; d < DIM; ++d) { df[d] = y[d] - p.Ytrain[s * DIM + d]; d2 += df[d] * df[d]; }
                if (!(d2 > 0.f)) continue;        // a coincident sample adds nothing
                coef = two_gb / ((0.001f + d2) * (p.a * powf(d2, p.b) + 1.f));
#pragma unroll
                for (int d = 0; d < DIM; ++d) y[d] += alpha * clip4(coef * df[d]);
            }
            p.next_neg[s_at] = nn + (double)n_neg * en;
        }
    }
#pragma unroll
    for (int d = 0; d < DIM; ++d) p.Y[i * DIM + d] = y[d];
}

}  // namespace
}  // namespace vsom

extern "C" {

size_t vsom_umap_transform_workspace_bytes(long M, int k) {
    if (M < 1 || k < 1) return 0;
    return 2 * vsom::align256(sizeof(double) * (size_t)M * (size_t)k);
}

int vsom_umap_transform_layout(const int64_t* knn_idx, const double* weights, const double* epochs_per_sample,
                               const float* Y_train, long N, float* Y, long M, int k, int dim, float a, float b, float gamma,
                               double initial_alpha, int n_epochs, int epoch_begin, int epoch_end, int negative_sample_rate,
                               uint64_t seed, int32_t* status, void* ws, size_t ws_bytes, vsom_stream_t stream) {
    using namespace vsom;
    VSOM_REQUIRE(knn_idx && weights && epochs_per_sample && Y_train && Y && status, VSOM_EINVAL,
                 "umap_transform_layout: null pointer");
    VSOM_REQUIRE(M >= 1 && N >= 1 && k >= 1 && M <= 0x7fffffffL - TRANSFORM_THREADS, VSOM_EINVAL,
                 "umap_transform_layout: bad sizes M=%ld N=%ld k=%d", M, N, k);
    VSOM_REQUIRE(k <= TRANSFORM_MAX_K, VSOM_EUNSUPPORTED, "umap_transform_layout: k=%d > %d", k, TRANSFORM_MAX_K);
    VSOM_REQUIRE(dim >= 1 && dim <= 4, VSOM_EUNSUPPORTED, "umap_transform_layout: dim=%d (1..4)", dim);
    VSOM_REQUIRE(n_epochs >= 0 && epoch_begin >= 0 && epoch_begin <= epoch_end && epoch_end <= n_epochs, VSOM_EINVAL,
                 "umap_transform_layout: bad epochs [%d, %d) of %d", epoch_begin, epoch_end, n_epochs);
    VSOM_REQUIRE(negative_sample_rate >= 1, VSOM_EINVAL, "umap_transform_layout: negative_sample_rate=%d",
                 negative_sample_rate);
    VSOM_REQUIRE(Y != Y_train, VSOM_EINVAL, "umap_transform_layout: Y must not alias Y_train");
    VSOM_REQUIRE(ws && aligned16(ws) && ws_bytes >= vsom_umap_transform_workspace_bytes(M, k), VSOM_EWORKSPACE,
                 "umap_transform_layout: workspace %zu < %zu bytes", ws_bytes, vsom_umap_transform_workspace_bytes(M, k));
    TransformP p = {};
    p.idx = knn_idx; p.weights = weights; p.eps = epochs_per_sample; p.Ytrain = Y_train; p.Y = Y;
    p.next = reinterpret_cast<double*>(ws);
    p.next_neg = reinterpret_cast<double*>(static_cast<char*>(ws) + align256(sizeof(double) * (size_t)M * (size_t)k));
    p.status = status; p.M = M; p.N = N; p.k = k; p.n_epochs = n_epochs; p.epoch_begin = epoch_begin;
    p.epoch_end = epoch_end; p.a = a; p.b = b; p.gamma = gamma; p.initial_alpha = initial_alpha;
    p.rate = (double)negative_sample_rate; p.seed = seed;
    const dim3 grid(cdiv(M, TRANSFORM_THREADS));
    switch (dim) {
        case 1: VSOM_LAUNCH(umap_transform_kernel<1>, grid, dim3(TRANSFORM_THREADS), 0, stream, p); break;
        case 2: VSOM_LAUNCH(umap_transform_kernel<2>, grid, dim3(TRANSFORM_THREADS), 0, stream, p); break;
        case 3: VSOM_LAUNCH(umap_transform_kernel<3>, grid, dim3(TRANSFORM_THREADS), 0, stream, p); break;
        default: VSOM_LAUNCH(umap_transform_kernel<4>, grid, dim3(TRANSFORM_THREADS), 0, stream, p); break;
    }
    return launch_status("umap_transform_layout");
}

long vsom_umap_neg_sample(uint64_t seed, int epoch, long edge, long p, long N) {
    if (N < 1 || epoch < 0 || edge < 0 || p < 0) return -1;
    return (long)(vsom::umap_neg_hash(seed, epoch, edge, p) % (uint64_t)N);
}

int vsom_umap_epoch(const int64_t* indptr, const int64_t* indices, const double* epochs_per_sample,
                    double* epoch_of_next_sample, const double* epochs_per_negative_sample,
                    double* epoch_of_next_negative_sample, const float* Y_in, float* Y_out, long N, int dim, float a,
                    float b, float gamma, float alpha, int epoch, uint64_t seed, vsom_stream_t stream) {
    using namespace vsom;
    VSOM_REQUIRE(indptr && indices && epochs_per_sample && epoch_of_next_sample && epochs_per_negative_sample &&
                     epoch_of_next_negative_sample && Y_in && Y_out,
                 VSOM_EINVAL, "umap_epoch: null pointer");
    VSOM_REQUIRE(N >= 1 && epoch >= 0, VSOM_EINVAL, "umap_epoch: bad sizes N=%ld epoch=%d", N, epoch);
    VSOM_REQUIRE(dim >= 1 && dim <= 4, VSOM_EUNSUPPORTED, "umap_epoch: dim=%d (1..4)", dim);
    VSOM_REQUIRE(Y_in != Y_out, VSOM_EINVAL, "umap_epoch: Y_out must not alias Y_in");
    EpochP p = {};
    p.indptr = indptr; p.indices = indices; p.eps = epochs_per_sample; p.next = epoch_of_next_sample;
    p.eps_neg = epochs_per_negative_sample; p.next_neg = epoch_of_next_negative_sample;
    p.Yin = Y_in; p.Yout = Y_out; p.N = N; p.a = a; p.b = b; p.gamma = gamma; p.alpha = alpha; p.epoch = epoch;
    p.seed = seed;
    const dim3 grid(cdiv(N, EPOCH_THREADS));
    switch (dim) {
        case 1: VSOM_LAUNCH(umap_epoch_kernel<1>, grid, dim3(EPOCH_THREADS), 0, stream, p); break;
        case 2: VSOM_LAUNCH(umap_epoch_kernel<2>, grid, dim3(EPOCH_THREADS), 0, stream, p); break;
        case 3: VSOM_LAUNCH(umap_epoch_kernel<3>, grid, dim3(EPOCH_THREADS), 0, stream, p); break;
        default: VSOM_LAUNCH(umap_epoch_kernel<4>, grid, dim3(EPOCH_THREADS), 0, stream, p); break;
    }
    return launch_status("umap_epoch");
}

}  // extern "C"
