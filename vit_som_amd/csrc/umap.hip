// UMAP for visualize_umap_progression (tools/evaluation.py:267-323): the step of umap-learn's fit that runs once per
// epoch (vit_som_amd/umap.py states the whole algorithm step by step).  The other step that touches the data, the
// exact kNN graph (vsom_umap_knn), is the self mode of the search in knn.hip.
//
//   vsom_umap_epoch        one synchronous epoch of optimize_layout_euclidean: one thread per vertex, walking its CSR row.
//   vsom_umap_neg_sample   the negative-sample hash the epoch evaluates, for the host.
//
// No floating-point atomics anywhere and every sum has one fixed order: a fit is bitwise reproducible.
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

}  // namespace
}  // namespace vsom

extern "C" {

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
