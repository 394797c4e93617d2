// UMAP for visualize_umap_progression (tools/evaluation.py:267-323): the two steps of umap-learn's fit that touch the
// data or run once per epoch (vit_som_amd/umap.py states the whole algorithm step by step).
//
//   vsom_umap_knn     exact k nearest neighbours (euclidean or cosine): the X X^T contraction on the f32 matrix cores
//                     (gemm_f32.h staging, v_mfma_f32_32x32x2_f32), a per-row top-k kept across a workgroup's column
//                     chunk, then a fixed-order merge of the per-chunk lists.
//   vsom_umap_epoch   one synchronous epoch of optimize_layout_euclidean: one thread per vertex, walking its CSR row.
//
// No floating-point atomics anywhere and every sum has one fixed order: a fit is bitwise reproducible.
#include "knn_common.h"

namespace vsom {
namespace {

constexpr int EPOCH_THREADS = 256;            // the kNN tile, list and order definitions: knn_common.h

// (row blocks, column tiles, chunks): chunks split every row's columns so that a small N still fills the GPU; the
// candidate buffer holds chunks * N * k entries, at most about max(N, KNN_TARGET_BLOCKS * KNN_BM) * k.
struct KnnPlan {
    int rb, ct, chunks;
};
inline KnnPlan knn_plan(long N) {
    KnnPlan p;
    p.rb = cdiv(N, KNN_BM);
    p.ct = cdiv(N, KNN_BN);
    const int want = cdiv(KNN_TARGET_BLOCKS, p.rb);
    p.chunks = want < 1 ? 1 : (want > p.ct ? p.ct : want);
    return p;
}

// Workspace: sq f32 [N] (squared row norms), cand_d f32 [chunks][N][k], cand_i i32 [chunks][N][k], each 256-aligned
struct KnnWs {
    float* sq;
    float* cand_d;
    int* cand_i;
    size_t bytes;
};
inline KnnWs knn_layout(void* ws, long N, int k) {
    const KnnPlan pl = knn_plan(N);
    const size_t sq = align256((size_t)N * 4), cand = align256((size_t)pl.chunks * N * k * 4);
    char* p = static_cast<char*>(ws);
    KnnWs w;
    w.sq = reinterpret_cast<float*>(p);
    w.cand_d = reinterpret_cast<float*>(p + sq);
    w.cand_i = reinterpret_cast<int*>(p + sq + cand);
    w.bytes = sq + 2 * cand;
    return w;
}

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

struct KnnP {
    const float* X;
    long ldx;
    int N, D, k, metric;
    const float* sq;
    float* cand_d;      // [chunks][N][k]
    int* cand_i;
    int ct, chunks;
    unsigned x_bytes;   // FAST path: extent of X for the bounds-checked buffer loads
    int vec;            // generic path: 16-byte loads legal
};

// One workgroup = 128 rows x one column chunk.  Per 64-column tile: the 128 x 64 block of X X^T on the f32 matrix
// cores (knn_tile_dots in knn_common.h: wave w owns rows 32w..32w+31), the
// distances into LDS, then every wave folds each of its 32 rows' 64 candidates into that row's list (registers: lane j
// holds entry j).  Row i against itself gets distance -1: it sorts before every real distance (>= 0) and is written
// out as 0, so row i comes first even when a duplicate of it has a lower index.  At the end the lists go to the
// chunk's candidate slab.
template <bool FAST>
__global__ __launch_bounds__(KNN_THREADS) void umap_knn_tile_kernel(const KnnP p) {
    constexpr int BM = KNN_BM, BN = KNN_BN;
    __shared__ __attribute__((aligned(16))) float lds[(BM + BN) * 36];
    __shared__ float sd[BM][BN + 1];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wm0 = wave * 32;
    const int bm0 = blockIdx.x * BM;
    const int chunk = blockIdx.y;
    const int ct0 = (int)((long)chunk * p.ct / p.chunks), ct1 = (int)((long)(chunk + 1) * p.ct / p.chunks);

    float ld_[32];
    int li_[32];
#pragma unroll
    for (int rr = 0; rr < 32; ++rr) { ld_[rr] = INFINITY; li_[rr] = 0x7fffffff; }

    const KnnOperand X = {p.X, p.ldx, p.N, p.x_bytes, p.vec};
    KnnStage<FAST> st;
    knn_stage_init<FAST>(st, X, bm0, X, t);

    for (int ctile = ct0; ctile < ct1; ++ctile) {
        const int bn0 = ctile * BN;
        f32x16 acc[2];
        knn_tile_dots<FAST>(st, X, bm0, X, bn0, p.D, lds, t, acc);

        // accumulator register v of tile j: row (v & 3) + 8 (v >> 2) + 4h, column 32j + r
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = j * 32 + r, gj = bn0 + col;
            const float sj = gj < p.N ? p.sq[gj] : 0.f;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int row = wm0 + (v & 3) + 8 * (v >> 2) + 4 * h, gi = bm0 + row;
                float d = INFINITY;
                if (gi < p.N && gj < p.N) d = gi == gj ? -1.f : knn_distance(acc[j][v], p.sq[gi], sj, p.metric);
                sd[row][col] = d;
            }
        }
        __syncthreads();        // also: every wave is past its last MFMA read of As / Bs before the next tile's lstore
        const int gj = bn0 + lane;
        const bool ok = gj < p.N;
#pragma unroll
        for (int rr = 0; rr < 32; ++rr)
            knn_insert(ld_[rr], li_[rr], ok ? sd[wm0 + rr][lane] : INFINITY, ok ? gj : 0x7fffffff, p.k, lane);
    }
#pragma unroll
    for (int rr = 0; rr < 32; ++rr) {
        const int gi = bm0 + wm0 + rr;
        if (gi < p.N && lane < p.k) {
            const size_t o = ((size_t)chunk * p.N + gi) * p.k + lane;
            p.cand_d[o] = ld_[rr];
            p.cand_i[o] = li_[rr];
        }
    }
}

// The per-chunk lists of a row merged in chunk order (one wave per row): the k smallest in (distance, index) order.
__global__ __launch_bounds__(KNN_MERGE_ROWS * 64) void umap_knn_merge_kernel(const float* __restrict__ cand_d,
                                                                             const int* __restrict__ cand_i, int N, int k,
                                                                             int chunks, int64_t* __restrict__ knn_idx,
                                                                             float* __restrict__ knn_dist) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * KNN_MERGE_ROWS + (threadIdx.x >> 6);
    if (i >= N) return;
    float ld = INFINITY;
    int li = 0x7fffffff;
    for (int c = 0; c < chunks; ++c) {
        const size_t o = ((size_t)c * N + i) * k + lane;
        knn_insert(ld, li, lane < k ? cand_d[o] : INFINITY, lane < k ? cand_i[o] : 0x7fffffff, k, lane);
    }
    if (lane < k) {
        knn_idx[(size_t)i * k + lane] = li;
        knn_dist[(size_t)i * k + lane] = fmaxf(ld, 0.f);          // row i itself: -1 -> 0
    }
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

size_t vsom_umap_knn_workspace_bytes(long N, int k) {
    if (N < 1 || k < 1) return 0;
    return vsom::knn_layout(nullptr, N, k).bytes;
}

int vsom_umap_knn(const float* X, long ldx, long N, int D, int k, int metric, int64_t* knn_idx, float* knn_dist, void* ws,
                  size_t ws_bytes, vsom_stream_t stream) {
    using namespace vsom;
    VSOM_REQUIRE(X && knn_idx && knn_dist, VSOM_EINVAL, "umap_knn: null pointer");
    VSOM_REQUIRE(N >= 2 && D >= 1 && k >= 1 && k < N && ldx >= D && N <= 0x7fffffffL - KNN_BM, VSOM_EINVAL,
                 "umap_knn: bad sizes N=%ld D=%d k=%d ldx=%ld", N, D, k, ldx);
    VSOM_REQUIRE(k <= KNN_MAX_K, VSOM_EUNSUPPORTED, "umap_knn: k=%d > %d", k, KNN_MAX_K);
    VSOM_REQUIRE(metric == VSOM_DIST_EUCLIDEAN || metric == VSOM_DIST_COSINE, VSOM_EUNSUPPORTED,
                 "umap_knn: metric %d (euclidean or cosine only)", metric);
    VSOM_REQUIRE(ws && aligned16(ws) && ws_bytes >= vsom_umap_knn_workspace_bytes(N, k), VSOM_EWORKSPACE,
                 "umap_knn: workspace too small or misaligned");
    const KnnPlan pl = knn_plan(N);
    const KnnWs w = knn_layout(ws, N, k);
    VSOM_LAUNCH(knn_sqnorm_kernel, dim3(cdiv(N, 256)), dim3(256), 0, stream, X, ldx, N, D, w.sq);
    KnnP p = {};
    p.X = X; p.ldx = ldx; p.N = (int)N; p.D = D; p.k = k; p.metric = metric; p.sq = w.sq;
    p.cand_d = w.cand_d; p.cand_i = w.cand_i; p.ct = pl.ct; p.chunks = pl.chunks;
    const bool vec = D % 4 == 0 && ldx % 4 == 0 && aligned16(X);
    const size_t extent = (size_t)N * ldx * 4;
    p.vec = vec;
    p.x_bytes = (unsigned)extent;
    if (vec && extent < (size_t)OOB - 256) {
        VSOM_LAUNCH(umap_knn_tile_kernel<true>, dim3(pl.rb, pl.chunks), dim3(KNN_THREADS), 0, stream, p);
    } else {
        VSOM_LAUNCH(umap_knn_tile_kernel<false>, dim3(pl.rb, pl.chunks), dim3(KNN_THREADS), 0, stream, p);
    }
    VSOM_LAUNCH(umap_knn_merge_kernel, dim3(cdiv(N, KNN_MERGE_ROWS)), dim3(KNN_MERGE_ROWS * 64), 0, stream,
                (const float*)w.cand_d, (const int*)w.cand_i, (int)N, k, pl.chunks, knn_idx, knn_dist);
    return launch_status("umap_knn");
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
