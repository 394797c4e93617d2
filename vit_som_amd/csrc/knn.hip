// k-nearest-neighbour probe (evaluate_knn; no counterpart in the reference): the neighbours of one set (queries) in
// another (the bank), streamed bank chunk by bank chunk, and the weighted class vote over them.
//
//   vsom_knn_query   exact k nearest bank rows of every query (euclidean or cosine): the Q X^T contraction on the f32
//                    matrix cores (knn_common.h: the tile, the order and the distance vsom_umap_knn uses), a per-query
//                    top-k kept across a workgroup's column chunk, then a fixed-order merge of the per-chunk lists that
//                    also takes the list already in the output when `accumulate` is set.
//   vsom_knn_vote    one wave per query: fp64 class scores in neighbour order, first argmax.
//
// No floating-point atomics and every sum has one fixed order: results are bitwise reproducible, and folding a bank in
// any number of pieces, in any order, gives bit for bit the lists of one call over the whole bank.
#include "knn_common.h"

namespace vsom {
namespace {

constexpr int VOTE_WAVES = 4;                // queries per vote workgroup (one wave each)
constexpr int VOTE_MAX_CLASSES = 1024;       // fp64 LDS score table per wave: 4 x 8 KB
constexpr int64_t KNN_NO_INDEX = 0x7fffffffffffffffLL;      // sorts after every real ordinal; stored as -1

// (query row blocks, bank column tiles, chunks): chunks split the bank's columns so that few queries still fill the GPU.
struct QueryPlan {
    int rb, ct, chunks;
};
inline QueryPlan query_plan(long Nq, long Nb) {
    QueryPlan p;
    p.rb = cdiv(Nq, KNN_BM);
    p.ct = cdiv(Nb, KNN_BN);
    const int want = cdiv(KNN_TARGET_BLOCKS, p.rb);
    p.chunks = want < 1 ? 1 : (want > p.ct ? p.ct : want);
    return p;
}

// Workspace: sqq f32 [Nq], sqx f32 [Nb], cand_d f32 [chunks][Nq][k], cand_i i32 [chunks][Nq][k], each 256-aligned.  The
// slabs are sized by a bound on chunks * Nq that grows with Nq -- chunks * rb <= min(ct * rb, KNN_TARGET_BLOCKS - 1 + rb)
// -- so that the size is monotone in every argument (chunks itself falls as Nq grows).
inline size_t knn_min(size_t a, size_t b) { return a < b ? a : b; }
struct QueryWs {
    float* sqq;
    float* sqx;
    float* cand_d;
    int* cand_i;
    size_t bytes;
};
inline QueryWs query_layout(void* ws, long Nq, long Nb, int k) {
    const QueryPlan pl = query_plan(Nq, Nb);
    const size_t blocks = knn_min((size_t)pl.ct * pl.rb, (size_t)KNN_TARGET_BLOCKS - 1 + pl.rb);
    const size_t sqq = align256((size_t)Nq * 4), sqx = align256((size_t)Nb * 4);
    const size_t cand = align256(blocks * KNN_BM * (size_t)k * 4);
    char* p = static_cast<char*>(ws);
    QueryWs w;
    w.sqq = reinterpret_cast<float*>(p);
    w.sqx = reinterpret_cast<float*>(p + sqq);
    w.cand_d = reinterpret_cast<float*>(p + sqq + sqx);
    w.cand_i = reinterpret_cast<int*>(p + sqq + sqx + cand);
    w.bytes = sqq + sqx + 2 * cand;
    return w;
}

struct QueryP {
    KnnOperand Q, X;
    int D, k, metric;
    const float* sqq;
    const float* sqx;
    const int64_t* exclude;     // [Nq] global bank ordinals, or null
    int64_t index_base;
    float* cand_d;              // [chunks][Nq][k]
    int* cand_i;                // bank rows of THIS call (the merge adds index_base)
    int ct, chunks;
};

// One workgroup = 128 queries x one chunk of bank columns.  Per 64-column tile: the 128 x 64 block of Q X^T
// (knn_tile_dots), the distances into LDS, then every wave folds each of its 32 queries' 64 candidates into that
// query's list (registers: lane j holds entry j).  A column outside the bank, or the one a query excludes, is offered
// as (+inf, no index): it is never inserted.  At the end the lists go to the chunk's candidate slab.
template <bool FAST>
__global__ __launch_bounds__(KNN_THREADS) void knn_query_tile_kernel(const QueryP p) {
    constexpr int BM = KNN_BM, BN = KNN_BN;
    __shared__ __attribute__((aligned(16))) float lds[(BM + BN) * 36];
    __shared__ float sd[BM][BN + 1];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wm0 = wave * 32;
    const int bm0 = blockIdx.x * BM;
    const int chunk = blockIdx.y;
    const int ct0 = (int)((long)chunk * p.ct / p.chunks), ct1 = (int)((long)(chunk + 1) * p.ct / p.chunks);
    const int Nq = p.Q.rows, Nb = p.X.rows;

    float ld_[32];
    int li_[32];
#pragma unroll
    for (int rr = 0; rr < 32; ++rr) { ld_[rr] = INFINITY; li_[rr] = 0x7fffffff; }

    // the bank row (of this call) each of the wave's queries must not receive: lane rr holds query wm0 + rr's, -1 = none
    int excl = -1;
    if (p.exclude && lane < 32 && bm0 + wm0 + lane < Nq) {
        const int64_t e = p.exclude[bm0 + wm0 + lane] - p.index_base;
        if (e >= 0 && e < Nb) excl = (int)e;
    }

    KnnStage<FAST> st;
    knn_stage_init<FAST>(st, p.Q, bm0, p.X, t);

    for (int ctile = ct0; ctile < ct1; ++ctile) {
        const int bn0 = ctile * BN;
        f32x16 acc[2];
        knn_tile_dots<FAST>(st, p.Q, bm0, p.X, bn0, p.D, lds, t, acc);

        // accumulator register v of tile j: row (v & 3) + 8 (v >> 2) + 4h, column 32j + r
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = j * 32 + r, gj = bn0 + col;
            const float sj = gj < Nb ? p.sqx[gj] : 0.f;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int row = wm0 + (v & 3) + 8 * (v >> 2) + 4 * h, gi = bm0 + row;
                float d = INFINITY;
                if (gi < Nq && gj < Nb) d = knn_distance(acc[j][v], p.sqq[gi], sj, p.metric);
                sd[row][col] = d;
            }
        }
        __syncthreads();        // also: every wave is past its last MFMA read of the LDS tiles before the next tile's stores
        const int gj = bn0 + lane;
#pragma unroll
        for (int rr = 0; rr < 32; ++rr) {
            const int ex = __shfl(excl, rr, 64);        // by every lane: a shuffle under `gj < Nb` would read inactive lanes as 0
            const bool ok = gj < Nb && gj != ex;
            knn_insert(ld_[rr], li_[rr], ok ? sd[wm0 + rr][lane] : INFINITY, ok ? gj : 0x7fffffff, p.k, lane);
        }
    }
#pragma unroll
    for (int rr = 0; rr < 32; ++rr) {
        const int gi = bm0 + wm0 + rr;
        if (gi < Nq && lane < p.k) {
            const size_t o = ((size_t)chunk * Nq + gi) * p.k + lane;
            p.cand_d[o] = ld_[rr];
            p.cand_i[o] = li_[rr];
        }
    }
}

// One wave per query: the list already in (idx, dist) when `accumulate` (an entry with idx < 0 is an empty slot), then
// the per-chunk lists in chunk order, folded into the k smallest by (distance, global ordinal).  Empty slots leave as
// (+inf, -1).
__global__ __launch_bounds__(KNN_MERGE_ROWS * 64) void knn_query_merge_kernel(const float* __restrict__ cand_d,
                                                                              const int* __restrict__ cand_i, int Nq, int k,
                                                                              int chunks, int64_t index_base, int accumulate,
                                                                              int64_t* __restrict__ idx,
                                                                              float* __restrict__ dist) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * KNN_MERGE_ROWS + (threadIdx.x >> 6);
    if (i >= Nq) return;
    float ld = INFINITY;
    int64_t li = KNN_NO_INDEX;
    if (accumulate) {           // the incoming list is offered like a chunk: its entries are re-inserted, not trusted to be sorted
        float cd = INFINITY;
        int64_t ci = KNN_NO_INDEX;
        if (lane < k) {
            const int64_t gi = idx[(size_t)i * k + lane];
            if (gi >= 0) { cd = dist[(size_t)i * k + lane]; ci = gi; }
        }
        knn_insert(ld, li, cd, ci, k, lane);
    }
    for (int c = 0; c < chunks; ++c) {
        const size_t o = ((size_t)c * Nq + i) * k + lane;
        float cd = INFINITY;
        int64_t ci = KNN_NO_INDEX;
        if (lane < k) {
            const int row = cand_i[o];
            if (row != 0x7fffffff) { cd = cand_d[o]; ci = index_base + row; }
        }
        knn_insert(ld, li, cd, ci, k, lane);
    }
    if (lane < k) {
        const bool empty = li == KNN_NO_INDEX;
        idx[(size_t)i * k + lane] = empty ? -1 : li;
        dist[(size_t)i * k + lane] = empty ? INFINITY : ld;
    }
}

struct VoteP {
    const int64_t* idx;
    const float* dist;
    int Nq, k;
    const int64_t* bank_labels;
    long n_bank;
    int n_classes, weights;
    float temperature;
    int64_t* pred;
    double* scores;     // [Nq][n_classes] or null
    int* status;        // [0] neighbours refused, [1] queries without a valid neighbour
};

// One wave per query.  Lane j holds neighbour j: its label and fp64 weight (0 weight and label -1 when skipped); lane 0
// adds the weights into the wave's LDS table in neighbour order j = 0..k-1; then the first argmax over the classes.
__global__ __launch_bounds__(VOTE_WAVES * 64) void knn_vote_kernel(const VoteP p) {
    __shared__ double table[VOTE_WAVES][VOTE_MAX_CLASSES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * VOTE_WAVES + wave;
    const bool active = i < p.Nq;                 // no early return: the workgroup meets at two barriers
    double* sc = table[wave];
    for (int c = lane; c < p.n_classes; c += 64) sc[c] = 0.0;

    int label = -1;
    float d = 0.f;
    bool refused = false;
    if (active && lane < p.k) {
        const int64_t n = p.idx[(size_t)i * p.k + lane];
        if (n >= 0) {
            if (n >= p.n_bank) {
                refused = true;
            } else {
                const int64_t y = p.bank_labels[n];
                if (y < 0 || y >= p.n_classes) refused = true;
                else { label = (int)y; d = p.dist[(size_t)i * p.k + lane]; }
            }
        }
    }
    const bool valid = label >= 0;
    double w = 0.0;
    if (p.weights == VSOM_KNN_UNIFORM) {
        w = 1.0;
    } else if (p.weights == VSOM_KNN_DISTANCE) {
        const bool any_zero = __ballot(valid && d == 0.f) != 0;
        w = any_zero ? (d == 0.f ? 1.0 : 0.0) : 1.0 / (double)d;
    } else {
        w = exp(-(double)d / (double)p.temperature);
    }
    if (!valid) w = 0.0;
    const unsigned long long vmask = __ballot(valid);
    const int n_refused = __popcll(__ballot(refused));
    __syncthreads();
    for (int j = 0; j < p.k; ++j) {
        const int cj = __shfl(label, j, 64);
        const double wj = __shfl(w, j, 64);
        if (lane == 0 && cj >= 0) sc[cj] += wj;
    }
    __syncthreads();
    if (!active) return;

    double best = -1.0;
    int arg = 0x7fffffff;
    for (int c = lane; c < p.n_classes; c += 64) {
        const double v = sc[c];
        if (p.scores) p.scores[(size_t)i * p.n_classes + c] = v;
        if (v > best) { best = v; arg = c; }           // ascending c: the first maximum of this lane's classes
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o, 64);
        const int oa = __shfl_xor(arg, o, 64);
        if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
    }
    if (lane == 0) {
        p.pred[i] = vmask ? arg : -1;
        if (n_refused) atomicAdd(&p.status[0], n_refused);
        if (!vmask) atomicAdd(&p.status[1], 1);
    }
}

}  // namespace
}  // namespace vsom

extern "C" {

size_t vsom_knn_query_workspace_bytes(long Nq, long Nb, int k) {
    if (Nq < 1 || Nb < 1 || k < 1) return 0;
    return vsom::query_layout(nullptr, Nq, Nb, k).bytes;
}

int vsom_knn_query(const float* Q, long ldq, long Nq, const float* X, long ldx, long Nb, int D, int k, int metric,
                   int64_t index_base, int accumulate, const int64_t* exclude, int64_t* idx, float* dist, void* ws,
                   size_t ws_bytes, vsom_stream_t stream) {
    using namespace vsom;
    VSOM_REQUIRE(Q && X && idx && dist, VSOM_EINVAL, "knn_query: null pointer");
    const long max_rows = 0x7fffffffL - KNN_BM;
    VSOM_REQUIRE(Nq >= 1 && Nb >= 1 && D >= 1 && k >= 1 && ldq >= D && ldx >= D && index_base >= 0 && Nq <= max_rows &&
                     Nb <= max_rows,
                 VSOM_EINVAL, "knn_query: bad sizes Nq=%ld Nb=%ld D=%d k=%d ldq=%ld ldx=%ld index_base=%lld", Nq, Nb, D, k, ldq,
                 ldx, (long long)index_base);
    VSOM_REQUIRE(k <= KNN_MAX_K, VSOM_EUNSUPPORTED, "knn_query: k=%d > %d", k, KNN_MAX_K);
    VSOM_REQUIRE(metric == VSOM_DIST_EUCLIDEAN || metric == VSOM_DIST_COSINE, VSOM_EUNSUPPORTED,
                 "knn_query: metric %d (euclidean or cosine only)", metric);
    VSOM_REQUIRE(ws && aligned16(ws) && ws_bytes >= vsom_knn_query_workspace_bytes(Nq, Nb, k), VSOM_EWORKSPACE,
                 "knn_query: workspace too small or misaligned");
    const QueryPlan pl = query_plan(Nq, Nb);
    const QueryWs w = query_layout(ws, Nq, Nb, k);
    VSOM_LAUNCH(knn_sqnorm_kernel, dim3(cdiv(Nq, 256)), dim3(256), 0, stream, Q, ldq, Nq, D, w.sqq);
    VSOM_LAUNCH(knn_sqnorm_kernel, dim3(cdiv(Nb, 256)), dim3(256), 0, stream, X, ldx, Nb, D, w.sqx);
    const bool qvec = D % 4 == 0 && ldq % 4 == 0 && aligned16(Q), xvec = D % 4 == 0 && ldx % 4 == 0 && aligned16(X);
    const size_t qext = (size_t)Nq * ldq * 4, xext = (size_t)Nb * ldx * 4;
    QueryP p = {};
    p.Q = {Q, ldq, (int)Nq, (unsigned)qext, qvec};
    p.X = {X, ldx, (int)Nb, (unsigned)xext, xvec};
    p.D = D; p.k = k; p.metric = metric; p.sqq = w.sqq; p.sqx = w.sqx; p.exclude = exclude; p.index_base = index_base;
    p.cand_d = w.cand_d; p.cand_i = w.cand_i; p.ct = pl.ct; p.chunks = pl.chunks;
    if (qvec && xvec && qext < (size_t)OOB - 256 && xext < (size_t)OOB - 256) {
        VSOM_LAUNCH(knn_query_tile_kernel<true>, dim3(pl.rb, pl.chunks), dim3(KNN_THREADS), 0, stream, p);
    } else {
        VSOM_LAUNCH(knn_query_tile_kernel<false>, dim3(pl.rb, pl.chunks), dim3(KNN_THREADS), 0, stream, p);
    }
    VSOM_LAUNCH(knn_query_merge_kernel, dim3(cdiv(Nq, KNN_MERGE_ROWS)), dim3(KNN_MERGE_ROWS * 64), 0, stream,
                (const float*)w.cand_d, (const int*)w.cand_i, (int)Nq, k, pl.chunks, index_base, accumulate, idx, dist);
    return launch_status("knn_query");
}

int vsom_knn_vote(const int64_t* idx, const float* dist, long Nq, int k, const int64_t* bank_labels, long n_bank,
                  int n_classes, int weights, float temperature, int64_t* pred, double* scores, int* status,
                  vsom_stream_t stream) {
    using namespace vsom;
    VSOM_REQUIRE(idx && dist && bank_labels && pred && status, VSOM_EINVAL, "knn_vote: null pointer");
    VSOM_REQUIRE(Nq >= 1 && Nq <= 0x7fffffffL - VOTE_WAVES && k >= 1 && n_bank >= 1 && n_classes >= 1, VSOM_EINVAL,
                 "knn_vote: bad sizes Nq=%ld k=%d n_bank=%ld n_classes=%d", Nq, k, n_bank, n_classes);
    VSOM_REQUIRE(k <= KNN_MAX_K, VSOM_EUNSUPPORTED, "knn_vote: k=%d > %d", k, KNN_MAX_K);
    VSOM_REQUIRE(n_classes <= VOTE_MAX_CLASSES, VSOM_EUNSUPPORTED, "knn_vote: n_classes=%d > %d", n_classes, VOTE_MAX_CLASSES);
    VSOM_REQUIRE(weights == VSOM_KNN_UNIFORM || weights == VSOM_KNN_DISTANCE || weights == VSOM_KNN_SOFTMAX, VSOM_EUNSUPPORTED,
                 "knn_vote: weights %d (uniform, distance or softmax)", weights);
    VSOM_REQUIRE(weights != VSOM_KNN_SOFTMAX || temperature > 0.f, VSOM_EINVAL, "knn_vote: temperature must be > 0");
    VoteP p = {};
    p.idx = idx; p.dist = dist; p.Nq = (int)Nq; p.k = k; p.bank_labels = bank_labels; p.n_bank = n_bank;
    p.n_classes = n_classes; p.weights = weights; p.temperature = temperature; p.pred = pred; p.scores = scores;
    p.status = status;
    VSOM_LAUNCH(knn_vote_kernel, dim3(cdiv(Nq, VOTE_WAVES)), dim3(VOTE_WAVES * 64), 0, stream, p);
    return launch_status("knn_vote");
}

}  // extern "C"
