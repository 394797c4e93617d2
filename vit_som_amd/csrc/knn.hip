// Exact k nearest neighbours on the f32 matrix cores, one search path behind two entry points, and the class vote of the
// kNN probe (evaluate_knn; no counterpart in the reference).
//
//   vsom_knn_query   the k nearest rows of a bank chunk for every query (euclidean or cosine), the bank streamed chunk by
//                    chunk: a fixed-order merge of the per-chunk lists also takes the list already in the output when
//                    `accumulate` is set.
//   vsom_umap_knn    the same search of a set among itself (UMAP's kNN graph): the self mode of the same kernels, which
//                    puts row i first in its own list at distance 0, before any duplicate of it with a lower index.
//   vsom_knn_vote    one wave per query: fp64 class scores in neighbour order, first argmax.
//   vsom_knn_ranks   the same contraction of a set with itself, counting instead of selecting: for every row and each
//                    row listed for it, how many other rows lie closer and how many exactly as far (trustworthiness and
//                    continuity of an embedding).  Integer atomics only.
//   vsom_silhouette  the same contraction once more, summing instead of counting: for every row the fixed-point sum of its
//                    distances to each cluster's members, then the silhouette coefficient.  Integer atomics only.
//   vsom_dbscan_*    the same contraction, thresholding: the eps-neighbourhood graph as a bit matrix, one
//                    wave64 ballot per word, no atomics; then the connected components of the core rows (int32,
//                    atomicMin only) and sklearn's DBSCAN labels.  The contract stands at the head of that section.
//   vsom_hdbscan_*   the same contraction, once per Boruvka round: every row's least mutual-reachability edge
//                    out of its component, then the components' hooks -- the minimum spanning tree HDBSCAN reads its
//                    hierarchy from, under a strict order of the edges.  Integer atomicMin only.
//
// What the five tile kernels share, written once next to knn_tile_dots: KnnBlock (where a thread stands: its rows, its
// accumulator column, the chunk's tiles -- the one chunk split and the one register-to-row map), knn_tile_dots (the
// tile of dot products) and knn_tile_walk (every dot product handed to the kernel's own distance predicate, then the
// barrier).  The four contractions of a set with itself also share the head of their parameter structs (SelfP) and
// their launch (knn_self_launch).  A kernel keeps its tile loop, its predicate -- which pairs are NaN, 0, -1 or +inf --
// and its wave-level epilogue, which is what it is there for.  The next self-contraction writes: a struct deriving from
// SelfP with its own fields, a kernel<FAST> of that shape, and an entry that fills those fields and calls knn_self_launch.
//
// The contract the search entry points keep (the rank pass takes its distances from the same four), written once below:
//   - the 128 x 64 tile of dot products (knn_tile_dots: the staging, the k-loop and the MFMA order of gemm_f32.h, shared
//     with gemm_f32_kernel and pca_gemm_kernel), every (row, row) pair summed over D in one fixed order that depends
//     neither on where the two rows fall in a tile nor on the sizes of the two sets;
//   - the squared norms summed in that same order (knn_sqnorm_kernel), so identical rows are at distance exactly 0;
//   - the distance from (dot, norm, norm) (knn_distance);
//   - the strict (distance, index) total order of the lists and the order-independent insertion (knn_less, knn_insert).
// No floating-point atomics and every sum has one fixed order: results are bitwise reproducible, and folding a bank in
// any number of pieces, in any order, gives bit for bit the lists of one call over the whole bank.
#include "gemm_f32.h"

namespace vsom {
namespace {

constexpr int KNN_BM = 128;                  // rows per workgroup (4 waves x 32)
constexpr int KNN_BN = 64;                   // columns per tile (two 32 x 32 accumulators per wave)
constexpr int KNN_THREADS = 256;
constexpr int KNN_MAX_K = 64;                // one list entry per lane
constexpr int KNN_TARGET_BLOCKS = 2048;      // workgroups wanted per launch (8 per CU): the column chunking stops there
constexpr int KNN_MERGE_ROWS = 4;            // rows per merge workgroup (one wave each)
constexpr int VOTE_WAVES = 4;                // queries per vote workgroup (one wave each)
constexpr int VOTE_MAX_CLASSES = 1024;       // fp64 LDS score table per wave: 4 x 8 KB
constexpr int64_t KNN_NO_INDEX = 0x7fffffffffffffffLL;      // sorts after every real ordinal; stored as -1

// Squared row norms in the order in which mfma_tile (gemm_f32.h: the one definition of the order) sums a row's products
// with itself: in groups of 8, k = kb + s then kb + 4 + s for s = 0..3 (lane half h feeds k = kb + 4h + s to MFMA step s;
// the instruction is bitwise fma(a_k1 b_k1, fma(a_k0 b_k0, c))).  So sq[i] is <x_i, x_i> of the contraction bit for bit,
// and the euclidean distance between two identical rows is exactly 0.
__device__ __forceinline__ float knn_sqnorm_row(const float* __restrict__ x, int D) {
    float s = 0.f;
    for (int kb = 0; kb < D; kb += 8) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float a0 = kb + j < D ? x[kb + j] : 0.f;
            const float a1 = kb + 4 + j < D ? x[kb + 4 + j] : 0.f;
            s = fmaf(a0, a0, s);
            s = fmaf(a1, a1, s);
        }
    }
    return s;
}
__global__ __launch_bounds__(256) void knn_sqnorm_kernel(const float* __restrict__ X, long ldx, long N, int D,
                                                        float* __restrict__ sq) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    sq[i] = knn_sqnorm_row(X + i * ldx, D);
}

// Strict total order of the lists: (distance, index) lexicographic.  I is int (row of this launch) or int64_t (global ordinal).
template <class I>
__device__ __forceinline__ bool knn_less(float d0, I i0, float d1, I i1) { return d0 < d1 || (d0 == d1 && i0 < i1); }

// Insert the wave's candidates (lane l offers (cd, ci)) into a row's sorted list (lane j < k holds entry j), lowest
// lane first.  The result is the k smallest of list and candidates in (distance, index) order: it does not depend on
// the order of insertion, hence neither on the tiling nor on the chunking.
template <class I>
__device__ __forceinline__ void knn_insert(float& ld, I& li, float cd, I ci, int k, int lane) {
    const float kd = __shfl(ld, k - 1, 64);
    const I ki = __shfl(li, k - 1, 64);
    unsigned long long mask = __ballot(knn_less(cd, ci, kd, ki));
    while (mask) {
        const int s = __builtin_ctzll(mask);
        mask &= mask - 1;
        const float xd = __shfl(cd, s, 64);
        const I xi = __shfl(ci, s, 64);
        const int pos = __popcll(__ballot(lane < k && knn_less(ld, li, xd, xi)));
        const float ud = __shfl_up(ld, 1, 64);
        const I ui = __shfl_up(li, 1, 64);
        if (pos < k) {
            if (lane > pos) { ld = ud; li = ui; }
            else if (lane == pos) { ld = xd; li = xi; }
        }
    }
}

// Distance from the dot product and the two squared norms (umap-learn's definitions; cosine of a zero row: 0 against
// another zero row, 1 against any other row).
// The bad-row contract: a pair with a row that holds a NaN or an infinity, or whose squared norm overflows fp32, has
// no distance: NaN, decided BEFORE the clamps (fmaxf(NaN, 0) is 0, which would make such a row everyone's nearest
// neighbour).  NaN is below, above and equal to nothing, so knn_less never inserts it and the rank pass never counts
// it; what reads a distance in another way tests d == d.  For finite operands every bit is as without the test.
__device__ __forceinline__ float knn_distance(float dot, float si, float sj, int metric) {
    if (metric == VSOM_DIST_EUCLIDEAN) {
        const float d2 = si + sj - 2.f * dot;
        return fabsf(d2) < INFINITY ? sqrtf(fmaxf(d2, 0.f)) : __builtin_nanf("");
    }
    if (!(si < INFINITY && sj < INFINITY && fabsf(dot) < INFINITY)) return __builtin_nanf("");
    if (si == 0.f && sj == 0.f) return 0.f;
    if (si == 0.f || sj == 0.f) return 1.f;
    if (dot == si && dot == sj) return 0.f;                          // identical rows
    return fmaxf(1.f - dot / (sqrtf(si) * sqrtf(sj)), 0.f);
}

// One operand of the contraction: rows [rows, D] with row stride ld.
using KnnOperand = F32Operand;

// The operand staging of one workgroup (gemm_f32.h, the NT form).  A kernel points it at its operands and computes the
// row offsets of its 128 A rows once (point, rows_a), knn_tile_dots those of a 64-row B tile once per tile (FAST path
// only; the generic path indexes from the pointers); point() alone moves it to operands that begin elsewhere in the
// same rows (the silhouette's later k-segments): the row offsets stay.
template <bool FAST>
using KnnStage = F32Stage<true, true, KNN_BM, KNN_BN, FAST>;

// Where one thread stands in a tile kernel's grid (row blocks, chunks) of 256-thread workgroups: its wave owns rows wm0..wm0 +
// 31 of the block's 128 (from bm0), its lane column r of each 32-column accumulator and the row half h (mfma_tile), and the
// workgroup the column tiles [ct0, ct1) of the launch's ct.  The one place that spells the chunk split: the chunks are
// disjoint and cover every tile, which dbscan_tile_kernel relies on -- it writes every word of adj exactly once and
// clears nothing.  row(v): the block row of accumulator register v, the one statement of mfma_tile's output layout.
struct KnnBlock {
    int t, lane, wave, r, h, wm0, bm0, chunk, ct0, ct1;
    __device__ __forceinline__ KnnBlock(int ct, int chunks)
        : t(threadIdx.x), lane(t & 63), wave(t >> 6), r(lane & 31), h(lane >> 5), wm0(wave * 32), bm0(blockIdx.x * KNN_BM),
          chunk(blockIdx.y) {
        auto first_tile = [&](int c) { return (int)((long)c * ct / chunks); };
        ct0 = first_tile(chunk); ct1 = first_tile(chunk + 1);
    }
    __device__ __forceinline__ int row(int v) const { return wm0 + (v & 3) + 8 * (v >> 2) + 4 * h; }
};

// acc[j] <- the 128 x 64 block <A[bm0 + .], B[bn0 + .]> over K on the f32 matrix cores: wave w owns rows 32w..32w+31,
// acc[j] columns 32j..32j+31 (register v of acc[j]: row KnnBlock::row(v), column 32j + r).  Operand tiles are
// staged global -> registers -> LDS by the staging, the k-loop and the MFMA order of gemm_f32_kernel, the same code
// (gemm_f32.h; lds: (128 + 64) * 36 floats).  Every pair's products are summed k-tile by k-tile, 8-group by 8-group,
// step s = 0..3 with k = kb + s before kb + 4 + s inside the instruction (mfma_tile): one order for every pair.  Rows
// outside either operand and k >= K contribute exact zeros.  All waves must call it; the caller synchronises before the
// next call overwrites the LDS tiles (knn_tile_walk does).
template <bool FAST>
__device__ __forceinline__ void knn_tile_dots(KnnStage<FAST>& st, const KnnBlock& g, const KnnOperand& A, const KnnOperand& B,
                                              int bn0, int K, float* lds, f32x16 (&acc)[2]) {
    constexpr int BM = KNN_BM, BN = KNN_BN;
    float* As = lds;
    float* Bs = lds + BM * 36;
    const int ktiles = (K + 31) >> 5;
    st.rows_b(B, bn0, g.t);
    auto gload = [&](int kt) { st.gload(A, g.bm0, B, bn0, kt << 5, K, g.t); };
    auto lstore = [&]() { st.lstore(As, Bs, g.t); };
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[j][v] = 0.f;
    auto tile = [&]() { mfma_tile<true, true, BM, BN>(As, Bs, g.wm0, 0, g.r, g.h, reinterpret_cast<f32x16 (&)[1][2]>(acc)); };
    F32_KLOOP(true, 0, ktiles, gload, lstore, tile);       // K >= 1: every entry refuses D < 1
}

// One pair of the tile as its thread holds it: accumulator register v, (row, col) in the block's 128 x 64 tile, (gi, gj) in
// the two sets.
struct KnnPair { int v, row, col, gi, gj; };

// The walk over a thread's 32 dot products of the tile at column bn0: column(col, gj) once for each of its two columns
// (that column's norm, label, ...: whatever the kernel reads per column), then pair(dot, KnnPair, that value) for the 16
// rows of the column.  The barrier at the end is every tile kernel's: what the pairs stored into LDS (the distances,
// sd[row][col]) is whole for the wave walks that follow, and every wave is past its last MFMA read of the LDS operand
// tiles before the next tile's stores.  All waves must call it.
template <class Column, class Pair>
__device__ __forceinline__ void knn_tile_walk(const KnnBlock& g, int bn0, const f32x16 (&acc)[2], Column&& column, Pair&& pair) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = j * 32 + g.r, gj = bn0 + col;
        const auto cv = column(col, gj);
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int row = g.row(v);
            pair(acc[j][v], KnnPair{v, row, col, g.bm0 + row, gj}, cv);
        }
    }
    __syncthreads();
}

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
// The 16-byte buffer loads (FAST) also need the operand's extent under the buffer limit.
inline bool knn_buffer_extent(size_t bytes) { return bytes < (size_t)OOB - 256; }

// Workspace: sqq f32 [Nq], sqx f32 [Nb], cand_d f32 [chunks][Nq][k], cand_i i32 [chunks][Nq][k], each 256-aligned.  The
// slabs are sized in whole row blocks (Nq <= rb * 128), by a bound on chunks * rb that grows with Nq -- chunks * rb <=
// min(ct * rb, KNN_TARGET_BLOCKS - 1 + rb) -- so that the size is monotone in every argument (chunks itself falls as Nq
// grows).  A self search (queries = bank) has the one norm array, sqx = sqq, and one size argument, so no such promise
// to keep: its slabs hold chunks * rb row blocks exactly.
inline size_t knn_min(size_t a, size_t b) { return a < b ? a : b; }
struct QueryWs {
    float* sqq;
    float* sqx;
    float* cand_d;
    int* cand_i;
    size_t bytes;
};
inline QueryWs query_layout(void* ws, long Nq, long Nb, int k, bool self) {
    const QueryPlan pl = query_plan(Nq, Nb);
    const size_t blocks = self ? (size_t)pl.chunks * pl.rb : knn_min((size_t)pl.ct * pl.rb, (size_t)KNN_TARGET_BLOCKS - 1 + pl.rb);
    const size_t sqq = align256((size_t)Nq * 4), sqx = self ? 0 : align256((size_t)Nb * 4);
    const size_t cand = align256(blocks * KNN_BM * (size_t)k * 4);
    char* p = static_cast<char*>(ws);
    QueryWs w;
    w.sqq = reinterpret_cast<float*>(p);
    w.sqx = self ? w.sqq : reinterpret_cast<float*>(p + sqq);
    w.cand_d = reinterpret_cast<float*>(p + sqq + sqx);
    w.cand_i = reinterpret_cast<int*>(p + sqq + sqx + cand);
    w.bytes = sqq + sqx + 2 * cand;
    return w;
}

struct QueryP {
    KnnOperand Q, X;            // a self search reads Q and sqq alone
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
// query's list (registers: lane j holds entry j).  A column outside the bank, the one a query excludes, or a pair
// without a distance (a bad row on either side, see knn_distance) is offered as (+inf, no index): it is never
// inserted, so a bad bank row is in no list and a bad query's list stays empty.  At the end the lists go to the
// chunk's candidate slab.
// SELF: the bank is the queries (both operands and both norms are read through Q's pointers), nothing is excluded, and
// row i against itself gets distance -1: it sorts before every real distance (>= 0) and the merge writes it out as 0, so
// row i comes first even when a duplicate of it has a lower index.  What SELF turns off is compiled out.
template <bool FAST, bool SELF>
__global__ __launch_bounds__(KNN_THREADS) void knn_tile_kernel(const QueryP p) {
    constexpr int BM = KNN_BM, BN = KNN_BN;
    __shared__ __attribute__((aligned(16))) float lds[(BM + BN) * 36];
    __shared__ float sd[BM][BN + 1];

    const KnnBlock g(p.ct, p.chunks);
    const int lane = g.lane, wm0 = g.wm0, bm0 = g.bm0;
    const KnnOperand& X = SELF ? p.Q : p.X;
    const float* sqx = SELF ? p.sqq : p.sqx;
    const int Nq = p.Q.rows, Nb = X.rows;

    float ld_[32];
    int li_[32];
#pragma unroll
    for (int rr = 0; rr < 32; ++rr) { ld_[rr] = INFINITY; li_[rr] = 0x7fffffff; }

    // the bank row (of this call) each of the wave's queries must not receive: lane rr holds query wm0 + rr's, -1 = none
    int excl = -1;
    if constexpr (!SELF) {
        if (p.exclude && lane < 32 && bm0 + wm0 + lane < Nq) {
            const int64_t e = p.exclude[bm0 + wm0 + lane] - p.index_base;
            if (e >= 0 && e < Nb) excl = (int)e;
        }
    }

    KnnStage<FAST> st;
    st.point(p.Q, X);
    st.rows_a(p.Q, bm0, g.t);

    for (int ctile = g.ct0; ctile < g.ct1; ++ctile) {
        const int bn0 = ctile * BN;
        f32x16 acc[2];
        knn_tile_dots<FAST>(st, g, p.Q, X, bn0, p.D, lds, acc);
        knn_tile_walk(
            g, bn0, acc, [&](int, int gj) { return gj < Nb ? sqx[gj] : 0.f; },
            [&](float dot, const KnnPair& c, float sj) {
                float d = INFINITY;
                if (c.gi < Nq && c.gj < Nb) d = SELF && c.gi == c.gj ? -1.f : knn_distance(dot, p.sqq[c.gi], sj, p.metric);
                sd[c.row][c.col] = d;
            });
        const int gj = bn0 + lane;
#pragma unroll
        for (int rr = 0; rr < 32; ++rr) {
            bool ok = gj < Nb;
            // by every lane, never under a run-time branch: a shuffle under `gj < Nb` would read inactive lanes as 0
            if constexpr (!SELF) ok &= gj != __shfl(excl, rr, 64);
            const float cd = sd[wm0 + rr][lane];
            ok &= cd == cd;     // a pair without a distance (knn_distance) is offered like a column outside the bank
            knn_insert(ld_[rr], li_[rr], ok ? cd : INFINITY, ok ? gj : 0x7fffffff, p.k, lane);
        }
    }
#pragma unroll
    for (int rr = 0; rr < 32; ++rr) {
        const int gi = bm0 + wm0 + rr;
        if (gi < Nq && lane < p.k) {
            const size_t o = ((size_t)g.chunk * Nq + gi) * (unsigned)p.k + lane;        // k >= 1: unsigned, a 32 x 32-bit multiply
            p.cand_d[o] = ld_[rr];
            p.cand_i[o] = li_[rr];
        }
    }
}

// One wave per query: the list already in (idx, dist) when `accumulate` (an entry with idx < 0 is an empty slot), then
// the per-chunk lists in chunk order, folded into the k smallest by (distance, global ordinal).  Empty slots leave as
// (+inf, -1).  `self`: the tile kernel's -1 of row i against itself leaves as 0.
__global__ __launch_bounds__(KNN_MERGE_ROWS * 64) void knn_merge_kernel(const float* __restrict__ cand_d,
                                                                        const int* __restrict__ cand_i, int Nq, int k,
                                                                        int chunks, int64_t index_base, int accumulate,
                                                                        int self, int64_t* __restrict__ idx,
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
        dist[(size_t)i * k + lane] = empty ? INFINITY : self ? fmaxf(ld, 0.f) : ld;
    }
}

// The search behind both entry points, arguments already checked: the norms, the tile kernel over (row blocks, chunks),
// the merge.  self: X is Q.  The 16-byte buffer loads (FAST) need D, both strides and both pointers 16-byte aligned and
// both extents under the buffer limit; anything else takes the element-wise loads, which feed the same values.
int knn_search(const char* name, bool self, const float* Q, long ldq, long Nq, const float* X, long ldx, long Nb, int D, int k,
               int metric, int64_t index_base, int accumulate, const int64_t* exclude, int64_t* idx, float* dist, void* ws,
               vsom_stream_t stream) {
    const QueryPlan pl = query_plan(Nq, Nb);
    const QueryWs w = query_layout(ws, Nq, Nb, k, self);
    VSOM_LAUNCH(knn_sqnorm_kernel, dim3(cdiv(Nq, 256)), dim3(256), 0, stream, Q, ldq, Nq, D, w.sqq);
    if (!self) VSOM_LAUNCH(knn_sqnorm_kernel, dim3(cdiv(Nb, 256)), dim3(256), 0, stream, X, ldx, Nb, D, w.sqx);
    const bool qvec = D % 4 == 0 && ldq % 4 == 0 && aligned16(Q), xvec = D % 4 == 0 && ldx % 4 == 0 && aligned16(X);
    const size_t qext = (size_t)Nq * ldq * 4, xext = (size_t)Nb * ldx * 4;
    QueryP p = {};
    p.Q = {Q, ldq, (int)Nq, (unsigned)qext, qvec};
    p.X = {X, ldx, (int)Nb, (unsigned)xext, xvec};
    p.D = D; p.k = k; p.metric = metric; p.sqq = w.sqq; p.sqx = w.sqx; p.exclude = exclude; p.index_base = index_base;
    p.cand_d = w.cand_d; p.cand_i = w.cand_i; p.ct = pl.ct; p.chunks = pl.chunks;
    const bool fast = qvec && xvec && knn_buffer_extent(qext) && knn_buffer_extent(xext);
    const dim3 grid(pl.rb, pl.chunks), block(KNN_THREADS);
    if (self) {
        if (fast) VSOM_LAUNCH((knn_tile_kernel<true, true>), grid, block, 0, stream, p);
        else VSOM_LAUNCH((knn_tile_kernel<false, true>), grid, block, 0, stream, p);
    } else {
        if (fast) VSOM_LAUNCH((knn_tile_kernel<true, false>), grid, block, 0, stream, p);
        else VSOM_LAUNCH((knn_tile_kernel<false, false>), grid, block, 0, stream, p);
    }
    VSOM_LAUNCH(knn_merge_kernel, dim3(cdiv(Nq, KNN_MERGE_ROWS)), dim3(KNN_MERGE_ROWS * 64), 0, stream,
                (const float*)w.cand_d, (const int*)w.cand_i, (int)Nq, k, pl.chunks, index_base, accumulate, (int)self, idx,
                dist);
    return launch_status(name);
}

// ---------------------------------------------------------------------------------------------- neighbour ranks
// A slot as the tile kernel reads it: the threshold d(i, n) and the neighbour n as a row of this launch (-1: nothing to count).
struct RankSlot {
    float thr;
    int nb;
};
// Workspace of vsom_knn_ranks: sq f32 [N], slot RankSlot [N][k], each 256-aligned.
struct RankWs {
    float* sq;
    RankSlot* slot;
    size_t bytes;
};
inline RankWs rank_layout(void* ws, long N, int k) {
    const size_t sq = align256((size_t)N * 4), slots = align256((size_t)N * k * sizeof(RankSlot));
    char* p = static_cast<char*>(ws);
    RankWs w;
    w.sq = reinterpret_cast<float*>(p);
    w.slot = reinterpret_cast<RankSlot*>(p + sq);
    w.bytes = sq + slots;
    return w;
}

// <x, y> over D in the order in which mfma_tile sums that pair (see knn_sqnorm_row): bit for bit the tile's value.
template <bool VEC>
__device__ __forceinline__ float knn_pair_dot(const float* __restrict__ x, const float* __restrict__ y, int D) {
    float s = 0.f;
#pragma unroll 2
    for (int kb = 0; kb < D; kb += 8) {
        float a[8], b[8];
        if constexpr (VEC) {                                         // D % 4 == 0: a group is whole or its upper half is missing
            const bool hi = kb + 4 < D;
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            const f32x4 a0 = *reinterpret_cast<const f32x4*>(x + kb), b0 = *reinterpret_cast<const f32x4*>(y + kb);
            const f32x4 a1 = hi ? *reinterpret_cast<const f32x4*>(x + kb + 4) : z;
            const f32x4 b1 = hi ? *reinterpret_cast<const f32x4*>(y + kb + 4) : z;
#pragma unroll
            for (int j = 0; j < 4; ++j) { a[j] = a0[j]; b[j] = b0[j]; a[4 + j] = a1[j]; b[4 + j] = b1[j]; }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                a[j] = kb + j < D ? x[kb + j] : 0.f;
                b[j] = kb + j < D ? y[kb + j] : 0.f;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            s = fmaf(a[j], b[j], s);
            s = fmaf(a[4 + j], b[4 + j], s);
        }
    }
    return s;
}

// One thread per slot (i, j): the threshold d(i, nbr[i][j]) exactly as the tile kernel will compute that pair, the
// neighbour as a row of this launch, and the slot's two counters at their start value.  A slot that is empty (-1),
// names row i itself or lies outside [0, N) never reads A: threshold NaN (no distance is below or equal to it),
// neighbour -1, counters -1 for good.  So does a slot whose pair has no distance (a bad row, see knn_distance); and as
// the tile kernel's distance to a bad row is NaN as well, such a row is counted for no slot of any other row.
template <bool VEC>
__global__ __launch_bounds__(256) void knn_rank_threshold_kernel(const float* __restrict__ A, long lda, long N, int D, int k,
                                                                int metric, const int64_t* __restrict__ nbr,
                                                                const float* __restrict__ sq, RankSlot* __restrict__ out,
                                                                int* __restrict__ less, int* __restrict__ tied) {
    const size_t slot = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (slot >= (size_t)N * k) return;
    const long i = (long)(slot / k);
    const int64_t n = nbr[slot];
    if (n < 0 || n >= N || n == i) {
        out[slot] = {__builtin_nanf(""), -1};
        less[slot] = -1;
        tied[slot] = -1;
        return;
    }
    const float dot = knn_pair_dot<VEC>(A + i * lda, A + n * lda, D);
    const float thr = knn_distance(dot, sq[i], sq[n], metric);
    const bool ok = thr == thr;                                      // a bad row on either side: nothing to count either
    out[slot] = {thr, ok ? (int)n : -1};
    less[slot] = ok ? 0 : -1;
    tied[slot] = ok ? 0 : -1;
}

// The load path of a set contracted with itself (vsom_knn_ranks, vsom_dbscan_neighbours): 16 bytes per lane, or
// element-wise loads that feed the same values.  One decision for both entries.
inline bool knn_self_vec(const float* A, long lda, int D) {
    const bool vec = D % 4 == 0 && lda % 4 == 0 && aligned16(A);
    return vec;
}

// What every tile kernel over a set contracted with itself reads: the head of its parameter struct.
struct SelfP {
    KnnOperand A;
    int D, metric;
    const float* sq;            // [N] squared norms in the contraction's order
    int ct, chunks;             // query_plan(N, N)
};

// The launch of a self-contraction's tile kernel, its own parameters already in p: fills the head from the set and its
// plan and launches TILE_FAST or TILE_GENERIC (the kernel's <true> and <false>) over (row blocks, chunks).  vec is the
// caller's decision on the pointer and the strides (knn_self_vec, or the entry's own line).  Returns the plan it launched.
template <class P, void (*TILE_FAST)(P), void (*TILE_GENERIC)(P)>
QueryPlan knn_self_launch(P p, const float* X, long ld, long N, int D, int metric, const float* sq, bool vec, vsom_stream_t stream) {
    const QueryPlan pl = query_plan(N, N);
    const size_t ext = (size_t)N * ld * 4;
    p.A = {X, ld, (int)N, (unsigned)ext, vec};
    p.D = D; p.metric = metric; p.sq = sq; p.ct = pl.ct; p.chunks = pl.chunks;
    const dim3 grid(pl.rb, pl.chunks), block(KNN_THREADS);
    if (vec && knn_buffer_extent(ext)) VSOM_LAUNCH(TILE_FAST, grid, block, 0, stream, p);
    else VSOM_LAUNCH(TILE_GENERIC, grid, block, 0, stream, p);
    return pl;
}

struct RankP : SelfP {
    int k;
    const RankSlot* slot;       // [N][k]
    int* less;                  // [N][k], 0 (or -1) on entry
    int* tied;
};

// One workgroup = 128 rows x one chunk of column tiles (KnnBlock), like knn_tile_kernel<., SELF>.  Per 64-column tile: the
// 128 x 64 block of A A^T (knn_tile_dots), the distances into LDS -- NaN for a column outside the set and for row i
// against itself, so neither is ever counted -- then every wave walks each of its 32 rows' 64 distances: lane j < k
// holds slot j's threshold and neighbour, all lanes read the same LDS word (a broadcast), and two integer counters per
// lane take d < threshold and d == threshold; the neighbour's own column is walked with the others and taken out again
// by one read of its word when it falls into the tile.  At the end the counters are added into less / tied with integer
// atomics: the result does not depend on the chunking or on the order of arrival.
template <bool FAST>
__global__ __launch_bounds__(KNN_THREADS, 2) void knn_rank_tile_kernel(const RankP p) {
    constexpr int BM = KNN_BM, BN = KNN_BN;
    __shared__ __attribute__((aligned(16))) float lds[(BM + BN) * 36];
    __shared__ float sd[BM][BN + 1];

    const KnnBlock g(p.ct, p.chunks);
    const int lane = g.lane, wm0 = g.wm0, bm0 = g.bm0;
    const int N = p.A.rows;

    // lane j < k of the wave holds slot j of each of its 32 rows: the two counters stay in registers over the chunk, the
    // threshold and the neighbour are read again for every tile (keeping them too would cost the second workgroup per CU)
    int ls_[32], td_[32];
#pragma unroll
    for (int rr = 0; rr < 32; ++rr) { ls_[rr] = 0; td_[rr] = 0; }
    const bool mine = lane < p.k;
    const int wrow0 = __builtin_amdgcn_readfirstlane(bm0 + wm0);     // the wave's first row, known to be wave-uniform
    const RankSlot* slots = p.slot + (size_t)wrow0 * p.k;

    KnnStage<FAST> st;
    st.point(p.A, p.A);
    st.rows_a(p.A, bm0, g.t);

    for (int ctile = g.ct0; ctile < g.ct1; ++ctile) {
        const int bn0 = ctile * BN;
        f32x16 acc[2];
        knn_tile_dots<FAST>(st, g, p.A, p.A, bn0, p.D, lds, acc);
        knn_tile_walk(
            g, bn0, acc, [&](int, int gj) { return gj < N ? p.sq[gj] : 0.f; },
            [&](float dot, const KnnPair& c, float sj) {
                float d = __builtin_nanf("");
                if (c.gi < N && c.gj < N && c.gi != c.gj) d = knn_distance(dot, p.sq[c.gi], sj, p.metric);
                sd[c.row][c.col] = d;
            });
        RankSlot sl_[32];
        int off = lane;
        asm volatile("" : "+v"(off));                                // computed per tile: 32 hoisted addresses cost the occupancy
#pragma unroll
        for (int rr = 0; rr < 32; ++rr) {
            const bool ok = mine && wrow0 + rr < N;
            sl_[rr] = ok ? slots[rr * p.k + off] : RankSlot{__builtin_nanf(""), -1};
        }
#pragma unroll
        for (int rr = 0; rr < 32; ++rr) {
            const float* row = sd[wm0 + rr];
            const float th = sl_[rr].thr;
            const int skip = sl_[rr].nb - bn0;                          // the neighbour's column of this tile, if it is one
            int ls = 0, td = 0;
#pragma unroll 8
            for (int c = 0; c < BN; ++c) {
                const float d = row[c];
                ls += d < th;
                td += d == th;
            }
            if (skip >= 0 && skip < BN) {                            // the neighbour's own column was walked too: take it out
                const float d = row[skip];
                ls -= d < th;
                td -= d == th;
            }
            ls_[rr] += ls;
            td_[rr] += td;
        }
    }
#pragma unroll
    for (int rr = 0; rr < 32; ++rr) {
        // a slot with nothing to count (threshold NaN) has counted nothing: its -1 stays
        if (wrow0 + rr < N && mine) {
            const size_t o = (size_t)(wrow0 + rr) * p.k + lane;
            if (ls_[rr]) atomicAdd(&p.less[o], ls_[rr]);
            if (td_[rr]) atomicAdd(&p.tied[o], td_[rr]);
        }
    }
}

// ---------------------------------------------------------------------------------------------- silhouette
// The same contraction of a set with itself, summing instead of counting: S[i][c] = the sum over the members j != i of
// cluster c of d(i, j), in fixed point.  Nothing of size N x N exists.
//
// The fixed-point unit.  With M the largest squared norm of the counted rows (an integer atomic max on ordered_key, read
// back by the kernels: it never visits the host) the bound is 2^e, the smallest power of two with 2^e > 4 sqrt(M):
// frexpf gives M < 2^x, so e = ceil((x + 4) / 2).  No euclidean distance of the set reaches it.  In exact arithmetic
// d <= |x_i| + |x_j| <= 2 sqrt(M).  As computed, d^2 = fl(s_i + s_j - 2 dot) with s <= M, and the fp32 dot product is off
// by at most g sum |a_k b_k| <= g |x_i| |x_j| with g = D u / (1 - D u), u = 2^-24, while the true squared norms are at
// most M / (1 - g): |dot| <= M (1 + g) / (1 - g) <= 2 M for D <= 2^22 (g <= 1/3).  So d^2 <= 6 M (1 + u)^3 < 8 M and
// d <= sqrtf(8 M) (1 + u) < 2.83 sqrt(M) (1 + u) < 4 sqrt(M): the factor 2 over the exact bound is the headroom, and the
// rounding uses less than half of it.  The cosine distance is at most 2 up to a few ulp (1 - dot / (|x_i| |x_j|) with
// the quotient within a few ulp of [-1, 1]); its bound is 4, e = 2, the same factor.  A distance becomes
// q = llrint((double)d * 2^(40 - e)) < 2^40, so a row's sum over fewer than 2^22 columns stays below 2^62: no 64-bit sum
// can wrap (SIL_MAX_N).  The proof is not what keeps the sums in range, though: a distance that is not below the bound
// (D > 2^22, a NaN, an overflowed norm) is treated as non-finite -- it adds nothing and is counted in status[1].
//
// Integer sums do not depend on the order of their terms and a pair's distance does not depend on where it falls in a
// tile (the contract above): every output is bit for bit independent of the chunking and of the order of the rows.
constexpr long SIL_MAX_N = (1L << 22) - 1;      // N 2^41 < 2^63
constexpr int SIL_FRAC = 40;                    // fractional bits of a distance relative to the bound 2^e
constexpr int SIL_ROWS = 4;                     // rows per finishing workgroup (one wave each)
constexpr int SIL_SEG = 128;                    // k-values per summation segment: four 32-wide k-tiles

// Segmented sums.  One fp32 chain over D products leaves a squared norm off by about 0.6 sqrt(D) 2^-24 relative (4e-6 at
// D = 12 288, 6e-7 at D = 256) -- one factor on every cosine of the row, a shift of all its distances that a mean over a
// cluster does not average away: s was off by 5e-7 at D = 12 288 and, on latents whose cosine distances are 1e-4, by
// 4.7e-5 at D = 256.  The silhouette therefore sums every pair, and every norm, segment by segment: SIL_SEG k-values in the
// order of knn_tile_dots (one call of it per segment, on operands that begin at the segment), then the segment sums added
// in ascending order, in fp32.  A chain's error grows with the root of its length and scales with its end value, so short
// chains of small sums win: 3.8e-8 and 2.3e-5 on the same two sets (measured; a host emulation of both orders reproduces
// all four figures).  Four k-tiles is the shortest segment in which knn_tile_dots still hides
// three of its four loads behind the matrix cores.
// What the contract gives carries over segment by segment: a pair's value does not depend on where it falls in a tile, and
// <x, x> is bit for bit the row's norm, so identical rows are still at distance exactly 0.  For D <= SIL_SEG there is one
// segment and the distance is bit for bit that of vsom_umap_knn.
__global__ __launch_bounds__(256) void sil_sqnorm_kernel(const float* __restrict__ X, long ldx, long N, int D,
                                                        float* __restrict__ sq) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float* x = X + i * ldx;
    float s = knn_sqnorm_row(x, D < SIL_SEG ? D : SIL_SEG);
    for (int k0 = SIL_SEG; k0 < D; k0 += SIL_SEG) s += knn_sqnorm_row(x + k0, D - k0 < SIL_SEG ? D - k0 : SIL_SEG);
    sq[i] = s;
}

// Workspace of vsom_silhouette, each section 256-aligned: S u64 [N][C] FIRST (a caller may read the sums there), acc i64
// [C + 1] (the fixed-point silhouette sums per cluster, the total last), ctrl u32 [64] ([0]: key of the largest squared
// norm), sq f32 [N].  S, acc and ctrl are cleared by one launch.
struct SilWs {
    unsigned long long* S;
    unsigned long long* acc;
    unsigned* ctrl;
    float* sq;
    size_t clear_words, bytes;
};
inline SilWs sil_layout(void* ws, long N, int C) {
    const size_t s = align256((size_t)N * C * 8), acc = align256(((size_t)C + 1) * 8), ctrl = 256, sq = align256((size_t)N * 4);
    char* p = static_cast<char*>(ws);
    SilWs w;
    w.S = reinterpret_cast<unsigned long long*>(p);
    w.acc = reinterpret_cast<unsigned long long*>(p + s);
    w.ctrl = reinterpret_cast<unsigned*>(p + s + acc);
    w.sq = reinterpret_cast<float*>(p + s + acc + ctrl);
    w.clear_words = (s + acc + ctrl) / 8;
    w.bytes = s + acc + ctrl + sq;
    return w;
}

__device__ __forceinline__ bool sil_label_ok(int64_t l, int C) { return l >= 0 && l < C; }

// The exponent e of the bound 2^e (see above) from the key of the largest squared norm; key 0: no counted row.
__device__ __forceinline__ int sil_bound_exp(unsigned key, int metric) {
    if (metric == VSOM_DIST_COSINE) return 2;
    const float M = key ? ordered_key_value(key) : 0.f;
    if (!(M < INFINITY)) return 66;             // an overflowed or NaN norm: every distance to that row is refused anyway
    if (M == 0.f) return 0;
    int x;
    frexpf(M, &x);                              // M = f 2^x, f in [0.5, 1)
    return (x + 5) >> 1;                        // ceil((x + 4) / 2), x in [-148, 128]
}

__global__ __launch_bounds__(256) void sil_clear_kernel(unsigned long long* __restrict__ words, size_t n_words,
                                                       unsigned long long* __restrict__ counts, int C,
                                                       unsigned long long* __restrict__ status) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_words; i += stride) words[i] = 0;
    for (size_t c = (size_t)blockIdx.x * 256 + threadIdx.x; c < (size_t)C; c += stride) counts[c] = 0;
    if (blockIdx.x == 0 && threadIdx.x < 4) status[threadIdx.x] = 0;
}

// One thread per row: the cluster sizes, the rows whose label is outside [0, C) (status[0]; they count for nothing, not
// even for the bound), and the largest squared norm of the others: one integer atomic max per wave.
__global__ __launch_bounds__(256) void sil_prepare_kernel(const int64_t* __restrict__ labels, const float* __restrict__ sq, long N,
                                                         int C, unsigned long long* __restrict__ counts,
                                                         unsigned* __restrict__ ctrl, unsigned long long* __restrict__ status) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    unsigned key = 0;
    bool bad = false;
    if (i < N) {
        const int64_t l = labels[i];
        if (sil_label_ok(l, C)) {
            atomicAdd(&counts[l], 1ull);
            const float s = sq[i];
            key = ordered_key(s < INFINITY ? s : INFINITY);          // a NaN norm sorts as +inf
        } else {
            bad = true;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned other = __shfl_xor(key, o, 64);
        key = other > key ? other : key;
    }
    const int n_bad = __popcll(__ballot(bad));
    if ((threadIdx.x & 63) == 0) {
        if (key) atomicMax(&ctrl[0], key);
        if (n_bad) atomicAdd(&status[0], (unsigned long long)n_bad);
    }
}

struct SilP : SelfP {
    int C;
    const int64_t* labels;
    const unsigned* ctrl;
    unsigned long long* S;          // [N][C]
    unsigned long long* status;
};

// One workgroup = 128 rows x one chunk of column tiles (KnnBlock).  Per 64-column tile: the labels
// of its columns into LDS (once; -1 for a column outside the set or the range), the 128 x 64 block of A A^T
// (knn_tile_dots), the distances into LDS -- 0 for a pair that adds nothing: (i, i), a row or column that is not
// counted, a distance that is refused -- then every wave walks its 32 rows with lane = column: the distance becomes
// fixed point, a segmented suffix sum over the runs of equal adjacent labels leaves each run's total in its first lane,
// and only those lanes issue an atomic, S[i][label] += total.  Integer additions all the way: any tree, any order of
// arrival and any chunking give the same sums.
template <bool FAST>
__global__ __launch_bounds__(KNN_THREADS, 2) void sil_tile_kernel(const SilP p) {
    constexpr int BM = KNN_BM, BN = KNN_BN;
    __shared__ __attribute__((aligned(16))) float lds[(BM + BN) * 36];
    __shared__ float sd[BM][BN + 1];
    __shared__ int collab[2][BN];           // by tile parity: wave 0 writes the next tile's while others still read this one's
    __shared__ int rowlab[BM];
    __shared__ float rowsq[BM];

    const KnnBlock g(p.ct, p.chunks);
    const int t = g.t, lane = g.lane, wm0 = g.wm0, bm0 = g.bm0;
    const int N = p.A.rows;

    const int e = sil_bound_exp(p.ctrl[0], p.metric);
    const float bound = ldexpf(1.f, e);
    const double scale = ldexp(1.0, SIL_FRAC - e);
    if (t < BM) {
        const int gi = bm0 + t;
        int l = -1;
        float s = 0.f;
        if (gi < N) {
            const int64_t v = p.labels[gi];
            if (sil_label_ok(v, p.C)) l = (int)v;
            s = p.sq[gi];
        }
        rowlab[t] = l;
        rowsq[t] = s;
    }
    int refused = 0;

    KnnStage<FAST> st;
    st.point(p.A, p.A);
    st.rows_a(p.A, bm0, t);      // the row offsets of the 128 A rows: once per workgroup

    for (int ctile = g.ct0; ctile < g.ct1; ++ctile) {
        const int bn0 = ctile * BN;
        const int par = (ctile - g.ct0) & 1;
        if (t < BN) {
            const int gj = bn0 + t;
            int l = -1;
            if (gj < N) {
                const int64_t v = p.labels[gj];
                if (sil_label_ok(v, p.C)) l = (int)v;
            }
            collab[par][t] = l;
        }
        f32x16 acc[2];
        for (int k0 = 0; k0 < p.D; k0 += SIL_SEG) {                         // segment by segment, see SIL_SEG
            const KnnOperand seg = {p.A.base + k0, p.A.ld, p.A.rows, p.A.bytes - 4u * (unsigned)k0, p.A.vec};
            const int len = p.D - k0 < SIL_SEG ? p.D - k0 : SIL_SEG;
            st.point(seg, seg);
            if (k0 == 0) {
                knn_tile_dots<FAST>(st, g, seg, seg, bn0, len, lds, acc);      // its barriers publish collab (and rowlab, rowsq)
            } else {
                f32x16 part[2];
                __syncthreads();                                            // every wave is past its reads of the LDS tiles
                knn_tile_dots<FAST>(st, g, seg, seg, bn0, len, lds, part);
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int v = 0; v < 16; ++v) acc[j][v] += part[j][v];
            }
        }

        struct Column { bool ok; float sq; };
        knn_tile_walk(
            g, bn0, acc,
            [&](int col, int gj) {
                const bool ok = collab[par][col] >= 0;
                return Column{ok, ok ? p.sq[gj] : 0.f};
            },
            [&](float dot, const KnnPair& c, const Column& cj) {
                float d = 0.f;
                if (cj.ok && rowlab[c.row] >= 0 && c.gi != c.gj) {
                    const float si = rowsq[c.row];
                    d = knn_distance(dot, si, cj.sq, p.metric);
                    // a pair without a distance is NaN (knn_distance) and fails d < bound; the norms are tested as well
                    if (!(si < INFINITY && cj.sq < INFINITY && d < bound)) { ++refused; d = 0.f; }
                }
                sd[c.row][c.col] = d;
            });

        const int lab = collab[par][lane];
        const int prev = __shfl_up(lab, 1, 64);
        const unsigned long long heads = __ballot(lane == 0 || lab != prev);
        const unsigned long long above = heads & ~((2ull << lane) - 1ull);          // the run heads after this lane
        const int last = above ? __builtin_ctzll(above) - 1 : 63;                    // the last lane of this lane's run
        const bool issue = ((heads >> lane) & 1) && lab >= 0;
#pragma unroll 4
        for (int rr = 0; rr < 32; ++rr) {
            // 2^52 + d 2^(40 - e) in one rounding (the product is exact: 24 bits times a power of two; it is below 2^40):
            // round-to-nearest-even leaves llrint(d 2^(40 - e)) in the low mantissa bits
            const double y = fma((double)sd[wm0 + rr][lane], scale, 0x1p52);
            unsigned long long q = (unsigned long long)__double_as_longlong(y) & 0xFFFFFFFFFFFFFull;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned long long up = __shfl_down(q, o, 64);
                if (lane + o <= last) q += up;
            }
            if (issue && q && rowlab[wm0 + rr] >= 0) atomicAdd(&p.S[(size_t)(bm0 + wm0 + rr) * p.C + lab], q);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) refused += __shfl_xor(refused, o, 64);
    if (lane == 0 && refused) atomicAdd(&p.status[1], (unsigned long long)refused);
}

struct SilOut {
    double* sil;
    double* a;
    double* b;
    int64_t* nearest;
};

// One wave per row, from S and the cluster sizes, in fp64 with contraction off: each of a, b and s is an exact
// conversion-and-scale followed by one correctly rounded division (s: a subtraction and a division).
//   a = S[i][own] unit / (n_own - 1);  b = min over the other non-empty clusters of S[i][c] unit / n_c, the lowest
//   cluster on a tie;  s = (b - a) / max(a, b), 0 for a singleton cluster and where max(a, b) = 0 (sklearn's nan_to_num),
//   0 too with no other non-empty cluster (b NaN, nearest -1).  A row whose label is out of range: NaN, NaN, NaN, -1.
// The row's s goes into its cluster's and the total's sum as llrint(s 2^40): integer sums again, so the means do not
// depend on the order of the rows either (2^-41 per row, far below what fp32 distances resolve).
__global__ __launch_bounds__(SIL_ROWS * 64) void sil_finish_kernel(const unsigned long long* __restrict__ S,
                                                                   const unsigned long long* __restrict__ counts,
                                                                   const int64_t* __restrict__ labels, long N, int C,
                                                                   const unsigned* __restrict__ ctrl, int metric, SilOut out,
                                                                   unsigned long long* __restrict__ acc) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * SIL_ROWS + (threadIdx.x >> 6);
    if (i >= N) return;
    const int64_t own = labels[i];
    if (!sil_label_ok(own, C)) {
        if (lane == 0) {
            const double nan = __builtin_nan("");
            out.sil[i] = nan;
            if (out.a) out.a[i] = nan;
            if (out.b) out.b[i] = nan;
            if (out.nearest) out.nearest[i] = -1;
        }
        return;
    }
    const double unit = ldexp(1.0, sil_bound_exp(ctrl[0], metric) - SIL_FRAC);
    const unsigned long long* row = S + (size_t)i * C;
    double best = INFINITY;
    int arg = 0x7fffffff;
    for (int c = lane; c < C; c += 64) {
        const unsigned long long n = counts[c];
        if (c == own || n == 0) continue;
        const double v = (double)row[c] * unit / (double)n;
        if (v < best) { best = v; arg = c; }           // ascending c: the first minimum of this lane's clusters
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o, 64);
        const int oa = __shfl_xor(arg, o, 64);
        if (ob < best || (ob == best && oa < arg)) { best = ob; arg = oa; }
    }
    if (lane) return;
    const unsigned long long n_own = counts[own];
    const bool other = arg != 0x7fffffff;
    const double a = n_own > 1 ? (double)row[own] * unit / (double)(n_own - 1) : 0.0;
    const double b = other ? best : __builtin_nan("");
    double s = 0.0;
    if (n_own > 1 && other) {
        const double m = a > b ? a : b;
        if (m > 0.0) s = (b - a) / m;
    }
    out.sil[i] = s;
    if (out.a) out.a[i] = a;
    if (out.b) out.b[i] = b;
    if (out.nearest) out.nearest[i] = other ? arg : -1;
    const unsigned long long q = (unsigned long long)llrint(ldexp(s, SIL_FRAC));     // two's complement: the sums are signed
    if (q) {
        atomicAdd(&acc[own], q);
        atomicAdd(&acc[C], q);
    }
}

// One workgroup: the cluster means and the score from the integer sums, the two cluster counts of status.
__global__ __launch_bounds__(256) void sil_means_kernel(const unsigned long long* __restrict__ acc,
                                                       const unsigned long long* __restrict__ counts, long N, int C,
                                                       double* __restrict__ cluster_mean, double* __restrict__ score,
                                                       unsigned long long* __restrict__ status) {
#pragma clang fp contract(off)
    __shared__ unsigned tally[2];
    if (threadIdx.x < 2) tally[threadIdx.x] = 0;
    __syncthreads();
    unsigned present = 0, single = 0;
    for (int c = threadIdx.x; c < C; c += 256) {
        const unsigned long long n = counts[c];
        present += n > 0;
        single += n == 1;
        if (cluster_mean) cluster_mean[c] = n ? ldexp((double)(long long)acc[c], -SIL_FRAC) / (double)n : __builtin_nan("");
    }
    if (present) atomicAdd(&tally[0], present);
    if (single) atomicAdd(&tally[1], single);
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long counted = (unsigned long long)N - status[0];
        score[0] = counted ? ldexp((double)(long long)acc[C], -SIL_FRAC) / (double)counted : __builtin_nan("");
        status[2] = tally[0];
        status[3] = tally[1];
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
        // exp(-(d - d_min) / T), d_min the query's smallest valid distance: the scores up to the common factor
        // exp(d_min / T).  Unshifted, euclidean distances of latent width (d > 52 at T = 0.07) underflow every weight
        // to 0 and the first argmax answers class 0.  The nearest valid neighbour weighs exactly 1.
        float dmin = valid ? d : INFINITY;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) dmin = fminf(dmin, __shfl_xor(dmin, o, 64));
        w = exp(-((double)d - (double)dmin) / (double)p.temperature);
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

// ---------------------------------------------------------------------------------------------- DBSCAN
// The same contraction of a set with itself a fourth time, thresholding instead of selecting, counting or summing: the
// eps-neighbourhood graph of DBSCAN (Ester et al. 1996; sklearn.cluster.DBSCAN) as a bit matrix, then the connected
// components of its core rows and sklearn's labels (vit_som_amd/dbscan.py; no counterpart in the reference).
//
// The bit contract (adj u64 [N][W], W = ceil(N / 64)):
//   - bit (j & 63) of adj[i][j >> 6] is set iff rows i and j have a distance and (double)d <= eps, d bit for bit the fp32
//     distance of vsom_umap_knn for that pair (euclidean with the root, cosine), eps the caller's double;
//   - the diagonal is set: a row is in its own neighbourhood, as in sklearn;
//   - bits of columns >= N are clear;
//   - a bad row (the contract at knn_distance; decided per row by dbscan_row_ok, so that a row without a distance to
//     itself has none to anyone) has no bit set anywhere, in its row or in its column, and is counted in status[0];
//   - a pair's value does not depend on where it falls in a tile and fp32 addition commutes: the matrix is symmetric bit
//     for bit.
// The tile kernel walks the 128 x 64 distance tile with lane = column, so one wave64 ballot IS word adj[i][tile].  The column
// chunks write disjoint words, every word exactly once: nothing is cleared beforehand, nothing is added atomically, and
// the result does not depend on the chunking.
//
// The components are int32 throughout, atomicMin is their only atomic, and nothing waits on another workgroup.
// root[i] of a core row starts at i and only ever falls, always to a core row of i's own component (a neighbour's root,
// the root's root).  A hook step that moves nothing has read a state in which root is constant along every edge between
// core rows, hence over every component; that constant c is a row of the component with root[c] <= c, every root of the
// component is >= its smallest core row m, and root[m] <= m: so c = m.  The fixed point is unique -- every core row's
// root is the smallest core row of its component -- and the result does not depend on the races on the way.
constexpr long DBSCAN_MAX_N = 131072;          // N^2 / 8 = 2 GiB of bits
constexpr int DBSCAN_ROWS = 4;                 // rows per workgroup of the row-walking kernels (one wave each)
constexpr int DBSCAN_SCAN = 1024;              // threads of the one-workgroup passes over the rows

// A row that has a distance to itself: its squared norm is finite (euclidean: so is the squared distance 2 s - 2 s).
__device__ __forceinline__ bool dbscan_row_ok(float s, int metric) {
    return metric == VSOM_DIST_EUCLIDEAN ? s + s < INFINITY : s < INFINITY;
}

struct NeighP : SelfP {
    double eps;
    unsigned long long* adj;    // [N][ct]
};

// One workgroup = 128 rows x one chunk of column tiles (KnnBlock).  Per 64-column tile: the 128 x 64
// block of A A^T (knn_tile_dots), the distances into LDS -- NaN for a column outside the set and for a pair with a bad
// row, 0 for a good row against itself -- then every wave ballots (double)d <= eps over each of its 32 rows with
// lane = column; lane rr keeps row rr's word and stores it as adj[row][tile].  NaN is below nothing: its bit is clear.
template <bool FAST>
__global__ __launch_bounds__(KNN_THREADS, 2) void dbscan_tile_kernel(const NeighP p) {
    constexpr int BM = KNN_BM, BN = KNN_BN;
    __shared__ __attribute__((aligned(16))) float lds[(BM + BN) * 36];
    __shared__ float sd[BM][BN + 1];

    const KnnBlock g(p.ct, p.chunks);
    const int lane = g.lane, wm0 = g.wm0, bm0 = g.bm0;
    const int N = p.A.rows;

    KnnStage<FAST> st;
    st.point(p.A, p.A);
    st.rows_a(p.A, bm0, g.t);

    for (int ctile = g.ct0; ctile < g.ct1; ++ctile) {
        const int bn0 = ctile * BN;
        f32x16 acc[2];
        knn_tile_dots<FAST>(st, g, p.A, p.A, bn0, p.D, lds, acc);
        struct Column { float sq; bool ok; };
        knn_tile_walk(
            g, bn0, acc,
            [&](int, int gj) {
                const float sj = gj < N ? p.sq[gj] : __builtin_nanf("");
                return Column{sj, dbscan_row_ok(sj, p.metric)};         // not ok: also a column outside the set
            },
            [&](float dot, const KnnPair& c, const Column& cj) {
                float d = __builtin_nanf("");
                if (c.gi < N && cj.ok) {
                    const float si = p.sq[c.gi];
                    if (dbscan_row_ok(si, p.metric)) d = c.gi == c.gj ? 0.f : knn_distance(dot, si, cj.sq, p.metric);
                }
                sd[c.row][c.col] = d;
            });
        unsigned long long word = 0;
#pragma unroll
        for (int rr = 0; rr < 32; ++rr) {
            const unsigned long long b = __ballot((double)sd[wm0 + rr][lane] <= p.eps);
            if (lane == rr) word = b;
        }
        const int gi = bm0 + wm0 + lane;
        if (lane < 32 && gi < N) p.adj[(size_t)gi * p.ct + ctile] = word;
    }
}

// One wave per row: count[i] = the set bits of row i (integer adds in the wave, no atomics).
__global__ __launch_bounds__(DBSCAN_ROWS * 64) void dbscan_count_kernel(const unsigned long long* __restrict__ adj, int N, int W,
                                                                        int* __restrict__ count) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * DBSCAN_ROWS + (threadIdx.x >> 6);
    if (i >= N) return;
    int c = 0;
    for (int w = lane; w < W; w += 64) c += __popcll(adj[(size_t)i * W + w]);
#pragma unroll
    for (int o = 32; o; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) count[i] = c;
}

// One workgroup: status[0] = the rows without a bit (with_bad: the bad rows -- a good row has its diagonal; else left
// alone), status[1] = the set bits of the matrix.  Per-thread sums in row order, then thread 0 adds the partial sums in
// thread order.
__global__ __launch_bounds__(DBSCAN_SCAN) void dbscan_status_kernel(const int* __restrict__ count, int N, int with_bad,
                                                                    int64_t* __restrict__ status) {
    __shared__ long long bits[DBSCAN_SCAN];
    __shared__ int bad[DBSCAN_SCAN];
    const int t = threadIdx.x;
    long long b = 0;
    int z = 0;
    for (int i = t; i < N; i += DBSCAN_SCAN) {
        const int c = count[i];
        b += c;
        z += c == 0;
    }
    bits[t] = b;
    bad[t] = z;
    __syncthreads();
    if (t == 0) {
        long long tb = 0, tz = 0;
        for (int k = 0; k < DBSCAN_SCAN; ++k) { tb += bits[k]; tz += bad[k]; }
        if (with_bad) status[0] = tz;
        status[1] = tb;
    }
}

// The same bit contract from a precomputed matrix M [N, N] (T float or double, row stride ldm).  One wave per row, lane =
// column: the ballot of (double)M[i][j] <= eps is word adj[i][j >> 6].  A NaN entry clears its bit and is counted in
// status[0] (cleared before the launch; an integer atomic, one per row that has any); the diagonal is set whatever it holds.
template <class T>
__global__ __launch_bounds__(DBSCAN_ROWS * 64) void dbscan_threshold_kernel(const T* __restrict__ M, long ldm, int N, int W, double eps,
                                                                            unsigned long long* __restrict__ adj,
                                                                            int* __restrict__ count,
                                                                            unsigned long long* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * DBSCAN_ROWS + (threadIdx.x >> 6);
    if (i >= N) return;
    const T* row = M + (size_t)i * ldm;
    int c = 0, nans = 0;
    for (int w = 0; w < W; ++w) {
        const int j = w * 64 + lane;
        const double d = j < N ? (double)row[j] : __builtin_nan("");
        const unsigned long long b = __ballot(j < N && (j == i || d <= eps));
        nans += __popcll(__ballot(j < N && d != d));
        c += __popcll(b);
        if (lane == 0) adj[(size_t)i * W + w] = b;
    }
    if (lane == 0) {
        count[i] = c;
        if (nans) atomicAdd(&status[0], (unsigned long long)nans);
    }
}
__global__ void dbscan_clear_status_kernel(int64_t* __restrict__ status) { status[threadIdx.x] = 0; }

// core[i] = count[i] >= min_samples; root[i] = i for a core row, -1 otherwise.
__global__ __launch_bounds__(256) void dbscan_init_kernel(const int* __restrict__ count, int N, int min_samples,
                                                          unsigned char* __restrict__ core, int* __restrict__ root) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const bool c = count[i] >= min_samples;
    core[i] = c;
    root[i] = c ? i : -1;
}

__global__ void dbscan_clear_changed_kernel(int* __restrict__ changed) { *changed = 0; }

// A root as another workgroup may be lowering it: one relaxed 4-byte load, so a value some atomicMin wrote or the start value.
__device__ __forceinline__ int dbscan_root(const int* root, int i) { return __atomic_load_n(root + i, __ATOMIC_RELAXED); }

// The hook step, one wave per core row, lane = column: the least root[j] over the set bits j of row i with core[j] (row
// i's own bit among them), atomicMin-ed into root[i] and into root[root[i]] when it is lower; `changed` is raised when
// anything moved.  A word without a bit is skipped (the word is wave-uniform).
__global__ __launch_bounds__(DBSCAN_ROWS * 64) void dbscan_hook_kernel(const unsigned long long* __restrict__ adj, int N, int W,
                                                                       const unsigned char* __restrict__ core, int* root,
                                                                       int* __restrict__ changed) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * DBSCAN_ROWS + (threadIdx.x >> 6);
    if (i >= N || !core[i]) return;
    int m = 0x7fffffff;
    for (int w = 0; w < W; ++w) {
        const unsigned long long word = adj[(size_t)i * W + w];
        if (!word) continue;
        const int j = w * 64 + lane;                                 // a set bit has j < N (the tail bits are clear); checked all the same
        if ((word >> lane & 1) && j < N && core[j]) m = min(m, dbscan_root(root, j));
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) m = min(m, __shfl_xor(m, o, 64));
    if (lane == 0) {
        const int r = dbscan_root(root, i);                          // a core row: 0 <= r <= i
        if (r >= 0 && r < N && m >= 0 && m < r) {
            atomicMin(&root[i], m);
            atomicMin(&root[r], m);
            *changed = 1;
        }
    }
}

// The pointer-jumping step, one thread per core row: root[i] <- the end of the chain root[root[...]].  A root points to a
// smaller or equal index, so the chase ends.
__global__ __launch_bounds__(256) void dbscan_jump_kernel(int N, const unsigned char* __restrict__ core, int* root) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N || !core[i]) return;
    const int r0 = dbscan_root(root, i);
    if (r0 < 0 || r0 >= N) return;                                   // not what vsom_dbscan_init and the hook step leave: nothing to chase
    int r = r0;
    for (int up = dbscan_root(root, r); up >= 0 && up < r; up = dbscan_root(root, r)) r = up;
    if (r < r0) atomicMin(&root[i], r);
}

// One workgroup: a cluster's number is the rank of its root (a core row with root[i] == i) among the roots, ascending --
// sklearn's numbering, which visits the rows in index order.  labels[root] = that rank, every other row -1 for now;
// record[0] = the clusters, record[1] = the core rows.  Thread t scans rows [t per, (t + 1) per).
__global__ __launch_bounds__(DBSCAN_SCAN) void dbscan_number_kernel(int N, const unsigned char* __restrict__ core,
                                                                    const int* __restrict__ root, int64_t* __restrict__ labels,
                                                                    int* __restrict__ record) {
    __shared__ int roots[DBSCAN_SCAN];
    __shared__ int cores[DBSCAN_SCAN];
    const int t = threadIdx.x;
    const int per = (N + DBSCAN_SCAN - 1) / DBSCAN_SCAN;
    const int i0 = min(t * per, N), i1 = min(i0 + per, N);
    int nr = 0, nc = 0;
    for (int i = i0; i < i1; ++i) {
        const bool c = core[i];
        nc += c;
        nr += c && root[i] == i;
    }
    roots[t] = nr;
    cores[t] = nc;
    __syncthreads();
    if (t == 0) {
        int sr = 0, sc = 0;
        for (int k = 0; k < DBSCAN_SCAN; ++k) {
            const int here = roots[k];
            roots[k] = sr;
            sr += here;
            sc += cores[k];
        }
        record[0] = sr;
        record[1] = sc;
    }
    __syncthreads();
    int next = roots[t];
    for (int i = i0; i < i1; ++i) labels[i] = core[i] && root[i] == i ? next++ : -1;
}

// A core row that is not a root takes its root's number (the roots' labels are not written here).
__global__ __launch_bounds__(256) void dbscan_core_label_kernel(int N, const unsigned char* __restrict__ core,
                                                                const int* __restrict__ root, int64_t* labels) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N || !core[i]) return;
    const int r = root[i];
    if (r != i && r >= 0 && r < N) labels[i] = labels[r];
}

// One wave per row that is not core, lane = column: the least number among its core neighbours -- sklearn expands the
// clusters one at a time in label order, so the first to reach a border point is the one with the smallest label -- or -1
// without a core neighbour.  Reads the labels of core rows only, writes those of the others.
__global__ __launch_bounds__(DBSCAN_ROWS * 64) void dbscan_border_kernel(const unsigned long long* __restrict__ adj, int N, int W,
                                                                         const unsigned char* __restrict__ core, int64_t* labels) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * DBSCAN_ROWS + (threadIdx.x >> 6);
    if (i >= N || core[i]) return;
    int m = 0x7fffffff;
    for (int w = 0; w < W; ++w) {
        const unsigned long long word = adj[(size_t)i * W + w];
        if (!word) continue;
        const int j = w * 64 + lane;
        if ((word >> lane & 1) && j < N && core[j]) m = min(m, (int)labels[j]);
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) m = min(m, __shfl_xor(m, o, 64));
    if (lane == 0) labels[i] = m == 0x7fffffff ? -1 : m;
}

// One workgroup: record[2] = the border rows (labelled, not core), record[3] = the noise rows.
__global__ __launch_bounds__(DBSCAN_SCAN) void dbscan_tally_kernel(int N, const unsigned char* __restrict__ core,
                                                                   const int64_t* __restrict__ labels, int* __restrict__ record) {
    __shared__ int border[DBSCAN_SCAN];
    __shared__ int noise[DBSCAN_SCAN];
    const int t = threadIdx.x;
    int nb = 0, nn = 0;
    for (int i = t; i < N; i += DBSCAN_SCAN) {
        const bool in = labels[i] >= 0;
        nb += in && !core[i];
        nn += !in;
    }
    border[t] = nb;
    noise[t] = nn;
    __syncthreads();
    if (t == 0) {
        int sb = 0, sn = 0;
        for (int k = 0; k < DBSCAN_SCAN; ++k) { sb += border[k]; sn += noise[k]; }
        record[2] = sb;
        record[3] = sn;
    }
}

// ---------------------------------------------------------------------------------------------- HDBSCAN
// The same contraction of a set with itself a fifth time, once per Boruvka round: the minimum spanning tree of the mutual
// reachability graph d_mr(i, j) = max(core_i, core_j, d(i, j)) of HDBSCAN (Campello, Moulavi, Sander 2013;
// sklearn.cluster.HDBSCAN; vit_som_amd/hdbscan.py; no counterpart in the reference) without ever holding that graph.
//
// The order.  Undirected edges are ordered by (w, lo, hi): w the fp32 value of d_mr, lo < hi the two rows.  The order is
// strict, so the tree is unique, a round -- every component takes its least outgoing edge -- can close no cycle but the
// mutual pair, and Kruskal under the same order rebuilds the tree edge for edge.  d is bit for bit the fp32 distance of
// vsom_umap_knn and the same bits seen from (i, j) and from (j, i) (the DBSCAN section's symmetry), fmaxf commutes.
//
// A round.  vsom_hdbscan_nearest leaves best[i] = the least (w, j) over the columns j with comp[j] != comp[i], packed
// as (fp32 bits of w) << 32 | j -- w >= 0, so its bits order as it does -- and all-ones for "none".  For a fixed row
// (w, j) orders the candidates exactly as (w, lo, hi) does.  vsom_hdbscan_merge takes per component the least of its
// rows' candidates under the full order in two integer atomicMin passes ((w, lo), then hi among the rows that attain it),
// hooks every component onto the one at the other end of its edge -- of a mutual pair only the larger label -- chases
// the hooks to their roots and relabels.  A label is a row of its component with comp[label] == label; a component that
// hooks emits its edge into edges[label], and that label is never a label again: the slots are disjoint, no counter is
// needed, and only the last root's slot stays empty.  The hooks are a forest (strict order, mutual pairs broken), so the
// chase from a label ends after fewer steps than there are components; its loop is bounded by N all the same.
// Integer atomics only; nothing waits on another workgroup; every value is a minimum under a strict order or a plain
// store of one: the edge list is bitwise reproducible whatever the chunking and the races.
constexpr unsigned long long HDB_NONE = ~0ull;
constexpr int HDB_COMPONENTS = 0, HDB_EDGES = 1, HDB_BAD = 2, HDB_ROUNDS = 3;       // the words of record

__device__ __forceinline__ unsigned long long hdb_key(float w, int j) {
    return (unsigned long long)(__float_as_uint(w) & 0x7fffffffu) << 32 | (unsigned)j;      // the mask: -0 orders as 0
}

struct HdbP : SelfP {
    const float* core;
    const int* comp;
    unsigned long long* best;   // [N], all-ones on entry
};

// One workgroup = 128 rows x one chunk of column tiles (KnnBlock).  The
// epilogue needs no LDS: a lane of the accumulators holds columns r and 32 + r of 16 rows (register v: KnnBlock::row(v)),
// so lane = column, and it keeps those 16 rows' squared norms, core distances, components and running
// best (w, j) in registers over the whole chunk.  A lane meets its columns in ascending order, so w < best keeps the
// lowest column among equals.  At the end of the chunk the 32 lanes of a half fold their keys with an integer minimum
// and one 64-bit atomicMin per (row, chunk) leaves the workgroup.  A row or column outside the set or without a distance
// to itself (dbscan_row_ok), a pair of one component -- the diagonal among them -- and a pair without a distance offer nothing.
template <bool FAST>
__global__ __launch_bounds__(KNN_THREADS, 2) void hdb_tile_kernel(const HdbP p) {
    constexpr int BM = KNN_BM, BN = KNN_BN;
    __shared__ __attribute__((aligned(16))) float lds[(BM + BN) * 36];

    const KnnBlock g(p.ct, p.chunks);
    const int r = g.r, bm0 = g.bm0;
    const int N = p.A.rows;

    float rsq[16], rcore[16], bw[16];
    int rcomp[16], bj[16];                                           // rcomp -1: a row that offers nothing
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int gi = bm0 + g.row(v);
        const bool in = gi < N;
        rsq[v] = in ? p.sq[gi] : 0.f;
        rcore[v] = in ? p.core[gi] : 0.f;
        rcomp[v] = in && dbscan_row_ok(rsq[v], p.metric) ? p.comp[gi] : -1;
        bw[v] = INFINITY;
        bj[v] = 0;
    }

    KnnStage<FAST> st;
    st.point(p.A, p.A);
    st.rows_a(p.A, bm0, g.t);

    for (int ctile = g.ct0; ctile < g.ct1; ++ctile) {
        const int bn0 = ctile * BN;
        f32x16 acc[2];
        knn_tile_dots<FAST>(st, g, p.A, p.A, bn0, p.D, lds, acc);
        // no LDS staging of the tile's comp / core values: one lane owns one column of the accumulator, so each of the 64
        // values is loaded by exactly the lane that uses it, once per tile, coalesced
        struct Column { float sq, core; int comp; };
        knn_tile_walk(
            g, bn0, acc,
            [&](int, int gj) {
                const bool in = gj < N;
                const float sj = in ? p.sq[gj] : 0.f;
                return Column{sj, in ? p.core[gj] : 0.f, in && dbscan_row_ok(sj, p.metric) ? p.comp[gj] : -1};
            },
            [&](float dot, const KnnPair& c, const Column& cj) {
                const int v = c.v;
                const float d = knn_distance(dot, rsq[v], cj.sq, p.metric);
                const float w = fmaxf(fmaxf(rcore[v], cj.core), d);
                if (rcomp[v] >= 0 && cj.comp >= 0 && cj.comp != rcomp[v] && d == d && w < bw[v]) { bw[v] = w; bj[v] = c.gj; }
            });
    }

    unsigned long long mine = HDB_NONE;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        unsigned long long key = bw[v] < INFINITY ? hdb_key(bw[v], bj[v]) : HDB_NONE;
#pragma unroll
        for (int o = 16; o; o >>= 1) {
            const unsigned long long other = __shfl_xor(key, o, 64);    // o < 32: within the half that shares these rows
            key = other < key ? other : key;
        }
        if (r == v) mine = key;
    }
    const int gi = bm0 + g.row(r);                                  // lane r < 16 of a half took register r's key
    if (r < 16 && gi < N && mine != HDB_NONE) atomicMin(&p.best[gi], mine);
}

__global__ __launch_bounds__(256) void hdb_clear_best_kernel(unsigned long long* __restrict__ best, int N) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < N) best[i] = HDB_NONE;
}

// One workgroup: record[HDB_BAD] = the rows without a distance to themselves or without a finite core distance.
__global__ __launch_bounds__(DBSCAN_SCAN) void hdb_bad_rows_kernel(const float* __restrict__ sq, const float* __restrict__ core, int N,
                                                                   int metric, int* __restrict__ record) {
    __shared__ int bad[DBSCAN_SCAN];
    const int t = threadIdx.x;
    int z = 0;
    for (int i = t; i < N; i += DBSCAN_SCAN) z += !(dbscan_row_ok(sq[i], metric) && fabsf(core[i]) < INFINITY);
    bad[t] = z;
    __syncthreads();
    if (t == 0) {
        int tz = 0;
        for (int k = 0; k < DBSCAN_SCAN; ++k) tz += bad[k];
        record[HDB_BAD] = tz;
    }
}

// The same round from a precomputed matrix M [N, N] (T float or double, row stride ldm).  One wave per row, lane = column
// modulo 64 in ascending order: w = max(core_i, core_j, (float)M[i][j]), which is the fp32 rounding of the maximum since
// rounding is monotone.  best[i] is a plain store: one wave owns the row.  An entry off the diagonal that is not finite as
// fp32 offers nothing and is counted in record[HDB_BAD] (cleared before the launch; an integer atomic, one per row that has any).
template <class T>
__global__ __launch_bounds__(DBSCAN_ROWS * 64) void hdb_matrix_kernel(const T* __restrict__ M, long ldm, int N,
                                                                      const float* __restrict__ core, const int* __restrict__ comp,
                                                                      unsigned long long* __restrict__ best, int* __restrict__ record) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * DBSCAN_ROWS + (threadIdx.x >> 6);
    if (i >= N) return;
    const T* row = M + (size_t)i * ldm;
    const float ci = core[i];
    const int mi = comp[i];
    float bw = INFINITY;
    int bj = 0, bad = 0;
    for (int j = lane; j < N; j += 64) {
        const float m = (float)row[j];
        const bool fin = fabsf(m) < INFINITY;
        bad += !fin && j != i;
        const float w = fmaxf(fmaxf(ci, core[j]), m);
        if (fin && comp[j] != mi && w < bw) { bw = w; bj = j; }
    }
    unsigned long long key = bw < INFINITY ? hdb_key(bw, bj) : HDB_NONE;
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const unsigned long long other = __shfl_xor(key, o, 64);
        key = other < key ? other : key;
        bad += __shfl_xor(bad, o, 64);
    }
    if (lane == 0) {
        best[i] = key;
        if (bad) atomicAdd(&record[HDB_BAD], bad);
    }
}
__global__ void hdb_clear_bad_kernel(int* __restrict__ record) { record[HDB_BAD] = 0; }

// comp[i] = i, edges[i] = (-1, -1, -1), record = (N components, no edge, no bad row, no round).
__global__ __launch_bounds__(256) void hdb_init_kernel(int N, int* __restrict__ comp, int* __restrict__ edges, int* __restrict__ record) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < N) {
        comp[i] = i;
        edges[3 * i] = edges[3 * i + 1] = edges[3 * i + 2] = -1;
    }
    if (i < 4) record[i] = i == HDB_COMPONENTS ? N : 0;
}

// The merge step's arrays, in the caller's work (int64 [2 N]): cbest u64 [N], then (hi, parent) int32 [N] each.
struct HdbWork {
    unsigned long long* cbest;
    int* chi;
    int* parent;
};
inline HdbWork hdb_work(int64_t* work, long N) {
    HdbWork w;
    w.cbest = reinterpret_cast<unsigned long long*>(work);
    w.chi = reinterpret_cast<int*>(work + N);
    w.parent = w.chi + N;
    return w;
}

__global__ __launch_bounds__(256) void hdb_merge_clear_kernel(int N, HdbWork w) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    w.cbest[i] = HDB_NONE;
    w.chi[i] = 0x7fffffff;
    w.parent[i] = i;
}

// Row i's candidate as an undirected edge: false without one (or with a component or a column that is no row index --
// not what vsom_hdbscan_init and _nearest leave; nothing is then read or written through it).
__device__ __forceinline__ bool hdb_candidate(const unsigned long long* best, const int* comp, int N, int i, int& c,
                                              unsigned long long& wlo, int& hi) {
    const unsigned long long k = best[i];
    const unsigned j = (unsigned)k;
    c = comp[i];
    if (k == HDB_NONE || j >= (unsigned)N || (unsigned)c >= (unsigned)N) return false;
    const unsigned lo = j < (unsigned)i ? j : (unsigned)i;
    hi = (int)(j < (unsigned)i ? (unsigned)i : j);
    wlo = (k & 0xffffffff00000000ull) | lo;
    return true;
}
// cbest[c] = the least (w, lo) over the rows of component c; then chi[c] = the least hi among the rows that attain it.
__global__ __launch_bounds__(256) void hdb_merge_low_kernel(const unsigned long long* __restrict__ best, const int* __restrict__ comp,
                                                            int N, HdbWork w) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    int c, hi;
    unsigned long long wlo;
    if (i < N && hdb_candidate(best, comp, N, i, c, wlo, hi)) atomicMin(&w.cbest[c], wlo);
}
__global__ __launch_bounds__(256) void hdb_merge_high_kernel(const unsigned long long* __restrict__ best, const int* __restrict__ comp,
                                                             int N, HdbWork w) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    int c, hi;
    unsigned long long wlo;
    if (i < N && hdb_candidate(best, comp, N, i, c, wlo, hi) && wlo == w.cbest[c]) atomicMin(&w.chi[c], hi);
}

// Label c (comp[c] == c) with an edge hooks onto the component at its other end and emits the edge into edges[c]; of a
// mutual pair -- both took the same (w, lo, hi) -- only the larger label does.
__global__ __launch_bounds__(256) void hdb_merge_hook_kernel(const int* __restrict__ comp, int N, HdbWork w, int* __restrict__ edges) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= N || comp[c] != c || w.cbest[c] == HDB_NONE) return;
    const int lo = (int)(unsigned)w.cbest[c], hi = w.chi[c];
    if (lo >= N || (unsigned)hi >= (unsigned)N) return;
    const int o = comp[lo] == c ? comp[hi] : comp[lo];
    if ((unsigned)o >= (unsigned)N || o == c) return;
    const bool mutual = w.cbest[o] == w.cbest[c] && w.chi[o] == hi;
    if (mutual && c < o) return;
    w.parent[c] = o;
    edges[3 * c] = lo;
    edges[3 * c + 1] = hi;
    edges[3 * c + 2] = (int)(unsigned)(w.cbest[c] >> 32);
}

// parent[c] <- the root of label c's tree of hooks.  Every value a racing read of parent can return is an ancestor (the
// hook or the root a finished thread stored), so the chase only ever moves up; the forest is shallower than N.
__global__ __launch_bounds__(256) void hdb_merge_jump_kernel(const int* __restrict__ comp, int N, int* parent) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= N || comp[c] != c) return;
    int r = dbscan_root(parent, c);
    for (int steps = 0; steps < N; ++steps) {
        const int up = dbscan_root(parent, r);
        if (up == r) break;
        r = up;
    }
    __atomic_store_n(parent + c, r, __ATOMIC_RELAXED);
}
__global__ __launch_bounds__(256) void hdb_merge_relabel_kernel(int N, const int* __restrict__ parent, int* __restrict__ comp) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int c = comp[i];
    if ((unsigned)c < (unsigned)N) comp[i] = parent[c];
}

// One workgroup: record = (the labels left, N less that: the edges so far, ., one round more).
__global__ __launch_bounds__(DBSCAN_SCAN) void hdb_merge_record_kernel(const int* __restrict__ comp, int N, int* __restrict__ record) {
    __shared__ int left[DBSCAN_SCAN];
    const int t = threadIdx.x;
    int n = 0;
    for (int i = t; i < N; i += DBSCAN_SCAN) n += comp[i] == i;
    left[t] = n;
    __syncthreads();
    if (t == 0) {
        int tn = 0;
        for (int k = 0; k < DBSCAN_SCAN; ++k) tn += left[k];
        record[HDB_COMPONENTS] = tn;
        record[HDB_EDGES] = N - tn;
        record[HDB_ROUNDS] += 1;
    }
}

}  // namespace
}  // namespace vsom

extern "C" {

size_t vsom_knn_query_workspace_bytes(long Nq, long Nb, int k) {
    if (Nq < 1 || Nb < 1 || k < 1) return 0;
    return vsom::query_layout(nullptr, Nq, Nb, k, false).bytes;
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
    return knn_search("knn_query", false, Q, ldq, Nq, X, ldx, Nb, D, k, metric, index_base, accumulate, exclude, idx, dist, ws,
                      stream);
}

size_t vsom_umap_knn_workspace_bytes(long N, int k) {
    if (N < 1 || k < 1) return 0;
    return vsom::query_layout(nullptr, N, N, k, true).bytes;
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
    return knn_search("umap_knn", true, X, ldx, N, X, ldx, N, D, k, metric, 0, 0, nullptr, knn_idx, knn_dist, ws, stream);
}

size_t vsom_knn_ranks_workspace_bytes(long N, int k) {
    if (N < 1 || k < 1) return 0;
    return vsom::rank_layout(nullptr, N, k).bytes;
}

int vsom_knn_ranks(const float* A, long lda, long N, int D, int metric, const int64_t* nbr, int k, int32_t* less, int32_t* tied,
                   void* ws, size_t ws_bytes, vsom_stream_t stream) {
    using namespace vsom;
    VSOM_REQUIRE(A && nbr && less && tied, VSOM_EINVAL, "knn_ranks: null pointer");
    VSOM_REQUIRE(N >= 2 && D >= 1 && k >= 1 && lda >= D && N <= 0x7fffffffL - KNN_BM, VSOM_EINVAL,
                 "knn_ranks: bad sizes N=%ld D=%d k=%d lda=%ld", N, D, k, lda);
    VSOM_REQUIRE(k <= KNN_MAX_K, VSOM_EUNSUPPORTED, "knn_ranks: k=%d > %d", k, KNN_MAX_K);
    VSOM_REQUIRE(metric == VSOM_DIST_EUCLIDEAN || metric == VSOM_DIST_COSINE, VSOM_EUNSUPPORTED,
                 "knn_ranks: metric %d (euclidean or cosine only)", metric);
    VSOM_REQUIRE(ws && aligned16(ws) && ws_bytes >= vsom_knn_ranks_workspace_bytes(N, k), VSOM_EWORKSPACE,
                 "knn_ranks: workspace too small or misaligned");
    const RankWs w = rank_layout(ws, N, k);
    const bool vec = knn_self_vec(A, lda, D);
    VSOM_LAUNCH(knn_sqnorm_kernel, dim3(cdiv(N, 256)), dim3(256), 0, stream, A, lda, N, D, w.sq);
    const dim3 slots((unsigned)(((size_t)N * k + 255) / 256));
    if (vec)
        VSOM_LAUNCH(knn_rank_threshold_kernel<true>, slots, dim3(256), 0, stream, A, lda, N, D, k, metric, nbr,
                    (const float*)w.sq, w.slot, less, tied);
    else
        VSOM_LAUNCH(knn_rank_threshold_kernel<false>, slots, dim3(256), 0, stream, A, lda, N, D, k, metric, nbr,
                    (const float*)w.sq, w.slot, less, tied);
    RankP p = {};
    p.k = k; p.slot = w.slot; p.less = less; p.tied = tied;
    knn_self_launch<RankP, knn_rank_tile_kernel<true>, knn_rank_tile_kernel<false>>(p, A, lda, N, D, metric, w.sq, vec, stream);
    return launch_status("knn_ranks");
}

size_t vsom_silhouette_workspace_bytes(long N, int n_clusters) {
    if (N < 1 || n_clusters < 1) return 0;
    return vsom::sil_layout(nullptr, N, n_clusters).bytes;
}

int vsom_silhouette(const float* X, long ldx, long N, int D, int metric, const int64_t* labels, int n_clusters, double* sil,
                    double* a, double* b, int64_t* nearest, int64_t* counts, double* cluster_mean, double* score,
                    int64_t* status, void* ws, size_t ws_bytes, vsom_stream_t stream) {
    using namespace vsom;
    VSOM_REQUIRE(X && labels && sil && counts && score && status, VSOM_EINVAL, "silhouette: null pointer");
    VSOM_REQUIRE(N >= 2 && D >= 1 && ldx >= D && n_clusters >= 1, VSOM_EINVAL, "silhouette: bad sizes N=%ld D=%d ldx=%ld n_clusters=%d",
                 N, D, ldx, n_clusters);
    VSOM_REQUIRE(N <= SIL_MAX_N, VSOM_EUNSUPPORTED, "silhouette: N=%ld > %ld (a row's fixed-point sum must stay below 2^63)", N,
                 SIL_MAX_N);
    VSOM_REQUIRE(metric == VSOM_DIST_EUCLIDEAN || metric == VSOM_DIST_COSINE, VSOM_EUNSUPPORTED,
                 "silhouette: metric %d (euclidean or cosine only)", metric);
    VSOM_REQUIRE(ws && aligned16(ws) && ws_bytes >= vsom_silhouette_workspace_bytes(N, n_clusters), VSOM_EWORKSPACE,
                 "silhouette: workspace too small or misaligned");
    const SilWs w = sil_layout(ws, N, n_clusters);
    const bool vec = D % 4 == 0 && ldx % 4 == 0 && aligned16(X);
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
    unsigned long long* stat = reinterpret_cast<unsigned long long*>(status);
    const size_t clear_blocks = (w.clear_words + 255) / 256;
    VSOM_LAUNCH(sil_clear_kernel, dim3((unsigned)(clear_blocks < 4096 ? clear_blocks : 4096)), dim3(256), 0, stream, w.S,
                w.clear_words, cnt, n_clusters, stat);
    VSOM_LAUNCH(sil_sqnorm_kernel, dim3(cdiv(N, 256)), dim3(256), 0, stream, X, ldx, N, D, w.sq);
    VSOM_LAUNCH(sil_prepare_kernel, dim3(cdiv(N, 256)), dim3(256), 0, stream, labels, (const float*)w.sq, N, n_clusters, cnt, w.ctrl,
                stat);
    SilP p = {};
    p.C = n_clusters; p.labels = labels; p.ctrl = w.ctrl; p.S = w.S; p.status = stat;
    knn_self_launch<SilP, sil_tile_kernel<true>, sil_tile_kernel<false>>(p, X, ldx, N, D, metric, w.sq, vec, stream);
    const SilOut out = {sil, a, b, nearest};
    VSOM_LAUNCH(sil_finish_kernel, dim3(cdiv(N, SIL_ROWS)), dim3(SIL_ROWS * 64), 0, stream, (const unsigned long long*)w.S,
                (const unsigned long long*)cnt, labels, N, n_clusters, (const unsigned*)w.ctrl, metric, out, w.acc);
    VSOM_LAUNCH(sil_means_kernel, dim3(1), dim3(256), 0, stream, (const unsigned long long*)w.acc, (const unsigned long long*)cnt, N,
                n_clusters, cluster_mean, score, stat);
    return launch_status("silhouette");
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

int vsom_dbscan_neighbours(const float* X, long ldx, long N, int D, int metric, double eps, float* sq, uint64_t* adj,
                           int32_t* count, int64_t* status, vsom_stream_t stream) {
    using namespace vsom;
    VSOM_REQUIRE(X && sq && adj && count && status, VSOM_EINVAL, "dbscan_neighbours: null pointer");
    VSOM_REQUIRE(N >= 2 && D >= 1 && ldx >= D && N <= 0x7fffffffL - KNN_BM, VSOM_EINVAL,
                 "dbscan_neighbours: bad sizes N=%ld D=%d ldx=%ld", N, D, ldx);
    VSOM_REQUIRE(eps >= 0.0, VSOM_EINVAL, "dbscan_neighbours: eps=%g must be >= 0", eps);
    VSOM_REQUIRE(N <= DBSCAN_MAX_N, VSOM_EUNSUPPORTED, "dbscan_neighbours: N=%ld > %ld (the bit matrix would pass 2 GiB)", N,
                 DBSCAN_MAX_N);
    VSOM_REQUIRE(metric == VSOM_DIST_EUCLIDEAN || metric == VSOM_DIST_COSINE, VSOM_EUNSUPPORTED,
                 "dbscan_neighbours: metric %d (euclidean or cosine only)", metric);
    const bool vec = knn_self_vec(X, ldx, D);
    VSOM_LAUNCH(knn_sqnorm_kernel, dim3(cdiv(N, 256)), dim3(256), 0, stream, X, ldx, N, D, sq);
    NeighP p = {};
    p.eps = eps; p.adj = reinterpret_cast<unsigned long long*>(adj);
    const QueryPlan pl =
        knn_self_launch<NeighP, dbscan_tile_kernel<true>, dbscan_tile_kernel<false>>(p, X, ldx, N, D, metric, sq, vec, stream);
    VSOM_LAUNCH(dbscan_count_kernel, dim3(cdiv(N, DBSCAN_ROWS)), dim3(DBSCAN_ROWS * 64), 0, stream,
                (const unsigned long long*)p.adj, (int)N, pl.ct, count);
    VSOM_LAUNCH(dbscan_status_kernel, dim3(1), dim3(DBSCAN_SCAN), 0, stream, (const int*)count, (int)N, 1, status);
    return launch_status("dbscan_neighbours");
}

int vsom_dbscan_threshold(const void* M, long ldm, long N, int is_f64, double eps, uint64_t* adj, int32_t* count, int64_t* status,
                          vsom_stream_t stream) {
    using namespace vsom;
    VSOM_REQUIRE(M && adj && count && status, VSOM_EINVAL, "dbscan_threshold: null pointer");
    VSOM_REQUIRE(N >= 2 && ldm >= N, VSOM_EINVAL, "dbscan_threshold: bad sizes N=%ld ldm=%ld", N, ldm);
    VSOM_REQUIRE(eps >= 0.0, VSOM_EINVAL, "dbscan_threshold: eps=%g must be >= 0", eps);
    VSOM_REQUIRE(N <= DBSCAN_MAX_N, VSOM_EUNSUPPORTED, "dbscan_threshold: N=%ld > %ld (the bit matrix would pass 2 GiB)", N,
                 DBSCAN_MAX_N);
    const int W = cdiv(N, 64);
    unsigned long long* words = reinterpret_cast<unsigned long long*>(adj);
    unsigned long long* stat = reinterpret_cast<unsigned long long*>(status);
    const dim3 grid(cdiv(N, DBSCAN_ROWS)), block(DBSCAN_ROWS * 64);
    VSOM_LAUNCH(dbscan_clear_status_kernel, dim3(1), dim3(2), 0, stream, status);
    if (is_f64)
        VSOM_LAUNCH(dbscan_threshold_kernel<double>, grid, block, 0, stream, static_cast<const double*>(M), ldm, (int)N, W, eps, words,
                    count, stat);
    else
        VSOM_LAUNCH(dbscan_threshold_kernel<float>, grid, block, 0, stream, static_cast<const float*>(M), ldm, (int)N, W, eps, words,
                    count, stat);
    VSOM_LAUNCH(dbscan_status_kernel, dim3(1), dim3(DBSCAN_SCAN), 0, stream, (const int*)count, (int)N, 0, status);
    return launch_status("dbscan_threshold");
}

int vsom_dbscan_init(const int32_t* count, long N, int min_samples, uint8_t* core, int32_t* root, vsom_stream_t stream) {
    using namespace vsom;
    VSOM_REQUIRE(count && core && root, VSOM_EINVAL, "dbscan_init: null pointer");
    VSOM_REQUIRE(N >= 1 && N <= DBSCAN_MAX_N && min_samples >= 1, VSOM_EINVAL, "dbscan_init: bad sizes N=%ld min_samples=%d", N,
                 min_samples);
    VSOM_LAUNCH(dbscan_init_kernel, dim3(cdiv(N, 256)), dim3(256), 0, stream, count, (int)N, min_samples, core, root);
    return launch_status("dbscan_init");
}

int vsom_dbscan_round(const uint64_t* adj, long N, const uint8_t* core, int32_t* root, int rounds, int32_t* changed,
                      vsom_stream_t stream) {
    using namespace vsom;
    VSOM_REQUIRE(adj && core && root && changed, VSOM_EINVAL, "dbscan_round: null pointer");
    VSOM_REQUIRE(N >= 1 && N <= DBSCAN_MAX_N && rounds >= 1 && rounds <= 1024, VSOM_EINVAL, "dbscan_round: bad sizes N=%ld rounds=%d",
                 N, rounds);
    const int W = cdiv(N, 64);
    const unsigned long long* words = reinterpret_cast<const unsigned long long*>(adj);
    VSOM_LAUNCH(dbscan_clear_changed_kernel, dim3(1), dim3(1), 0, stream, changed);
    for (int s = 0; s < rounds; ++s) {
        VSOM_LAUNCH(dbscan_hook_kernel, dim3(cdiv(N, DBSCAN_ROWS)), dim3(DBSCAN_ROWS * 64), 0, stream, words, (int)N, W, core, root,
                    changed);
        VSOM_LAUNCH(dbscan_jump_kernel, dim3(cdiv(N, 256)), dim3(256), 0, stream, (int)N, core, root);
    }
    return launch_status("dbscan_round");
}

int vsom_dbscan_finish(const uint64_t* adj, long N, const uint8_t* core, const int32_t* root, int64_t* labels, int32_t* record,
                       vsom_stream_t stream) {
    using namespace vsom;
    VSOM_REQUIRE(adj && core && root && labels && record, VSOM_EINVAL, "dbscan_finish: null pointer");
    VSOM_REQUIRE(N >= 1 && N <= DBSCAN_MAX_N, VSOM_EINVAL, "dbscan_finish: bad sizes N=%ld", N);
    const int W = cdiv(N, 64);
    const unsigned long long* words = reinterpret_cast<const unsigned long long*>(adj);
    VSOM_LAUNCH(dbscan_number_kernel, dim3(1), dim3(DBSCAN_SCAN), 0, stream, (int)N, core, root, labels, record);
    VSOM_LAUNCH(dbscan_core_label_kernel, dim3(cdiv(N, 256)), dim3(256), 0, stream, (int)N, core, root, labels);
    VSOM_LAUNCH(dbscan_border_kernel, dim3(cdiv(N, DBSCAN_ROWS)), dim3(DBSCAN_ROWS * 64), 0, stream, words, (int)N, W, core, labels);
    VSOM_LAUNCH(dbscan_tally_kernel, dim3(1), dim3(DBSCAN_SCAN), 0, stream, (int)N, core, (const int64_t*)labels, record);
    return launch_status("dbscan_finish");
}

int vsom_hdbscan_init(long N, int32_t* comp, int32_t* edges, int32_t* record, vsom_stream_t stream) {
    using namespace vsom;
    VSOM_REQUIRE(comp && edges && record, VSOM_EINVAL, "hdbscan_init: null pointer");
    VSOM_REQUIRE(N >= 2, VSOM_EINVAL, "hdbscan_init: bad sizes N=%ld", N);
    VSOM_REQUIRE(N <= DBSCAN_MAX_N, VSOM_EUNSUPPORTED, "hdbscan_init: N=%ld > %ld", N, DBSCAN_MAX_N);
    VSOM_LAUNCH(hdb_init_kernel, dim3(cdiv(N, 256)), dim3(256), 0, stream, (int)N, comp, edges, record);
    return launch_status("hdbscan_init");
}

int vsom_hdbscan_nearest(const float* X, long ldx, long N, int D, int metric, const float* core, const int32_t* comp, float* sq,
                         uint64_t* best, int32_t* record, vsom_stream_t stream) {
    using namespace vsom;
    VSOM_REQUIRE(X && core && comp && sq && best && record, VSOM_EINVAL, "hdbscan_nearest: null pointer");
    VSOM_REQUIRE(N >= 2 && D >= 1 && ldx >= D, VSOM_EINVAL, "hdbscan_nearest: bad sizes N=%ld D=%d ldx=%ld", N, D, ldx);
    VSOM_REQUIRE(N <= DBSCAN_MAX_N, VSOM_EUNSUPPORTED, "hdbscan_nearest: N=%ld > %ld", N, DBSCAN_MAX_N);
    VSOM_REQUIRE(metric == VSOM_DIST_EUCLIDEAN || metric == VSOM_DIST_COSINE, VSOM_EUNSUPPORTED,
                 "hdbscan_nearest: metric %d (euclidean or cosine only)", metric);
    const bool vec = knn_self_vec(X, ldx, D);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(best);
    VSOM_LAUNCH(knn_sqnorm_kernel, dim3(cdiv(N, 256)), dim3(256), 0, stream, X, ldx, N, D, sq);
    VSOM_LAUNCH(hdb_clear_best_kernel, dim3(cdiv(N, 256)), dim3(256), 0, stream, keys, (int)N);
    VSOM_LAUNCH(hdb_bad_rows_kernel, dim3(1), dim3(DBSCAN_SCAN), 0, stream, (const float*)sq, core, (int)N, metric, record);
    HdbP p = {};
    p.core = core; p.comp = comp; p.best = keys;
    knn_self_launch<HdbP, hdb_tile_kernel<true>, hdb_tile_kernel<false>>(p, X, ldx, N, D, metric, sq, vec, stream);
    return launch_status("hdbscan_nearest");
}

int vsom_hdbscan_nearest_matrix(const void* M, long ldm, long N, int is_f64, const float* core, const int32_t* comp, uint64_t* best,
                                int32_t* record, vsom_stream_t stream) {
    using namespace vsom;
    VSOM_REQUIRE(M && core && comp && best && record, VSOM_EINVAL, "hdbscan_nearest_matrix: null pointer");
    VSOM_REQUIRE(N >= 2 && ldm >= N, VSOM_EINVAL, "hdbscan_nearest_matrix: bad sizes N=%ld ldm=%ld", N, ldm);
    VSOM_REQUIRE(N <= DBSCAN_MAX_N, VSOM_EUNSUPPORTED, "hdbscan_nearest_matrix: N=%ld > %ld", N, DBSCAN_MAX_N);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(best);
    const dim3 grid(cdiv(N, DBSCAN_ROWS)), block(DBSCAN_ROWS * 64);
    VSOM_LAUNCH(hdb_clear_bad_kernel, dim3(1), dim3(1), 0, stream, record);
    if (is_f64)
        VSOM_LAUNCH(hdb_matrix_kernel<double>, grid, block, 0, stream, static_cast<const double*>(M), ldm, (int)N, core, comp, keys,
                    record);
    else
        VSOM_LAUNCH(hdb_matrix_kernel<float>, grid, block, 0, stream, static_cast<const float*>(M), ldm, (int)N, core, comp, keys,
                    record);
    return launch_status("hdbscan_nearest_matrix");
}

int vsom_hdbscan_merge(const uint64_t* best, long N, int32_t* comp, int32_t* edges, int64_t* work, int32_t* record,
                       vsom_stream_t stream) {
    using namespace vsom;
    VSOM_REQUIRE(best && comp && edges && work && record, VSOM_EINVAL, "hdbscan_merge: null pointer");
    VSOM_REQUIRE(N >= 2, VSOM_EINVAL, "hdbscan_merge: bad sizes N=%ld", N);
    VSOM_REQUIRE(N <= DBSCAN_MAX_N, VSOM_EUNSUPPORTED, "hdbscan_merge: N=%ld > %ld", N, DBSCAN_MAX_N);
    const unsigned long long* keys = reinterpret_cast<const unsigned long long*>(best);
    const HdbWork w = hdb_work(work, N);
    const dim3 grid(cdiv(N, 256)), block(256);
    const int n = (int)N;
    VSOM_LAUNCH(hdb_merge_clear_kernel, grid, block, 0, stream, n, w);
    VSOM_LAUNCH(hdb_merge_low_kernel, grid, block, 0, stream, keys, (const int*)comp, n, w);
    VSOM_LAUNCH(hdb_merge_high_kernel, grid, block, 0, stream, keys, (const int*)comp, n, w);
    VSOM_LAUNCH(hdb_merge_hook_kernel, grid, block, 0, stream, (const int*)comp, n, w, edges);
    VSOM_LAUNCH(hdb_merge_jump_kernel, grid, block, 0, stream, (const int*)comp, n, w.parent);
    VSOM_LAUNCH(hdb_merge_relabel_kernel, grid, block, 0, stream, n, (const int*)w.parent, comp);
    VSOM_LAUNCH(hdb_merge_record_kernel, dim3(1), dim3(DBSCAN_SCAN), 0, stream, (const int*)comp, n, record);
    return launch_status("hdbscan_merge");
}

}  // extern "C"
