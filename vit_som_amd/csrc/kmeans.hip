// k-means (Lloyd) for evaluate_kmeans (tools/evaluation.py:54-91): the steps of sklearn.cluster.KMeans
// (_kmeans.py, algorithm="lloyd", dense fp32 input, unit sample weights) that touch the data.
//
//   vsom_kmeans_assign     E-step + the partial M-step in one launch (lloyd_iter_chunked_dense).
//   vsom_kmeans_update     fixed-order reduction of the per-workgroup slabs, new centres, status (changed labels,
//                          center_shift_tot, empty clusters, inertia).
//   vsom_kmeans_relocate   _relocate_empty_clusters_dense for the moves the host chose, then the centres again.
//   vsom_kmeanspp_dist     the distance / potential step of _kmeans_plusplus.
//   vsom_kmeans_colvar     mean(var(X, axis=0)) of _tolerance.
//
// No floating-point atomics anywhere: every sum has one fixed order, so a fit is bitwise reproducible.
#include "row_tile.h"

namespace vsom {
namespace {

constexpr int KM_THREADS = 512;              // 8 waves
constexpr int KM_WAVES = KM_THREADS / 64;
constexpr int KM_RB = 4;                     // rows per wave, register-blocked: one LDS centre read serves 4 rows
constexpr int KM_GROUP = KM_WAVES * KM_RB;   // 32 rows per workgroup step
constexpr int KM_LDS = 144 * 1024;           // centre tile [KC][DT]; gfx950 has 160 KiB per CU
constexpr int KM_MAX_GROUPS = 256;           // one workgroup per CU
constexpr int KM_MAX_K = 1024;               // per-cluster counts and flags share the LDS allocation
constexpr size_t KM_SLAB_BUDGET = size_t(128) << 20;
constexpr int KM_COLVAR_CHUNKS = 64;
constexpr int KM_RED_THREADS = 256;

// Workgroups of the assign pass: one per CU, fewer when the [G, k, D] slabs would pass 128 MiB (large k * D).
inline int km_groups(long N, int D, int k) {
    const size_t per = (size_t)k * (size_t)D * 4 + (size_t)k * 4;
    long g = (long)(KM_SLAB_BUDGET / per);
    if (g < 1) g = 1;
    if (g > KM_MAX_GROUPS) g = KM_MAX_GROUPS;
    const long need = (N + KM_GROUP - 1) / KM_GROUP;
    return (int)(g < need ? g : need);
}

// Workspace layout (each piece 256-byte aligned):
//   slabs  f32 [G][k][D]   per-workgroup cluster sums        (also the colvar partials, f64 [64][2][D])
//   cnt    i32 [G][k]      per-workgroup cluster counts
//   chg    i32 [G]         per-workgroup changed labels
//   sums   f32 [k][D]      reduced cluster sums (what the relocation edits)
//   part   f64 [P]         per-block partials of the centre shift
//   amax   i32 [1]         first argmax of the counts (where _average_centers puts an empty cluster)
struct KmWs {
    float* slabs;
    int* cnt;
    int* chg;
    float* sums;
    double* part;
    int* amax;
    long rows_per_group;    // rows of a workgroup of the assign pass (not rounded to 32)
    int G;                  // workgroups the assign pass runs: every one of them gets rows
    size_t bytes;
};

// blocks of the centre pass: one element per thread (each thread sums G slab values), at most 4096 blocks
inline int km_shift_blocks(int D, int k) { const int b = cdiv((long)k * D, KM_RED_THREADS); return b < 4096 ? b : 4096; }

inline KmWs km_layout(void* ws, long N, int D, int k) {
    KmWs w = {};
    const int G0 = km_groups(N, D, k);          // sizes the sections; the canonical split runs G <= G0 workgroups
    const Split rows = even_split(N, G0);
    w.rows_per_group = rows.per;
    w.G = rows.count;
    size_t slab = align256((size_t)G0 * k * D * 4);
    const size_t colvar = align256((size_t)KM_COLVAR_CHUNKS * 2 * D * 8);
    if (colvar > slab) slab = colvar;
    const size_t cnt = align256((size_t)G0 * k * 4), chg = align256((size_t)G0 * 4);
    const size_t sums = align256((size_t)k * D * 4), part = align256((size_t)km_shift_blocks(D, k) * 8);
    char* p = static_cast<char*>(ws);
    w.slabs = reinterpret_cast<float*>(p);
    w.cnt = reinterpret_cast<int*>(p + slab);
    w.chg = reinterpret_cast<int*>(p + slab + cnt);
    w.sums = reinterpret_cast<float*>(p + slab + cnt + chg);
    w.part = reinterpret_cast<double*>(p + slab + cnt + chg + sums);
    w.amax = reinterpret_cast<int*>(p + slab + cnt + chg + sums + part);
    w.bytes = slab + cnt + chg + sums + part + 256;
    return w;
}

struct AssignP {
    const float* X;
    long ldx;
    long N;
    int D, k;
    const float* C;
    int64_t* labels;
    const int64_t* prev;
    float* mind;
    float* slabs;   // [G][k][D]
    int* cnt;       // [G][k]
    int* chg;       // [G]
    long rows_per_group;
    int dt;         // centre D-tile (multiple of 4 * 64 in the vector path, of 64 in the scalar path)
};

// a piece's squared distance to a centre: f32, one fma chain over the piece's columns
struct SqDist {
    static constexpr int PLANES = 1;
    typedef float Acc;
    static __device__ __forceinline__ float term(f32x4 x, const f32x4 (&c)[1]) {
        const f32x4 e = x - c[0];
        float s = e.x * e.x;
        s = fmaf(e.y, e.y, s);
        s = fmaf(e.z, e.z, s);
        return fmaf(e.w, e.w, s);
    }
    static __device__ __forceinline__ float term(float x, const float (&c)[1]) { const float e = x - c[0]; return e * e; }
};

// sklearn lloyd_iter_chunked_dense (_k_means_lloyd.pyx) for one workgroup's contiguous row range, 32 rows at a time:
//  (1) distances: row_tile_pass (row_tile.h) with SqDist, wave w on rows 4w..4w+3 of the step.  Per (row, centre) the lane
//      sums its pieces in column order, then a butterfly sums the 64 lanes (same value on every lane); labels = first argmin.
//  (2) partial M-step: the 32 rows are read again (non-temporally: their last use) and added into
//      this workgroup's slab, thread t owning the pieces t*VEC + 512*VEC*m, rows in (label, row) order, one
//      read-modify-write of the slab per label present in the step.  Slab rows never touched are zeroed at the end.
template <int KC, int VEC>
__global__ __launch_bounds__(KM_THREADS) void kmeans_assign_kernel(AssignP p) {
    typedef Vec<VEC> V;
    typedef typename V::T vT;
    extern __shared__ __attribute__((aligned(16))) float lds_c[];     // [KC][dt]
    __shared__ int s_lab[KM_GROUP], s_ord[KM_GROUP];
    __shared__ int s_nrows, s_changed;
    int* s_cnt = reinterpret_cast<int*>(lds_c + (size_t)KC * p.dt);   // [k] counts, then [k] seen flags
    int* s_seen = s_cnt + p.k;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int D = p.D, k = p.k;
    const long r0 = (long)blockIdx.x * p.rows_per_group;
    const long r1 = min(p.N, r0 + p.rows_per_group);
    float* slab = p.slabs + (size_t)blockIdx.x * k * D;
    for (int j = tid; j < k; j += KM_THREADS) { s_cnt[j] = 0; s_seen[j] = 0; }
    if (tid == 0) s_changed = 0;
    const float* const centres[1] = {p.C};
    const int nchunks = (k + KC - 1) / KC;
    const bool resident = nchunks == 1 && D <= p.dt;                // centres staged once for the whole range
    __syncthreads();

    for (long base = r0; base < r1; base += KM_GROUP) {
        float best[KM_RB];
        int bidx[KM_RB];
#pragma unroll
        for (int r = 0; r < KM_RB; ++r) { best[r] = INFINITY; bidx[r] = 0; }
        const long rw = base + wave * KM_RB;
        for (int ch = 0; ch < nchunks; ++ch) {
            const int j0 = ch * KC, kc = min(KC, k - j0);
            float acc[KM_RB][KC];
#pragma unroll
            for (int r = 0; r < KM_RB; ++r)
#pragma unroll
                for (int j = 0; j < KC; ++j) acc[r][j] = 0.f;
            row_tile_pass<KM_THREADS, KM_RB, KC, VEC, SqDist>(p.X, p.ldx, rw, r1, D, centres, j0, kc, lds_c, p.dt,
                                                              !resident || base == r0, acc);
#pragma unroll
            for (int r = 0; r < KM_RB; ++r)
#pragma unroll
                for (int j = 0; j < KC; ++j) {
                    const float s = wave_sum(acc[r][j]);
                    if (j < kc && s < best[r]) { best[r] = s; bidx[r] = j0 + j; }
                }
        }
        // labels, mind, changed; the step's labels into LDS for the M-step
#pragma unroll
        for (int r = 0; r < KM_RB; ++r) {
            const long row = rw + r;
            if (lane == 0) {
                if (row < r1) {
                    const int64_t before = p.prev[row];     // read before the store: prev may alias labels
                    p.labels[row] = bidx[r];
                    p.mind[row] = best[r];
                    if (before != bidx[r]) atomicAdd(&s_changed, 1);
                }
                s_lab[wave * KM_RB + r] = row < r1 ? bidx[r] : -1;
            }
        }
        __syncthreads();
        if (tid == 0) {                          // stable order by label (32 entries, insertion sort)
            int n = 0;
            for (int r = 0; r < KM_GROUP; ++r) {
                const int L = s_lab[r];
                if (L < 0) continue;
                s_cnt[L] += 1;
                int q = n++;
                while (q > 0 && s_lab[s_ord[q - 1]] > L) { s_ord[q] = s_ord[q - 1]; --q; }
                s_ord[q] = r;
            }
            s_nrows = n;
        }
        __syncthreads();
        const int n = s_nrows;
        for (int d = tid * VEC; d < D; d += KM_THREADS * VEC) {
            vT run = V::zero();
            for (int s0 = 0; s0 < n; s0 += 8) {
                vT xs[8];                        // eight independent loads in flight, then the ordered adds
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    xs[u] = s0 + u < n ? V::load_nt(p.X + (base + s_ord[s0 + u]) * p.ldx + d) : V::zero();
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int s = s0 + u;
                    if (s >= n) break;
                    const int L = s_lab[s_ord[s]];
                    run += xs[u];
                    if (s + 1 == n || s_lab[s_ord[s + 1]] != L) {
                        float* dst = slab + (size_t)L * D + d;
                        V::store(dst, s_seen[L] ? V::load(dst) + run : run);
                        run = V::zero();
                    }
                }
            }
        }
        __syncthreads();
        if (tid == 0)
            for (int s = 0; s < n; ++s) s_seen[s_lab[s_ord[s]]] = 1;
        __syncthreads();
    }
    // clusters this workgroup never saw: zero slab rows; counts and the changed total
    for (int j = 0; j < k; ++j) {
        if (s_seen[j]) continue;
        for (int d = tid; d < D; d += KM_THREADS) slab[(size_t)j * D + d] = 0.f;
    }
    for (int j = tid; j < k; j += KM_THREADS) p.cnt[(size_t)blockIdx.x * k + j] = s_cnt[j];
    if (tid == 0) p.chg[blockIdx.x] = s_changed;
}

__device__ int first_argmax(const int64_t* counts, int k) {      // np.argmax
    int a = 0;
    for (int j = 1; j < k; ++j)
        if (counts[j] > counts[a]) a = j;
    return a;
}

// status[0] = changed labels, status[2] = empty clusters, status[3] = inertia = sum(mind) (fp64, fixed order);
// counts[j] = sum_g cnt[g][j]
__global__ __launch_bounds__(KM_RED_THREADS) void kmeans_counts_kernel(const int* __restrict__ cnt, const int* __restrict__ chg,
                                                                       int G, int k, const float* __restrict__ mind, long N,
                                                                       int64_t* __restrict__ counts, int* __restrict__ amax,
                                                                       double* __restrict__ status) {
    __shared__ double sh[KM_RED_THREADS];
    double in = 0.0;
    for (long i = threadIdx.x; i < N; i += KM_RED_THREADS) in += (double)mind[i];
    in = block_sum_f64<KM_RED_THREADS>(in, sh);
    double ch = 0.0;
    for (int g = threadIdx.x; g < G; g += KM_RED_THREADS) ch += (double)chg[g];
    ch = block_sum_f64<KM_RED_THREADS>(ch, sh);
    double empty = 0.0;
    for (int j = threadIdx.x; j < k; j += KM_RED_THREADS) {
        long c = 0;
        for (int g = 0; g < G; ++g) c += cnt[(size_t)g * k + j];
        counts[j] = c;
        empty += c == 0 ? 1.0 : 0.0;
    }
    empty = block_sum_f64<KM_RED_THREADS>(empty, sh);  // (its barriers make every counts[j] visible to thread 0)
    if (threadIdx.x == 0) {
        status[0] = ch; status[2] = empty; status[3] = in;
        *amax = first_argmax(counts, k);
    }
}

// sum_g slabs[g][e] in g order, or sums[e] when G == 0 (sums already hold the relocated totals)
__device__ __forceinline__ float cluster_sum(const float* __restrict__ slabs, int G, long kd, const float* sums, long e) {
    if (G == 0) return sums[e];
    float s = 0.f;
#pragma unroll 8
    for (int g = 0; g < G; ++g) s += slabs[(size_t)g * kd + e];
    return s;
}

// sums[j][d] = the cluster sums; new = _average_centers (_k_means_common.pyx): sums[j] * (1 / counts[j]), and an empty
// cluster takes the row of the heaviest cluster a = argmax(counts) -- averaged when a < j, the raw sum when a > j (sklearn
// overwrites in place, in j order); part[block] = the block's sum of (new - old)^2 (fp64)
__global__ __launch_bounds__(KM_RED_THREADS) void kmeans_centres_kernel(const float* __restrict__ slabs, int G, int k, int D,
                                                                        float* __restrict__ sums, const int64_t* __restrict__ counts,
                                                                        const int* __restrict__ amax,
                                                                        const float* __restrict__ Cold, float* __restrict__ Cnew,
                                                                        double* __restrict__ part) {
    __shared__ double sh[KM_RED_THREADS];
    const long kd = (long)k * D;
    const int a = *amax;
    double sh2 = 0.0;
    for (long e = (long)blockIdx.x * KM_RED_THREADS + threadIdx.x; e < kd; e += (long)gridDim.x * KM_RED_THREADS) {
        const float s = cluster_sum(slabs, G, kd, sums, e);
        if (G > 0) sums[e] = s;
        const long j = e / D, c = counts[j];
        const float o = Cold[e];
        float v;
        if (c > 0) {
            v = s * (1.0f / (float)c);
        } else {
            const float sa = cluster_sum(slabs, G, kd, sums, (long)a * D + (e - j * D));
            v = a < j ? sa * (1.0f / (float)counts[a]) : sa;
        }
        Cnew[e] = v;
        const double df = (double)v - (double)o;
        sh2 += df * df;
    }
    sh2 = block_sum_f64<KM_RED_THREADS>(sh2, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = sh2;
}

__global__ __launch_bounds__(KM_RED_THREADS) void kmeans_shift_kernel(const double* __restrict__ part, int P,
                                                                      double* __restrict__ status) {
    __shared__ double sh[KM_RED_THREADS];
    double s = 0.0;
    for (int i = threadIdx.x; i < P; i += KM_RED_THREADS) s += part[i];
    s = block_sum_f64<KM_RED_THREADS>(s, sh);
    if (threadIdx.x == 0) status[1] = s;
}

// _relocate_empty_clusters_dense, moves in the host's order: moves[2i] = empty cluster, moves[2i+1] = the far sample
__global__ __launch_bounds__(KM_RED_THREADS) void kmeans_relocate_kernel(const float* __restrict__ X, long ldx, int D, int k,
                                                                         const int64_t* __restrict__ labels,
                                                                         const int64_t* __restrict__ moves, int nmoves,
                                                                         float* __restrict__ sums, int64_t* __restrict__ counts,
                                                                         int* __restrict__ amax, double* __restrict__ status) {
    __shared__ double sh[KM_RED_THREADS];
    for (int i = 0; i < nmoves; ++i) {
        const long newc = moves[2 * i], far = moves[2 * i + 1];
        const long oldc = labels[far];
        for (int d = threadIdx.x; d < D; d += KM_RED_THREADS) {
            const float x = X[far * ldx + d];
            sums[oldc * D + d] -= x;
            sums[newc * D + d] = x;
        }
        __syncthreads();
        if (threadIdx.x == 0) { counts[newc] = 1; counts[oldc] -= 1; }
        __syncthreads();
    }
    double empty = 0.0;
    for (int j = threadIdx.x; j < k; j += KM_RED_THREADS) empty += counts[j] == 0 ? 1.0 : 0.0;
    empty = block_sum_f64<KM_RED_THREADS>(empty, sh);
    if (threadIdx.x == 0) { status[2] = empty; *amax = first_argmax(counts, k); }
}

// _kmeans_plusplus: dist[t][i] = min(closest[i], |x_i - x_cand[t]|^2), one wave per row
__global__ __launch_bounds__(256) void kmeanspp_dist_kernel(const float* __restrict__ X, long ldx, long N, int D,
                                                            const int64_t* __restrict__ cand, int T,
                                                            const float* __restrict__ closest, float* __restrict__ dist) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    const float* xi = X + i * ldx;
    for (int t = 0; t < T; ++t) {
        const float* xc = X + cand[t] * ldx;
        float s = 0.f;
        for (int d = lane; d < D; d += 64) { const float e = xi[d] - xc[d]; s = fmaf(e, e, s); }
        s = wave_sum(s);
        if (lane == 0) dist[(size_t)t * N + i] = closest ? fminf(closest[i], s) : s;
    }
}

// pots[t] = sum_i dist[t][i] (fp64, fixed order), one block per candidate
__global__ __launch_bounds__(KM_RED_THREADS) void kmeanspp_pot_kernel(const float* __restrict__ dist, long N,
                                                                      double* __restrict__ pots) {
    __shared__ double sh[KM_RED_THREADS];
    const float* d = dist + (size_t)blockIdx.x * N;
    double s = 0.0;
    for (long i = threadIdx.x; i < N; i += KM_RED_THREADS) s += (double)d[i];
    s = block_sum_f64<KM_RED_THREADS>(s, sh);
    if (threadIdx.x == 0) pots[blockIdx.x] = s;
}

// _tolerance: per row chunk and column fp64 sum and sum of squares -> part[c][0|1][D]
__global__ __launch_bounds__(256) void kmeans_colstats_kernel(const float* __restrict__ X, long ldx, long N, int D,
                                                              double* __restrict__ part) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= D) return;
    const long per = (N + gridDim.y - 1) / gridDim.y;
    const long a = (long)blockIdx.y * per, b = min(N, a + per);
    double s = 0.0, q = 0.0;
    for (long i = a; i < b; ++i) { const double x = X[i * ldx + d]; s += x; q += x * x; }
    part[((size_t)blockIdx.y * 2) * D + d] = s;
    part[((size_t)blockIdx.y * 2 + 1) * D + d] = q;
}

// out[0] = mean_d var_d (population variance, np.var), chunks summed in order
__global__ __launch_bounds__(KM_RED_THREADS) void kmeans_colvar_kernel(const double* __restrict__ part, int chunks, long N, int D,
                                                                       double* __restrict__ out) {
    __shared__ double sh[KM_RED_THREADS];
    double acc = 0.0;
    for (int d = threadIdx.x; d < D; d += KM_RED_THREADS) {
        double s = 0.0, q = 0.0;
        for (int c = 0; c < chunks; ++c) { s += part[(size_t)c * 2 * D + d]; q += part[((size_t)c * 2 + 1) * D + d]; }
        const double m = s / (double)N;
        acc += fmax(q / (double)N - m * m, 0.0);
    }
    acc = block_sum_f64<KM_RED_THREADS>(acc, sh);
    if (threadIdx.x == 0) out[0] = acc / (double)D;
}

template <int KC, int VEC>
int launch_assign(const AssignP& p, int G, hipStream_t stream) {
    return row_tile_launch<AssignP, kmeans_assign_kernel<KC, VEC>>(p, G, KM_THREADS, (size_t)KC * p.dt * 4 + (size_t)2 * p.k * 4,
                                                                   KM_LDS + 2 * KM_MAX_K * 4, "kmeans_assign_kernel", stream);
}

}  // namespace
}  // namespace vsom

extern "C" {

size_t vsom_kmeans_workspace_bytes(long N, int D, int k) {
    if (N < 1 || D < 1 || k < 1) return 0;
    return vsom::km_layout(nullptr, N, D, k).bytes;
}

int vsom_kmeans_assign(const float* X, long ldx, long N, int D, const float* centers, int k, int64_t* labels,
                       const int64_t* prev_labels, float* mind, void* ws, size_t ws_bytes, vsom_stream_t stream) {
    using namespace vsom;
    VSOM_REQUIRE(X && centers && labels && prev_labels && mind, VSOM_EINVAL, "kmeans_assign: null pointer");
    VSOM_REQUIRE(N >= 1 && D >= 1 && k >= 1 && k <= N && ldx >= D, VSOM_EINVAL,
                 "kmeans_assign: bad sizes N=%ld D=%d k=%d ldx=%ld", N, D, k, ldx);
    VSOM_REQUIRE(k <= KM_MAX_K, VSOM_EUNSUPPORTED, "kmeans_assign: k=%d > %d", k, KM_MAX_K);
    VSOM_REQUIRE(ws && aligned16(ws) && ws_bytes >= vsom_kmeans_workspace_bytes(N, D, k), VSOM_EWORKSPACE,
                 "kmeans_assign: workspace too small or misaligned");
    const KmWs w = km_layout(ws, N, D, k);
    AssignP p = {};
    p.X = X; p.ldx = ldx; p.N = N; p.D = D; p.k = k; p.C = centers;
    p.labels = labels; p.prev = prev_labels; p.mind = mind;
    p.slabs = w.slabs; p.cnt = w.cnt; p.chg = w.chg;
    p.rows_per_group = w.rows_per_group;
    const bool vec = D % 4 == 0 && ldx % 4 == 0 && aligned16(X) && aligned16(centers);
    const int KC = k <= 4 ? 4 : k <= 8 ? 8 : k <= 12 ? 12 : 16;
    p.dt = row_tile_width(KM_LDS, 1, KC, vec ? 4 : 1, D);
    switch (KC * 2 + (vec ? 1 : 0)) {
        case 9: return launch_assign<4, 4>(p, w.G, stream);
        case 8: return launch_assign<4, 1>(p, w.G, stream);
        case 17: return launch_assign<8, 4>(p, w.G, stream);
        case 16: return launch_assign<8, 1>(p, w.G, stream);
        case 25: return launch_assign<12, 4>(p, w.G, stream);
        case 24: return launch_assign<12, 1>(p, w.G, stream);
        case 33: return launch_assign<16, 4>(p, w.G, stream);
        default: return launch_assign<16, 1>(p, w.G, stream);
    }
}

int vsom_kmeans_update(const float* centers_old, float* centers_new, long N, int D, int k, const float* mind,
                       int64_t* counts, double* status, void* ws, size_t ws_bytes, vsom_stream_t stream) {
    using namespace vsom;
    VSOM_REQUIRE(centers_old && centers_new && mind && counts && status, VSOM_EINVAL, "kmeans_update: null pointer");
    VSOM_REQUIRE(N >= 1 && D >= 1 && k >= 1 && k <= N, VSOM_EINVAL, "kmeans_update: bad sizes N=%ld D=%d k=%d", N, D, k);
    VSOM_REQUIRE(centers_old != centers_new, VSOM_EINVAL, "kmeans_update: centers_new must not alias centers_old");
    VSOM_REQUIRE(ws && aligned16(ws) && ws_bytes >= vsom_kmeans_workspace_bytes(N, D, k), VSOM_EWORKSPACE,
                 "kmeans_update: workspace too small or misaligned");
    const KmWs w = km_layout(ws, N, D, k);
    const int P = km_shift_blocks(D, k);
    VSOM_LAUNCH(kmeans_counts_kernel, dim3(1), dim3(KM_RED_THREADS), 0, stream, w.cnt, w.chg, w.G, k, mind, N, counts, w.amax,
                status);
    VSOM_LAUNCH(kmeans_centres_kernel, dim3(P), dim3(KM_RED_THREADS), 0, stream, w.slabs, w.G, k, D, w.sums, counts, w.amax, centers_old,
                centers_new, w.part);
    VSOM_LAUNCH(kmeans_shift_kernel, dim3(1), dim3(KM_RED_THREADS), 0, stream, w.part, P, status);
    return launch_status("kmeans_update");
}

int vsom_kmeans_relocate(const float* X, long ldx, long N, int D, int k, const int64_t* labels, const int64_t* moves,
                         int n_moves, const float* centers_old, float* centers_new, int64_t* counts, double* status,
                         void* ws, size_t ws_bytes, vsom_stream_t stream) {
    using namespace vsom;
    VSOM_REQUIRE(X && labels && moves && centers_old && centers_new && counts && status, VSOM_EINVAL,
                 "kmeans_relocate: null pointer");
    VSOM_REQUIRE(N >= 1 && D >= 1 && k >= 1 && k <= N && ldx >= D && n_moves >= 1 && n_moves <= k, VSOM_EINVAL,
                 "kmeans_relocate: bad sizes");
    VSOM_REQUIRE(centers_old != centers_new, VSOM_EINVAL, "kmeans_relocate: centers_new must not alias centers_old");
    VSOM_REQUIRE(ws && aligned16(ws) && ws_bytes >= vsom_kmeans_workspace_bytes(N, D, k), VSOM_EWORKSPACE,
                 "kmeans_relocate: workspace too small or misaligned");
    const KmWs w = km_layout(ws, N, D, k);
    const int P = km_shift_blocks(D, k);
    VSOM_LAUNCH(kmeans_relocate_kernel, dim3(1), dim3(KM_RED_THREADS), 0, stream, X, ldx, D, k, labels, moves, n_moves, w.sums,
                counts, w.amax, status);
    VSOM_LAUNCH(kmeans_centres_kernel, dim3(P), dim3(KM_RED_THREADS), 0, stream, (const float*)nullptr, 0, k, D, w.sums, counts, w.amax,
                centers_old, centers_new, w.part);
    VSOM_LAUNCH(kmeans_shift_kernel, dim3(1), dim3(KM_RED_THREADS), 0, stream, w.part, P, status);
    return launch_status("kmeans_relocate");
}

int vsom_kmeanspp_dist(const float* X, long ldx, long N, int D, const int64_t* candidates, int n_candidates,
                       const float* closest, float* dist, double* pots, vsom_stream_t stream) {
    using namespace vsom;
    VSOM_REQUIRE(X && candidates && dist && pots, VSOM_EINVAL, "kmeanspp_dist: null pointer");
    VSOM_REQUIRE(N >= 1 && D >= 1 && ldx >= D && n_candidates >= 1 && n_candidates <= 64, VSOM_EINVAL,
                 "kmeanspp_dist: bad sizes N=%ld D=%d ldx=%ld T=%d", N, D, ldx, n_candidates);
    VSOM_LAUNCH(kmeanspp_dist_kernel, dim3(cdiv(N, 4)), dim3(256), 0, stream, X, ldx, N, D, candidates, n_candidates, closest,
                dist);
    VSOM_LAUNCH(kmeanspp_pot_kernel, dim3(n_candidates), dim3(KM_RED_THREADS), 0, stream, dist, N, pots);
    return launch_status("kmeanspp_dist");
}

int vsom_kmeans_colvar(const float* X, long ldx, long N, int D, int k, double* out, void* ws, size_t ws_bytes,
                       vsom_stream_t stream) {
    using namespace vsom;
    VSOM_REQUIRE(X && out, VSOM_EINVAL, "kmeans_colvar: null pointer");
    VSOM_REQUIRE(N >= 1 && D >= 1 && k >= 1 && k <= N && ldx >= D, VSOM_EINVAL, "kmeans_colvar: bad sizes");
    VSOM_REQUIRE(ws && aligned16(ws) && ws_bytes >= vsom_kmeans_workspace_bytes(N, D, k), VSOM_EWORKSPACE,
                 "kmeans_colvar: workspace too small or misaligned");
    const KmWs w = km_layout(ws, N, D, k);
    double* part = reinterpret_cast<double*>(w.slabs);
    VSOM_LAUNCH(kmeans_colstats_kernel, dim3(cdiv(D, 256), KM_COLVAR_CHUNKS), dim3(256), 0, stream, X, ldx, N, D, part);
    VSOM_LAUNCH(kmeans_colvar_kernel, dim3(1), dim3(KM_RED_THREADS), 0, stream, part, KM_COLVAR_CHUNKS, N, D, out);
    return launch_status("kmeans_colvar");
}

}  // extern "C"
