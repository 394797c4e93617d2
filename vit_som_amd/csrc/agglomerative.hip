// Agglomerative clustering for vit_som_amd/agglomerative.py ("Agglomerative clustering"): the two parts
// of sklearn.cluster.AgglomerativeClustering / scipy.cluster.hierarchy.linkage that cost time.
//
//   vsom_agglo_distances   the full symmetric [N, N] fp64 matrix in the DIRECT form -- sum (x - y)^2, sum |x - y|,
//                          1 - x.y / sqrt(|x|^2 |y|^2) -- every difference, product and sum in fp64 on the f32 values.
//                          64 x 64 tiles of the upper triangle, 32 columns of both row blocks staged through LDS, a 4 x 4
//                          block of pairs per thread; the tile is written to both halves, so D[i, j] and D[j, i] are the
//                          same bits.
//   vsom_agglo_merge       the generic greedy algorithm with a nearest-neighbour array, all N - 1 steps enqueued from here:
//                          pick (one workgroup: the minimum of (distance, smaller slot, larger slot), a total order),
//                          update (Lance-Williams on row and column b, adjacency rows OR-ed, neighbours taken or
//                          flagged), rescan (one workgroup per flagged slot).
//
// No floating-point atomics, no cooperative launch, no loop that waits for another workgroup: every dependency is a kernel
// boundary and every trip count is fixed by N and D.  Two runs on the same input give the same bits.
#include <limits.h>
#include <math.h>

#include "common.h"

namespace vsom {
namespace {

constexpr int AG_MAX_N = 16384;              // the fp64 matrix is then 2 GiB
constexpr int AG_TILE = 64;                  // pairs tile: 64 x 64
constexpr int AG_KC = 32;                    // columns staged per step
constexpr int AG_LD = AG_TILE + 4;           // LDS row stride in floats: 272 bytes, a multiple of 16
constexpr int AG_THREADS = 256;              // 16 x 16 threads, 4 x 4 pairs each
constexpr int AG_PICK_THREADS = 1024;
constexpr int AG_ROW_THREADS = 256;          // update: one slot per thread; rescan: one workgroup per slot

// ---- the three metrics: what one column adds to a pair's fp64 accumulator
struct Euclid {
    static constexpr bool NORMS = false, ROOT = true;
    static __device__ __forceinline__ double term(double x, double y, double acc) {
        const double e = x - y;              // exact: both are f32 values
        return fma(e, e, acc);
    }
};
struct Manhattan {
    static constexpr bool NORMS = false, ROOT = false;
    static __device__ __forceinline__ double term(double x, double y, double acc) { return acc + fabs(x - y); }
};
struct Cosine {
    static constexpr bool NORMS = true, ROOT = false;
    static __device__ __forceinline__ double term(double x, double y, double acc) { return fma(x, y, acc); }
};

__device__ __forceinline__ int nonfinite(float v) { return isfinite(v) ? 0 : 1; }

// Tile (bi, bj), bi <= bj, of the matrix.  status[0] counts the values of X that are not finite, status[1] the rows of
// zero length (cosine); both are counted by the diagonal tiles alone, which stage every row exactly once.
template <class M, int VEC>
__global__ __launch_bounds__(AG_THREADS) void agglo_dist_kernel(const float* __restrict__ X, long ldx, int N, int D, int squared,
                                                                double* __restrict__ out, long ldo, int* __restrict__ status) {
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bi > bj) return;
    __shared__ __attribute__((aligned(16))) float sa[AG_KC][AG_LD];
    __shared__ __attribute__((aligned(16))) float sb[AG_KC][AG_LD];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int i0 = bi * AG_TILE, j0 = bj * AG_TILE;
    double acc[4][4], na[4], nb[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        na[r] = 0.0; nb[r] = 0.0;
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
    }
    int bad = 0;
    for (int k0 = 0; k0 < D; k0 += AG_KC) {
        if (VEC == 4) {                                               // D % 4 == 0: a quad is inside the row or past it
            for (int e = tid; e < AG_TILE * AG_KC / 4; e += AG_THREADS) {
                const int row = e >> 3, q = e & 7, k = k0 + 4 * q;
                f32x4 va = {0.f, 0.f, 0.f, 0.f}, vb = {0.f, 0.f, 0.f, 0.f};
                if (k < D) {
                    if (i0 + row < N) va = *reinterpret_cast<const f32x4*>(X + (size_t)(i0 + row) * ldx + k);
                    if (j0 + row < N) vb = *reinterpret_cast<const f32x4*>(X + (size_t)(j0 + row) * ldx + k);
                }
                sa[4 * q + 0][row] = va.x; sa[4 * q + 1][row] = va.y; sa[4 * q + 2][row] = va.z; sa[4 * q + 3][row] = va.w;
                sb[4 * q + 0][row] = vb.x; sb[4 * q + 1][row] = vb.y; sb[4 * q + 2][row] = vb.z; sb[4 * q + 3][row] = vb.w;
                bad += nonfinite(va.x) + nonfinite(va.y) + nonfinite(va.z) + nonfinite(va.w);
            }
        } else {
            for (int e = tid; e < AG_TILE * AG_KC; e += AG_THREADS) {
                const int row = e >> 5, kk = e & 31, k = k0 + kk;
                float va = 0.f, vb = 0.f;
                if (k < D) {
                    if (i0 + row < N) va = X[(size_t)(i0 + row) * ldx + k];
                    if (j0 + row < N) vb = X[(size_t)(j0 + row) * ldx + k];
                }
                sa[kk][row] = va;
                sb[kk][row] = vb;
                bad += nonfinite(va);
            }
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < AG_KC; ++kk) {                          // columns past D hold zeros: they add nothing
            const f32x4 a4 = *reinterpret_cast<const f32x4*>(&sa[kk][ty * 4]);
            const f32x4 b4 = *reinterpret_cast<const f32x4*>(&sb[kk][tx * 4]);
            const double a[4] = {(double)a4.x, (double)a4.y, (double)a4.z, (double)a4.w};
            const double b[4] = {(double)b4.x, (double)b4.y, (double)b4.z, (double)b4.w};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[r][c] = M::term(a[r], b[c], acc[r][c]);
                if (M::NORMS) {
                    na[r] = fma(a[r], a[r], na[r]);
                    nb[r] = fma(b[r], b[r], nb[r]);
                }
            }
        }
        __syncthreads();
    }
    if (bi == bj && bad) atomicAdd(status, bad);                      // an integer count
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = i0 + ty * 4 + r;
        if (i >= N) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = j0 + tx * 4 + c;
            if (j >= N) continue;
            double v = acc[r][c];
            if (M::NORMS) {
                const double den = __dsqrt_rn(na[r] * nb[c]);         // sqrt(s * s) == s: identical rows give 1 - 1
                v = den > 0.0 ? 1.0 - v / den : 1.0;
                v = v > 0.0 ? v : 0.0;
                if (i == j && !(na[r] > 0.0)) atomicAdd(status + 1, 1);
            } else if (M::ROOT && !squared) {
                v = __dsqrt_rn(v);
            }
            if (i == j) v = 0.0;
            out[(size_t)i * ldo + j] = v;
            if (bi != bj) out[(size_t)j * ldo + i] = v;               // a diagonal tile computes both halves, in the same order
        }
    }
}

__global__ void agglo_clear_kernel(int* __restrict__ status, int n) {
    if ((int)threadIdx.x < n) status[threadIdx.x] = 0;
}

// ---- the merge loop's state, carved from the workspace after the matrix and the adjacency
struct Slots {
    double* M;                // [N][N]
    unsigned char* adj;       // [N][N] or null
    int* active;              // [N]
    int* size;                // [N]
    int* id;                  // [N] the cluster a slot holds, in scipy's numbering
    int* nn;                  // [N] nearest active adjacent slot, -1: none
    int* flag;                // [N] the slot's nearest has to be searched again
    double* nnd;              // [N] its distance
    int* rec_i;               // the step's pair: a, b, size of a, size of b, "a slot other than b was flagged"
    double* rec_d;            // its distance
};
struct Layout { size_t adj, active, size, id, nn, flag, nnd, rec, total; };
inline Layout ag_layout(long N, int connectivity) {
    Layout l;
    const size_t n = (size_t)N;
    size_t o = align256(n * n * 8);
    l.adj = o;    o += connectivity ? align256(n * n) : 0;
    l.active = o; o += align256(n * 4);
    l.size = o;   o += align256(n * 4);
    l.id = o;     o += align256(n * 4);
    l.nn = o;     o += align256(n * 4);
    l.flag = o;   o += align256(n * 4);
    l.nnd = o;    o += align256(n * 8);
    l.rec = o;    o += 256;
    l.total = o;
    return l;
}

// (distance, smaller slot, larger slot): a total order over the pairs.  A NaN distance never wins.
__device__ __forceinline__ bool key_less(double d1, int lo1, int hi1, double d2, int lo2, int hi2) {
    return d1 < d2 || (d1 == d2 && (lo1 < lo2 || (lo1 == lo2 && hi1 < hi2)));
}

// the least key of a workgroup, on every thread; "none" is (inf, INT_MAX, INT_MAX)
template <int THREADS>
__device__ void block_min_key(double& d, int& lo, int& hi, double* sd, int* slo, int* shi) {
    const int t = threadIdx.x;
    sd[t] = d; slo[t] = lo; shi[t] = hi;
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (t < s && key_less(sd[t + s], slo[t + s], shi[t + s], sd[t], slo[t], shi[t])) {
            sd[t] = sd[t + s]; slo[t] = slo[t + s]; shi[t] = shi[t + s];
        }
        __syncthreads();
    }
    d = sd[0]; lo = slo[0]; hi = shi[0];
    __syncthreads();
}

__global__ __launch_bounds__(AG_ROW_THREADS) void agglo_init_kernel(Slots s, int N, int* __restrict__ status) {
    const int k = blockIdx.x * AG_ROW_THREADS + threadIdx.x;
    if (k < N) {
        s.active[k] = 1; s.size[k] = 1; s.id[k] = k; s.nn[k] = -1; s.flag[k] = 1;
        s.nnd[k] = INFINITY;
    }
    if (k < 4) status[k] = 0;
    if (k < 8) s.rec_i[k] = k < 2 ? -1 : 0;
    if (k == 0) s.rec_d[0] = 0.0;
}

// Step `step`: the least (distance, smaller slot, larger slot) over the slots' nearest neighbours -> the pair (a, b), a < b,
// children[step] (smaller id first), distances[step] (the square root for Ward).  The merged cluster takes slot b.
__global__ __launch_bounds__(AG_PICK_THREADS) void agglo_pick_kernel(Slots s, int N, int step, int ward, int* __restrict__ children,
                                                                     double* __restrict__ distances, int* __restrict__ status) {
    __shared__ double sd[AG_PICK_THREADS];
    __shared__ int slo[AG_PICK_THREADS], shi[AG_PICK_THREADS];
    double d = INFINITY;
    int lo = INT_MAX, hi = INT_MAX;
    for (int k = threadIdx.x; k < N; k += AG_PICK_THREADS) {
        const int j = s.nn[k];
        if (!s.active[k] || j < 0) continue;
        const int l = k < j ? k : j, h = k < j ? j : k;
        const double v = s.nnd[k];
        if (key_less(v, l, h, d, lo, hi)) { d = v; lo = l; hi = h; }
    }
    block_min_key<AG_PICK_THREADS>(d, lo, hi, sd, slo, shi);
    if (threadIdx.x != 0) return;
    status[2] += s.rec_i[4];                          // the step before flagged a slot other than its b
    s.rec_i[4] = 0;
    if (lo == INT_MAX) {                              // no two adjacent clusters are left: the graph has another component
        s.rec_i[0] = -1; s.rec_i[1] = -1;
        children[2 * step] = -1; children[2 * step + 1] = -1;
        distances[step] = NAN;
        status[0] += 1;
        return;
    }
    const int a = lo, b = hi, ia = s.id[a], ib = s.id[b];
    children[2 * step] = ia < ib ? ia : ib;
    children[2 * step + 1] = ia < ib ? ib : ia;
    distances[step] = ward ? __dsqrt_rn(d) : d;
    s.rec_i[0] = a; s.rec_i[1] = b; s.rec_i[2] = s.size[a]; s.rec_i[3] = s.size[b];
    s.rec_d[0] = d;
    s.active[a] = 0;
    s.size[b] += s.size[a];
    s.id[b] = N + step;
}

// d(k, a + b) from d(k, a), d(k, b), d(a, b) and the three sizes.  No contraction: the host restatement rounds every
// product, sum and quotient once, and ties have to fall the same way on both sides.
__device__ __forceinline__ double lance_williams(int linkage, double dka, double dkb, double dab, int na, int nb, int nk) {
#pragma clang fp contract(off)
    switch (linkage) {
        case VSOM_AGGLO_SINGLE: return dka < dkb ? dka : dkb;
        case VSOM_AGGLO_COMPLETE: return dka > dkb ? dka : dkb;
        case VSOM_AGGLO_AVERAGE: {
            const double x = (double)na, y = (double)nb;
            return (x * dka + y * dkb) / (x + y);
        }
        default: {                                    // Ward, on squared distances
            const double t = (double)(na + nb + nk);
            const double r = ((double)(nk + na) * dka + (double)(nk + nb) * dkb - (double)nk * dab) / t;
            return r > 0.0 ? r : 0.0;
        }
    }
}

// Thread k: row and column b of the matrix (and of the adjacency) at slot k, then k's nearest neighbour: b when the new
// distance wins under the order, a flag when it was a or b.  Rows a and b are read, entry (b, k) and (k, b) written: no
// thread reads what another writes.
__global__ __launch_bounds__(AG_ROW_THREADS) void agglo_update_kernel(Slots s, int N, int linkage, int* __restrict__ status) {
    const int a = s.rec_i[0];
    if (a < 0) return;
    const int b = s.rec_i[1], na = s.rec_i[2], nb = s.rec_i[3];
    const int k = blockIdx.x * AG_ROW_THREADS + threadIdx.x;
    if (k >= N) return;
    if (k == b) { s.flag[b] = 1; return; }
    if (!s.active[k]) return;                         // a retired in the pick
    const size_t n = (size_t)N;
    const double dn = lance_williams(linkage, s.M[a * n + k], s.M[b * n + k], s.rec_d[0], na, nb, s.size[k]);
    s.M[b * n + k] = dn;
    s.M[k * n + b] = dn;
    bool adjacent = true;
    if (s.adj) {
        const unsigned char u = s.adj[a * n + k] | s.adj[b * n + k];
        s.adj[b * n + k] = u;
        s.adj[k * n + b] = u;
        adjacent = u != 0;
    }
    const int j = s.nn[k];
    if (j == a || j == b) {
        s.flag[k] = 1;
        s.rec_i[4] = 1;                               // every writer stores the same value
        atomicAdd(status + 1, 1);
    } else if (adjacent) {
        const int l = k < b ? k : b, h = k < b ? b : k;
        if (j < 0 || key_less(dn, l, h, s.nnd[k], k < j ? k : j, k < j ? j : k)) { s.nn[k] = b; s.nnd[k] = dn; }
    }
}

// Workgroup k: nothing unless slot k is flagged; else its nearest active adjacent slot under the order, from row k.
__global__ __launch_bounds__(AG_ROW_THREADS) void agglo_rescan_kernel(Slots s, int N) {
    __shared__ double sd[AG_ROW_THREADS];
    __shared__ int slo[AG_ROW_THREADS], shi[AG_ROW_THREADS];
    const int k = blockIdx.x;
    if (!s.flag[k]) return;                           // uniform over the workgroup
    const double* row = s.M + (size_t)k * N;
    const unsigned char* arow = s.adj ? s.adj + (size_t)k * N : nullptr;
    double d = INFINITY;
    int lo = INT_MAX, hi = INT_MAX;
    for (int j = threadIdx.x; j < N; j += AG_ROW_THREADS) {
        if (j == k || !s.active[j] || (arow && !arow[j])) continue;
        const int l = k < j ? k : j, h = k < j ? j : k;
        const double v = row[j];
        if (key_less(v, l, h, d, lo, hi)) { d = v; lo = l; hi = h; }
    }
    block_min_key<AG_ROW_THREADS>(d, lo, hi, sd, slo, shi);
    if (threadIdx.x == 0) {
        s.nn[k] = lo == INT_MAX ? -1 : (lo == k ? hi : lo);
        s.nnd[k] = d;
        s.flag[k] = 0;
    }
}

template <class M>
int launch_distances(bool vec, const float* X, long ldx, int N, int D, int squared, double* out, long ldo, int* status,
                     hipStream_t stream) {
    const int T = cdiv(N, AG_TILE);
    if (vec)
        VSOM_LAUNCH((agglo_dist_kernel<M, 4>), dim3(T, T), dim3(AG_THREADS), 0, stream, X, ldx, N, D, squared, out, ldo, status);
    else
        VSOM_LAUNCH((agglo_dist_kernel<M, 1>), dim3(T, T), dim3(AG_THREADS), 0, stream, X, ldx, N, D, squared, out, ldo, status);
    return launch_status("agglo_dist_kernel");
}

}  // namespace
}  // namespace vsom

extern "C" {

long vsom_agglo_workspace_bytes(long N, int connectivity) {
    using namespace vsom;
    if (N < 1 || N > AG_MAX_N) return 0;
    return (long)ag_layout(N, connectivity).total;
}

int vsom_agglo_distances(const float* X, long ldx, long N, int D, int metric, int squared, double* out, long ldo, int* status,
                         vsom_stream_t stream) {
    using namespace vsom;
    VSOM_REQUIRE(X && out && status, VSOM_EINVAL, "agglo_distances: null pointer");
    VSOM_REQUIRE(N >= 1 && D >= 1 && ldx >= D && ldo >= N, VSOM_EINVAL, "agglo_distances: bad sizes N=%ld D=%d ldx=%ld ldo=%ld", N, D,
                 ldx, ldo);
    VSOM_REQUIRE(N <= AG_MAX_N, VSOM_EUNSUPPORTED, "agglo_distances: N=%ld > %d (the fp64 matrix would pass 2 GiB)", N, AG_MAX_N);
    VSOM_REQUIRE(metric == VSOM_AGGLO_EUCLIDEAN || metric == VSOM_AGGLO_MANHATTAN || metric == VSOM_AGGLO_COSINE, VSOM_EUNSUPPORTED,
                 "agglo_distances: metric %d is none of euclidean (0), manhattan (1), cosine (2)", metric);
    VSOM_LAUNCH(agglo_clear_kernel, dim3(1), dim3(64), 0, stream, status, 2);
    const bool vec = D % 4 == 0 && ldx % 4 == 0 && aligned16(X);
    switch (metric) {
        case VSOM_AGGLO_EUCLIDEAN: return launch_distances<Euclid>(vec, X, ldx, (int)N, D, squared, out, ldo, status, stream);
        case VSOM_AGGLO_MANHATTAN: return launch_distances<Manhattan>(vec, X, ldx, (int)N, D, squared, out, ldo, status, stream);
        default: return launch_distances<Cosine>(vec, X, ldx, (int)N, D, squared, out, ldo, status, stream);
    }
}

int vsom_agglo_merge(void* ws, long ws_size, long N, int linkage, int connectivity, int* children, double* distances, int* status,
                     vsom_stream_t stream) {
    using namespace vsom;
    VSOM_REQUIRE(children && distances && status, VSOM_EINVAL, "agglo_merge: null pointer");
    VSOM_REQUIRE(N >= 2, VSOM_EINVAL, "agglo_merge: bad size N=%ld (at least 2 rows)", N);
    VSOM_REQUIRE(N <= AG_MAX_N, VSOM_EUNSUPPORTED, "agglo_merge: N=%ld > %d (the fp64 matrix would pass 2 GiB)", N, AG_MAX_N);
    VSOM_REQUIRE(linkage >= VSOM_AGGLO_WARD && linkage <= VSOM_AGGLO_SINGLE, VSOM_EUNSUPPORTED,
                 "agglo_merge: linkage %d is none of ward (0), average (1), complete (2), single (3)", linkage);
    const Layout l = ag_layout(N, connectivity);
    VSOM_REQUIRE(ws && ws_size >= (long)l.total, VSOM_EWORKSPACE, "agglo_merge: workspace holds %ld bytes < %ld (too small)",
                 ws ? ws_size : 0L, (long)l.total);
    VSOM_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7u) == 0, VSOM_EALIGN, "agglo_merge: the workspace is not 8-byte aligned");
    char* base = static_cast<char*>(ws);
    Slots s;
    s.M = reinterpret_cast<double*>(base);
    s.adj = connectivity ? reinterpret_cast<unsigned char*>(base + l.adj) : nullptr;
    s.active = reinterpret_cast<int*>(base + l.active);
    s.size = reinterpret_cast<int*>(base + l.size);
    s.id = reinterpret_cast<int*>(base + l.id);
    s.nn = reinterpret_cast<int*>(base + l.nn);
    s.flag = reinterpret_cast<int*>(base + l.flag);
    s.nnd = reinterpret_cast<double*>(base + l.nnd);
    s.rec_i = reinterpret_cast<int*>(base + l.rec);
    s.rec_d = reinterpret_cast<double*>(base + l.rec + 64);
    const int n = (int)N, blocks = cdiv(N, AG_ROW_THREADS), ward = linkage == VSOM_AGGLO_WARD;
    VSOM_LAUNCH(agglo_init_kernel, dim3(blocks), dim3(AG_ROW_THREADS), 0, stream, s, n, status);
    VSOM_LAUNCH(agglo_rescan_kernel, dim3(n), dim3(AG_ROW_THREADS), 0, stream, s, n);
    for (int step = 0; step < n - 1; ++step) {
        VSOM_LAUNCH(agglo_pick_kernel, dim3(1), dim3(AG_PICK_THREADS), 0, stream, s, n, step, ward, children, distances, status);
        VSOM_LAUNCH(agglo_update_kernel, dim3(blocks), dim3(AG_ROW_THREADS), 0, stream, s, n, linkage, status);
        VSOM_LAUNCH(agglo_rescan_kernel, dim3(n), dim3(AG_ROW_THREADS), 0, stream, s, n);
        if (step % 256 == 255) {
            const int rc = launch_status("agglo_merge");
            if (rc != VSOM_OK) return rc;
        }
    }
    return launch_status("agglo_merge");
}

}  // extern "C"
