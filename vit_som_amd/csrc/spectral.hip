// Spectral embedding for vit_som_amd/spectral.py ("Spectral embedding"): the device side of a
// Chebyshev-filtered subspace iteration on M = D^-1/2 A D^-1/2, A a symmetric affinity in CSR (int64 indptr / indices, fp64
// data, the convention of vsom_tsne_step) with its diagonal ignored.  Everything is fp64: weights, the block, the sums.
//
//   vsom_spectral_degrees   d = row sums without the diagonal, s = d^-1/2, the list of rows longer than one chunk, refusals.
//   vsom_spectral_spmm      Yout = alpha (M Y1 - c Y1) - beta Y0 on a row-major [N, l] block, l <= 32: lanes are block
//                           columns, so one neighbour's block row is one contiguous gather.
//   vsom_spectral_gram      G = V^T V and H = V^T W, row slabs summed in slab order.
//   vsom_spectral_rotate    Vout = V T.
//   vsom_spectral_residual  per column |W_j - theta_j V_j|^2, computed from the differences themselves.
//   vsom_spectral_embed     E = sign_j s_i V[i, first + j] as f32, sklearn's deterministic sign found here.
//
// The order of every sum is fixed by the operands alone.  A row's sum is cut into chunks of SP_CHUNK entries in CSR order:
// a chunk is one fma chain, the chunks' sums are added in chunk order.  A row of at most SP_CHUNK entries is therefore one
// chain; a longer row gives the same bits whether one lane group walks its chunks (no list of long rows given) or a
// workgroup of its own spreads them over eight groups (the list vsom_spectral_degrees writes).  No floating-point atomics,
// no cooperative launch, no loop that waits for another workgroup; every access is a natural 4- or 8-byte one.
#include <math.h>

#include "common.h"

namespace vsom {
namespace {

constexpr long SP_MAX_N = 131072;
constexpr int SP_MAX_L = 32;
constexpr int SP_CHUNK = 512;                // entries of one fma chain; a multiple of every group width
constexpr int SP_THREADS = 256;
constexpr int SP_MAX_SLABS = 1024;
constexpr int SP_STATUS = 5;                 // isolated rows, bad indices, bad weights, bad indptr, long rows
constexpr int SP_TILE = 32;                  // rows of V and W staged per step of the Gram kernel

__global__ void spectral_clear_kernel(int64_t* status) {
    if (threadIdx.x < SP_STATUS) status[threadIdx.x] = 0;
}

// The entries [p0, p1) of row `row`, or an empty range when indptr does not describe one inside [0, nnz].
__device__ __forceinline__ bool row_range(const int64_t* __restrict__ indptr, long row, long nnz, long& p0, long& p1) {
    p0 = indptr[row];
    p1 = indptr[row + 1];
    if (p0 < 0 || p1 < p0 || p1 > nnz) {
        p0 = p1 = 0;
        return false;
    }
    return true;
}

// One thread per row: the chain of the degree is the CSR order itself.
__global__ __launch_bounds__(SP_THREADS) void spectral_degrees_kernel(const int64_t* __restrict__ indptr, const int64_t* __restrict__ indices,
                                                                      const double* __restrict__ data, long N, long nnz,
                                                                      double* __restrict__ d, double* __restrict__ s,
                                                                      int32_t* __restrict__ heavy, int64_t* __restrict__ status) {
    const long row = (long)blockIdx.x * SP_THREADS + threadIdx.x;
    if (row >= N) return;
    long p0, p1;
    if (!row_range(indptr, row, nnz, p0, p1)) atomicAdd((unsigned long long*)(status + 3), 1ull);
    double sum = 0.0;
    int bad_index = 0, bad_weight = 0;
    for (long p = p0; p < p1; ++p) {
        const long j = indices[p];
        const double w = data[p];
        if (j < 0 || j >= N) { ++bad_index; continue; }
        if (!(w >= 0.0) || !isfinite(w)) { ++bad_weight; continue; }
        if (j != row) sum += w;
    }
    if (bad_index) atomicAdd((unsigned long long*)(status + 1), (unsigned long long)bad_index);
    if (bad_weight) atomicAdd((unsigned long long*)(status + 2), (unsigned long long)bad_weight);
    d[row] = sum;
    s[row] = sum > 0.0 ? 1.0 / __dsqrt_rn(sum) : 0.0;
    if (!(sum > 0.0)) atomicAdd((unsigned long long*)(status + 0), 1ull);
    if (p1 - p0 > SP_CHUNK) {                                   // the list's order is the race's; no result depends on it
        const unsigned long long at = atomicAdd((unsigned long long*)(status + 4), 1ull);
        heavy[at] = (int32_t)row;                               // at < N: a row is listed once
    }
}

// The chain of one chunk [p0, p1) of row `row` for block column t of a group of W lanes: the lanes load W entries at once
// and hand them round, every lane then walks them in CSR order.  The diagonal and an index outside [0, N) add nothing.
template <int W>
__device__ __forceinline__ double chunk_chain(const int64_t* __restrict__ indices, const double* __restrict__ data,
                                              const double* __restrict__ s, const double* __restrict__ Y1, long ld, long N, long row,
                                              long p0, long p1, int t, int l) {
    constexpr int U = W < 8 ? W : 8;                             // gathers in flight per lane
    const int tt = t < l ? t : l - 1;                             // a lane past the block loads a column that exists; its sum is dropped
    double acc = 0.0;
    for (long q = p0; q < p1; q += W) {
        const long p = q + t;
        long j = -1;
        double w = 0.0;
        if (p < p1) {
            j = indices[p];
            if (j == row || j < 0 || j >= N) j = -1;
            else w = data[p] * s[j];
        }
        const int n = (int)((p1 - q) < (long)W ? (p1 - q) : (long)W);
        for (int e0 = 0; e0 < n; e0 += U) {
            // the U loads are issued before the first of them is needed; a skipped entry loads the row's own block row and
            // adds nothing; the chain itself stays in CSR order
            long je[U];
            double we[U], y[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                je[u] = __shfl(j, e0 + u, W);
                we[u] = __shfl(w, e0 + u, W);
                if (e0 + u >= n) je[u] = -1;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) y[u] = Y1[(je[u] >= 0 ? je[u] : row) * ld + tt];
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (je[u] >= 0) acc = fma(we[u], y[u], acc);
        }
    }
    return acc;
}

__device__ __forceinline__ void spmm_store(double total, long row, int t, const double* __restrict__ s, const double* __restrict__ Y1,
                                           const double* __restrict__ Y0, double* __restrict__ Yout, long ld, double alpha, double c,
                                           double beta) {
    const double m = s[row] * total;
    double r = alpha * fma(-c, Y1[row * ld + t], m);
    if (Y0) r = fma(-beta, Y0[row * ld + t], r);
    Yout[row * ld + t] = r;
}

// 256 / W rows per workgroup, one group of W lanes per row.  With a list of long rows those are left to spmm_heavy_kernel.
template <int W>
__global__ __launch_bounds__(SP_THREADS) void spmm_kernel(const int64_t* __restrict__ indptr, const int64_t* __restrict__ indices,
                                                          const double* __restrict__ data, const double* __restrict__ s, long N, long nnz,
                                                          int skip_long, const double* __restrict__ Y1, const double* __restrict__ Y0,
                                                          double* __restrict__ Yout, long ld, int l, double alpha, double c, double beta) {
    const int t = threadIdx.x % W;
    const long row = (long)blockIdx.x * (SP_THREADS / W) + threadIdx.x / W;
    if (row >= N) return;                                        // a whole group leaves together
    long p0, p1;
    row_range(indptr, row, nnz, p0, p1);
    if (skip_long && p1 - p0 > SP_CHUNK) return;
    double total = 0.0;
    for (long q = p0; q < p1; q += SP_CHUNK) {
        const long q1 = q + SP_CHUNK < p1 ? q + SP_CHUNK : p1;
        const double part = chunk_chain<W>(indices, data, s, Y1, ld, N, row, q, q1, t, l);
        total = q == p0 ? part : total + part;
    }
    if (t < l) spmm_store(total, row, t, s, Y1, Y0, Yout, ld, alpha, c, beta);
}

// One workgroup per listed row: eight groups of 32 lanes take eight consecutive chunks at a time, group 0 adds their sums
// in chunk order.
__global__ __launch_bounds__(SP_THREADS) void spmm_heavy_kernel(const int64_t* __restrict__ indptr, const int64_t* __restrict__ indices,
                                                                const double* __restrict__ data, const double* __restrict__ s, long N,
                                                                long nnz, const int32_t* __restrict__ heavy, const double* __restrict__ Y1,
                                                                const double* __restrict__ Y0, double* __restrict__ Yout, long ld, int l,
                                                                double alpha, double c, double beta) {
    constexpr int G = SP_THREADS / 32;
    __shared__ double part[G][32];
    const int t = threadIdx.x & 31, g = threadIdx.x >> 5;
    const long row = heavy[blockIdx.x];
    if (row < 0 || row >= N) return;
    long p0, p1;
    row_range(indptr, row, nnz, p0, p1);
    if (p1 - p0 <= SP_CHUNK) return;                             // spmm_kernel wrote it
    const long chunks = (p1 - p0 + SP_CHUNK - 1) / SP_CHUNK;
    double total = 0.0;
    for (long k0 = 0; k0 < chunks; k0 += G) {
        const long k = k0 + g;
        if (k < chunks) {
            const long q = p0 + k * SP_CHUNK, q1 = q + SP_CHUNK < p1 ? q + SP_CHUNK : p1;
            part[g][t] = chunk_chain<32>(indices, data, s, Y1, ld, N, row, q, q1, t, l);
        }
        __syncthreads();
        if (g == 0) {
            const int n = (int)(chunks - k0 < G ? chunks - k0 : G);
            for (int e = 0; e < n; ++e) total = (k0 + e == 0) ? part[e][t] : total + part[e][t];
        }
        __syncthreads();
    }
    if (g == 0 && t < l) spmm_store(total, row, t, s, Y1, Y0, Yout, ld, alpha, c, beta);
}

// ---- Gram matrices: slab b holds rows [b per, (b + 1) per); entry (a, c) of a slab is one chain over its rows.
__global__ __launch_bounds__(SP_THREADS) void gram_slab_kernel(const double* __restrict__ V, const double* __restrict__ Wm, long ld, long N,
                                                               int l, long per, double* __restrict__ parts) {
    __shared__ double sv[SP_TILE][SP_MAX_L];
    __shared__ double sw[SP_TILE][SP_MAX_L];
    const int tid = threadIdx.x, ll = l * l;
    const long r0 = (long)blockIdx.x * per, r1 = r0 + per < N ? r0 + per : N;
    double g[4] = {0.0, 0.0, 0.0, 0.0}, h[4] = {0.0, 0.0, 0.0, 0.0};
    for (long base = r0; base < r1; base += SP_TILE) {
        const int rows = (int)(r1 - base < SP_TILE ? r1 - base : SP_TILE);
        for (int e = tid; e < rows * l; e += SP_THREADS) {
            const int r = e / l, col = e - r * l;
            sv[r][col] = V[(base + r) * ld + col];
            if (Wm) sw[r][col] = Wm[(base + r) * ld + col];
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = tid + u * SP_THREADS;
            if (e < ll) {
                const int a = e / l, b = e - a * l;
                for (int r = 0; r < rows; ++r) {
                    g[u] = fma(sv[r][a], sv[r][b], g[u]);
                    if (Wm) h[u] = fma(sv[r][a], sw[r][b], h[u]);
                }
            }
        }
        __syncthreads();
    }
    double* out = parts + (size_t)blockIdx.x * 2 * ll;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int e = tid + u * SP_THREADS;
        if (e < ll) {
            out[e] = g[u];
            out[ll + e] = h[u];
        }
    }
}

// out[e] = parts[0][e] + parts[1][e] + ... in slab order; `width` values per slab at stride `pitch`.
__global__ __launch_bounds__(SP_THREADS) void slab_sum_kernel(const double* __restrict__ parts, int slabs, int pitch, int offset, int width,
                                                              double* __restrict__ out) {
    const int e = blockIdx.x * SP_THREADS + threadIdx.x;
    if (e >= width) return;
    double acc = parts[offset + e];
    for (int b = 1; b < slabs; ++b) acc += parts[(size_t)b * pitch + offset + e];
    out[e] = acc;
}

// ---- residuals: thread (r, c) walks rows r, r + 8, ... of the slab for column c; the eight sums are added in r order.
__global__ __launch_bounds__(SP_THREADS) void residual_slab_kernel(const double* __restrict__ V, const double* __restrict__ Wm, long ld, long N,
                                                                   int l, const double* __restrict__ theta, long per,
                                                                   double* __restrict__ parts) {
    constexpr int G = SP_THREADS / 32;
    __shared__ double sh[G][32];
    const int c = threadIdx.x & 31, r = threadIdx.x >> 5;
    const long r0 = (long)blockIdx.x * per, r1 = r0 + per < N ? r0 + per : N;
    double acc = 0.0;
    if (c < l) {
        const double th = theta[c];
        for (long i = r0 + r; i < r1; i += G) {
            const double e = fma(-th, V[i * ld + c], Wm[i * ld + c]);
            acc = fma(e, e, acc);
        }
    }
    sh[r][c] = acc;
    __syncthreads();
    if (r == 0 && c < l) {
        double sum = sh[0][c];
        for (int k = 1; k < G; ++k) sum += sh[k][c];
        parts[(size_t)blockIdx.x * l + c] = sum;
    }
}

// ---- Vout = V T: T in LDS, thread (r, c) one element of 8 rows at a time, the chain over k in index order.
__global__ __launch_bounds__(SP_THREADS) void rotate_kernel(const double* __restrict__ V, long ldv, long N, int l, const double* __restrict__ T,
                                                            int l_out, double* __restrict__ Vout, long ldo) {
    constexpr int G = SP_THREADS / 32, ROWS = 64;
    __shared__ double st[SP_MAX_L][SP_MAX_L];
    for (int e = threadIdx.x; e < l * l_out; e += SP_THREADS) st[e / l_out][e % l_out] = T[e];
    __syncthreads();
    const int c = threadIdx.x & 31, r = threadIdx.x >> 5;
    if (c >= l_out) return;
    const long r0 = (long)blockIdx.x * ROWS, r1 = r0 + ROWS < N ? r0 + ROWS : N;
    for (long i = r0 + r; i < r1; i += G) {
        double acc = 0.0;
        for (int k = 0; k < l; ++k) acc = fma(V[i * ldv + k], st[k][c], acc);
        Vout[i * ldo + c] = acc;
    }
}

// ---- the embedding: one workgroup per output column.  The sign is that of the entry of largest |s_i v_i|, the smaller
// row on a tie (numpy's argmax in sklearn's _deterministic_vector_sign_flip); a NaN never wins.
__global__ __launch_bounds__(SP_THREADS) void embed_kernel(const double* __restrict__ V, long ldv, const double* __restrict__ s, long N,
                                                           int first, float* __restrict__ E, long lde, double* __restrict__ sign) {
    __shared__ double smag[SP_THREADS];
    __shared__ long srow[SP_THREADS];
    const int j = blockIdx.x, tid = threadIdx.x;
    const double* col = V + first + j;
    double best = -1.0;
    long at = N;
    for (long i = tid; i < N; i += SP_THREADS) {
        const double m = fabs(s[i] * col[i * ldv]);
        if (m > best) { best = m; at = i; }                       // rows ascend: the first of equal entries stays
    }
    smag[tid] = best;
    srow[tid] = at;
    __syncthreads();
    for (int w = SP_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) {
            const double m = smag[tid + w];
            const long i = srow[tid + w];
            if (m > smag[tid] || (m == smag[tid] && i < srow[tid])) { smag[tid] = m; srow[tid] = i; }
        }
        __syncthreads();
    }
    const long top = srow[0];
    const double sg = (top < N && s[top] * col[top * ldv] < 0.0) ? -1.0 : 1.0;
    if (tid == 0) sign[j] = sg;
    for (long i = tid; i < N; i += SP_THREADS) E[i * lde + j] = (float)(sg * (s[i] * col[i * ldv]));
}

inline long slab_rows(long N, int slabs) { return even_split(N, slabs, 64).per; }
inline int slab_count(long N, int slabs) { return even_split(N, slabs, 64).count; }

// [a, a + na) and [b, b + nb) in bytes
inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + nb && y < x + na;
}
inline size_t block_bytes(long N, long ld, int l) { return ((size_t)(N - 1) * ld + l) * sizeof(double); }

int block_shape(const char* who, long N, long ld, int l) {
    VSOM_REQUIRE(N >= 1 && l >= 1 && ld >= l, VSOM_EINVAL, "%s: N = %ld, l = %d, ld = %ld (wants N >= 1, 1 <= l <= ld)", who, N, l, ld);
    VSOM_REQUIRE(N <= SP_MAX_N && l <= SP_MAX_L, VSOM_EUNSUPPORTED, "%s: N = %ld, l = %d (N <= %ld, l <= %d)", who, N, l, SP_MAX_N,
                 SP_MAX_L);
    return VSOM_OK;
}

int slab_workspace(const char* who, long N, int l, int slabs, const void* ws, long ws_size) {
    VSOM_REQUIRE(slabs >= 1 && slabs <= SP_MAX_SLABS, VSOM_EINVAL, "%s: slabs = %d (1 .. %d)", who, slabs, SP_MAX_SLABS);
    const long need = vsom_spectral_ws_size(N, l, slabs);
    VSOM_REQUIRE(ws != nullptr && ws_size >= need, VSOM_EWORKSPACE, "%s: workspace too small or null (%ld < %ld bytes)", who,
                 ws ? ws_size : 0L, need);
    VSOM_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 8 == 0, VSOM_EALIGN, "%s: workspace must be 8-byte aligned", who);
    return VSOM_OK;
}

}  // namespace
}  // namespace vsom

using namespace vsom;

extern "C" {

int vsom_spectral_degrees(const int64_t* indptr, const int64_t* indices, const double* data, long N, long nnz, double* d, double* s,
                          int32_t* heavy, int64_t* status, vsom_stream_t stream) {
    VSOM_REQUIRE(indptr && d && s && heavy && status, VSOM_EINVAL, "vsom_spectral_degrees: null pointer");
    VSOM_REQUIRE(N >= 1 && nnz >= 0, VSOM_EINVAL, "vsom_spectral_degrees: N = %ld, nnz = %ld", N, nnz);
    VSOM_REQUIRE(nnz == 0 || (indices && data), VSOM_EINVAL, "vsom_spectral_degrees: null indices or data with nnz = %ld", nnz);
    VSOM_REQUIRE(N <= SP_MAX_N, VSOM_EUNSUPPORTED, "vsom_spectral_degrees: N = %ld > %ld", N, SP_MAX_N);
    VSOM_LAUNCH(spectral_clear_kernel, dim3(1), dim3(64), 0, stream, status);
    VSOM_LAUNCH(spectral_degrees_kernel, dim3(cdiv(N, SP_THREADS)), dim3(SP_THREADS), 0, stream, indptr, indices, data, N, nnz, d, s,
                heavy, status);
    return launch_status("spectral_degrees_kernel");
}

int vsom_spectral_spmm(const int64_t* indptr, const int64_t* indices, const double* data, const double* s, long N, long nnz,
                       const int32_t* heavy, int n_heavy, const double* Y1, const double* Y0, double* Yout, long ld, int l,
                       double alpha, double c, double beta, vsom_stream_t stream) {
    VSOM_REQUIRE(indptr && s && Y1 && Yout, VSOM_EINVAL, "vsom_spectral_spmm: null pointer");
    VSOM_REQUIRE(nnz >= 0 && (nnz == 0 || (indices && data)), VSOM_EINVAL, "vsom_spectral_spmm: nnz = %ld, or null indices / data", nnz);
    if (int rc = block_shape("vsom_spectral_spmm", N, ld, l)) return rc;
    VSOM_REQUIRE(n_heavy >= 0 && n_heavy <= N && (n_heavy == 0 || heavy), VSOM_EINVAL, "vsom_spectral_spmm: n_heavy = %d (0 .. N, with a list)",
                 n_heavy);
    const size_t bytes = block_bytes(N, ld, l);
    VSOM_REQUIRE(!overlap(Yout, bytes, Y1, bytes) && !(Y0 && overlap(Yout, bytes, Y0, bytes)), VSOM_EINVAL,
                 "vsom_spectral_spmm: Yout overlaps an input block");
    const int skip = heavy != nullptr;
#define SPMM(W)                                                                                                                  \
    VSOM_LAUNCH(spmm_kernel<W>, dim3(cdiv(N, SP_THREADS / W)), dim3(SP_THREADS), 0, stream, indptr, indices, data, s, N, nnz, skip, Y1, Y0, \
                Yout, ld, l, alpha, c, beta)
    if (l == 1) SPMM(1);
    else if (l == 2) SPMM(2);
    else if (l <= 4) SPMM(4);
    else if (l <= 8) SPMM(8);
    else if (l <= 16) SPMM(16);
    else SPMM(32);
#undef SPMM
    if (int rc = launch_status("spmm_kernel")) return rc;
    if (n_heavy > 0) {
        VSOM_LAUNCH(spmm_heavy_kernel, dim3(n_heavy), dim3(SP_THREADS), 0, stream, indptr, indices, data, s, N, nnz, heavy, Y1, Y0, Yout, ld,
                    l, alpha, c, beta);
        return launch_status("spmm_heavy_kernel");
    }
    return VSOM_OK;
}

long vsom_spectral_ws_size(long N, int l, int slabs) {
    if (N < 1 || N > SP_MAX_N || l < 1 || l > SP_MAX_L || slabs < 1 || slabs > SP_MAX_SLABS) return 0;
    return (long)slab_count(N, slabs) * 2 * l * l * (long)sizeof(double);
}

int vsom_spectral_gram(const double* V, const double* W, long ld, long N, int l, int slabs, double* G, double* H, void* ws, long ws_size,
                       vsom_stream_t stream) {
    VSOM_REQUIRE(V && G && ((W == nullptr) == (H == nullptr)), VSOM_EINVAL, "vsom_spectral_gram: null pointer, or W without H");
    if (int rc = block_shape("vsom_spectral_gram", N, ld, l)) return rc;
    if (int rc = slab_workspace("vsom_spectral_gram", N, l, slabs, ws, ws_size)) return rc;
    const int count = slab_count(N, slabs), ll = l * l;
    double* parts = static_cast<double*>(ws);
    VSOM_LAUNCH(gram_slab_kernel, dim3(count), dim3(SP_THREADS), 0, stream, V, W, ld, N, l, slab_rows(N, slabs), parts);
    VSOM_LAUNCH(slab_sum_kernel, dim3(cdiv(ll, SP_THREADS)), dim3(SP_THREADS), 0, stream, (const double*)parts, count, 2 * ll, 0, ll, G);
    if (H) VSOM_LAUNCH(slab_sum_kernel, dim3(cdiv(ll, SP_THREADS)), dim3(SP_THREADS), 0, stream, (const double*)parts, count, 2 * ll, ll, ll, H);
    return launch_status("spectral gram kernels");
}

int vsom_spectral_rotate(const double* V, long ldv, long N, int l, const double* T, int l_out, double* Vout, long ldo, vsom_stream_t stream) {
    VSOM_REQUIRE(V && T && Vout, VSOM_EINVAL, "vsom_spectral_rotate: null pointer");
    if (int rc = block_shape("vsom_spectral_rotate", N, ldv, l)) return rc;
    if (int rc = block_shape("vsom_spectral_rotate", N, ldo, l_out)) return rc;
    VSOM_REQUIRE(!overlap(Vout, block_bytes(N, ldo, l_out), V, block_bytes(N, ldv, l)), VSOM_EINVAL, "vsom_spectral_rotate: Vout overlaps V");
    VSOM_LAUNCH(rotate_kernel, dim3(cdiv(N, 64)), dim3(SP_THREADS), 0, stream, V, ldv, N, l, T, l_out, Vout, ldo);
    return launch_status("rotate_kernel");
}

int vsom_spectral_residual(const double* V, const double* W, long ld, long N, int l, const double* theta, int slabs, double* out, void* ws,
                           long ws_size, vsom_stream_t stream) {
    VSOM_REQUIRE(V && W && theta && out, VSOM_EINVAL, "vsom_spectral_residual: null pointer");
    if (int rc = block_shape("vsom_spectral_residual", N, ld, l)) return rc;
    if (int rc = slab_workspace("vsom_spectral_residual", N, l, slabs, ws, ws_size)) return rc;
    const int count = slab_count(N, slabs);
    double* parts = static_cast<double*>(ws);
    VSOM_LAUNCH(residual_slab_kernel, dim3(count), dim3(SP_THREADS), 0, stream, V, W, ld, N, l, theta, slab_rows(N, slabs), parts);
    VSOM_LAUNCH(slab_sum_kernel, dim3(1), dim3(SP_THREADS), 0, stream, (const double*)parts, count, l, 0, l, out);
    return launch_status("spectral residual kernels");
}

int vsom_spectral_embed(const double* V, long ldv, const double* s, long N, int first, int n_out, float* E, long lde, double* sign,
                        vsom_stream_t stream) {
    VSOM_REQUIRE(V && s && E && sign, VSOM_EINVAL, "vsom_spectral_embed: null pointer");
    VSOM_REQUIRE(N >= 1 && first >= 0 && n_out >= 1 && ldv >= first + n_out && lde >= n_out, VSOM_EINVAL,
                 "vsom_spectral_embed: N = %ld, first = %d, n_out = %d, ldv = %ld, lde = %ld", N, first, n_out, ldv, lde);
    VSOM_REQUIRE(N <= SP_MAX_N && first + n_out <= SP_MAX_L, VSOM_EUNSUPPORTED, "vsom_spectral_embed: N = %ld, first + n_out = %d (N <= %ld, <= %d)",
                 N, first + n_out, SP_MAX_N, SP_MAX_L);
    VSOM_LAUNCH(embed_kernel, dim3(n_out), dim3(SP_THREADS), 0, stream, V, ldv, s, N, first, E, lde, sign);
    return launch_status("embed_kernel");
}

}  // extern "C"
