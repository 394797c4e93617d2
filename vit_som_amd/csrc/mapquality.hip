// Map quality (no counterpart in the reference's tools/evaluation.py): the fold over what the BMU pass leaves behind --
// quantization error, topographic error, hit map, nearest sample per unit (vsom_map_stats) -- and the prototype-to-prototype
// pass of the U-matrix (vsom_umatrix).  Every accumulation is an integer or a fixed-order fp64 sum: bitwise reproducible.
#include "common.h"

namespace vsom {

constexpr int MQ_ROWS = 8;        // rows of dist per workgroup (two per wave)
constexpr int MQ_NBR = 8;         // neighbour slots per unit

// (value, index) lexicographic minimum over the wave; every lane ends with the result.
__device__ __forceinline__ void wave_argmin(float& v, int& i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
}

// One workgroup folds MQ_ROWS rows.  Pass 1, one wave per row: NaN scan and the argmin over k != bmu, then the row's three
// integer atomics.  Pass 2, one thread per column (four with VEC): the minimum of the packed (key, ordinal) words over the
// workgroup's valid rows in a register -- the rows are still in cache -- and ONE 64-bit atomic min per column.
template <bool VEC>
__global__ __launch_bounds__(256) void map_stats_kernel(const float* __restrict__ dist, const int64_t* __restrict__ bmu, long B, int K,
                                                        const float* __restrict__ pos, float adj_r2, long first,
                                                        unsigned long long* __restrict__ hits, unsigned long long* __restrict__ qe_fix,
                                                        unsigned long long* __restrict__ te, unsigned long long* __restrict__ nearest,
                                                        int* __restrict__ bad, int64_t* __restrict__ second) {
    __shared__ int valid[MQ_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long row0 = (long)blockIdx.x * MQ_ROWS;

    for (int r = wave; r < MQ_ROWS; r += 4) {
        const long i = row0 + r;
        if (i >= B) {                                      // wave-uniform
            if (lane == 0) valid[r] = 0;
            continue;
        }
        const int64_t b64 = bmu[i];
        const bool in_range = b64 >= 0 && b64 < K;
        const int b = in_range ? (int)b64 : -1;
        const float* row = dist + i * K;
        float best = INFINITY;
        int arg = 0x7fffffff;
        bool nan = false;
        auto see = [&](float v, int k) {
            nan |= v != v;
            if (k != b && (v < best || (v == best && k < arg))) { best = v; arg = k; }
        };
        if (VEC) {
            for (int k = lane * 4; k < K; k += 256) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(row + k);
                see(v.x, k); see(v.y, k + 1); see(v.z, k + 2); see(v.w, k + 3);
            }
        } else {
            for (int k = lane; k < K; k += 64) see(row[k], k);
        }
        wave_argmin(best, arg);
        nan = __any(nan);
        const float db = in_range ? row[b] : 0.f;
        if (arg == 0x7fffffff) arg = b == 0 ? 1 : 0;      // only a row of NaNs leaves none: the row is skipped below
        const bool ok = in_range && !nan && fabsf(db) < 2147483648.f;
        if (lane == 0) {
            valid[r] = ok;
            if (!ok) {
                atomicAdd(bad, 1);
            } else {
                const double dx = (double)pos[2 * b] - (double)pos[2 * arg], dy = (double)pos[2 * b + 1] - (double)pos[2 * arg + 1];
                atomicAdd(hits + b, 1ull);
                atomicAdd(qe_fix + b, (unsigned long long)llrint((double)db * 4294967296.0));
                if (dx * dx + dy * dy > (double)adj_r2) atomicAdd(te, 1ull);
                if (second) second[i] = arg;
            }
        }
    }
    __syncthreads();

    auto fold = [&](unsigned long long& m, float v, int r) {
        const unsigned long long w = ((unsigned long long)ordered_key(v) << 32) | (unsigned long long)(first + row0 + r);
        m = w < m ? w : m;
    };
    if (VEC) {
        for (int k = tid * 4; k < K; k += 1024) {
            unsigned long long m0 = ~0ull, m1 = ~0ull, m2 = ~0ull, m3 = ~0ull;
#pragma unroll
            for (int r = 0; r < MQ_ROWS; ++r) {
                if (!valid[r]) continue;                   // workgroup-uniform
                const f32x4 v = *reinterpret_cast<const f32x4*>(dist + (row0 + r) * K + k);
                fold(m0, v.x, r); fold(m1, v.y, r); fold(m2, v.z, r); fold(m3, v.w, r);
            }
            if (m0 != ~0ull) {                             // some row was valid: all four columns hold a word
                atomicMin(nearest + k, m0); atomicMin(nearest + k + 1, m1);
                atomicMin(nearest + k + 2, m2); atomicMin(nearest + k + 3, m3);
            }
        }
    } else {
        for (int k = tid; k < K; k += 256) {
            unsigned long long m = ~0ull;
#pragma unroll
            for (int r = 0; r < MQ_ROWS; ++r) {
                if (!valid[r]) continue;
                fold(m, dist[(row0 + r) * K + k], r);
            }
            if (m != ~0ull) atomicMin(nearest + k, m);
        }
    }
}

// One workgroup per unit.  Wave 0 lists the unit's grid neighbours in ascending index order (ballot + prefix count); then the
// unit's row and the neighbours' rows are streamed once, every thread keeping fp64 partial sums per neighbour (exact fp64
// products / differences of the fp32 values); a butterfly per wave and the four waves in order give the row sums.
template <int DISTANCE, bool VEC>
__global__ __launch_bounds__(256) void umatrix_kernel(const float* __restrict__ W, int K, int L, const float* __restrict__ pos,
                                                      float adj_r2, int* __restrict__ nbr_idx, float* __restrict__ nbr_dist,
                                                      float* __restrict__ u, int* __restrict__ status) {
    constexpr int NACC = DISTANCE == VSOM_DIST_COSINE ? 2 * MQ_NBR + 1 : MQ_NBR;
    __shared__ int nbr[MQ_NBR];
    __shared__ int n_nbr;
    __shared__ double part[4][NACC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = blockIdx.x;

    if (wave == 0) {
        const double px = pos[2 * k], py = pos[2 * k + 1];
        int cnt = 0;
        for (int j0 = 0; j0 < K; j0 += 64) {               // wave-uniform trip count
            const int j = j0 + lane;
            bool near = false;
            if (j < K && j != k) {
                const double dx = (double)pos[2 * j] - px, dy = (double)pos[2 * j + 1] - py;
                near = dx * dx + dy * dy <= (double)adj_r2;
            }
            const unsigned long long mask = __ballot(near);
            const int slot = cnt + __popcll(mask & ((1ull << lane) - 1ull));
            if (near && slot < MQ_NBR) nbr[slot] = j;
            cnt += __popcll(mask);
        }
        if (lane == 0) {
            if (cnt > MQ_NBR) { atomicMax(status, cnt); cnt = MQ_NBR; }
            n_nbr = cnt;
        }
    }
    __syncthreads();
    const int cnt = n_nbr;
    int nb[MQ_NBR];
#pragma unroll
    for (int n = 0; n < MQ_NBR; ++n) nb[n] = n < cnt ? nbr[n] : k;

    double acc[NACC];
#pragma unroll
    for (int n = 0; n < NACC; ++n) acc[n] = 0.0;
    const float* wk = W + (long)k * L;
    auto term = [&](int n, float a, float b) {
        const double da = a, db = b;
        if (DISTANCE == VSOM_DIST_COSINE) {
            acc[n] += da * db;
            acc[MQ_NBR + n] += db * db;
        } else if (DISTANCE == VSOM_DIST_EUCLIDEAN) {
            const double d = da - db;
            acc[n] += d * d;
        } else {
            acc[n] += fabs(da - db);
        }
    };
    if (VEC) {
        for (int e = tid * 4; e < L; e += 1024) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(wk + e);
            if (DISTANCE == VSOM_DIST_COSINE)
                acc[2 * MQ_NBR] += (double)a.x * a.x + (double)a.y * a.y + (double)a.z * a.z + (double)a.w * a.w;
#pragma unroll
            for (int n = 0; n < MQ_NBR; ++n) {
                if (n < cnt) {                             // workgroup-uniform
                    const f32x4 b = *reinterpret_cast<const f32x4*>(W + (long)nb[n] * L + e);
                    term(n, a.x, b.x); term(n, a.y, b.y); term(n, a.z, b.z); term(n, a.w, b.w);
                }
            }
        }
    } else {
        for (int e = tid; e < L; e += 256) {
            const float a = wk[e];
            if (DISTANCE == VSOM_DIST_COSINE) acc[2 * MQ_NBR] += (double)a * a;
#pragma unroll
            for (int n = 0; n < MQ_NBR; ++n)
                if (n < cnt) term(n, a, W[(long)nb[n] * L + e]);
        }
    }
#pragma unroll
    for (int n = 0; n < NACC; ++n) {
        const double s = wave_sum_f64(acc[n]);
        if (lane == 0) part[wave][n] = s;
    }
    __syncthreads();
    if (tid < MQ_NBR) {
        const int n = tid;
        float d = 0.f;
        if (n < cnt) {
            const double s = ((part[0][n] + part[1][n]) + part[2][n]) + part[3][n];
            if (DISTANCE == VSOM_DIST_COSINE) {
                const double na = ((part[0][2 * MQ_NBR] + part[1][2 * MQ_NBR]) + part[2][2 * MQ_NBR]) + part[3][2 * MQ_NBR];
                const double nn = ((part[0][MQ_NBR + n] + part[1][MQ_NBR + n]) + part[2][MQ_NBR + n]) + part[3][MQ_NBR + n];
                // |a| |b| as sqrt(|a|^2 |b|^2): for identical rows the quotient is then exactly 1.  Either norm below the
                // layer's epsilon: the clamped product, as F.normalize forms it.
                const double den = (na >= 1e-24 && nn >= 1e-24) ? sqrt(na * nn) : fmax(sqrt(na), 1e-12) * fmax(sqrt(nn), 1e-12);
                d = (float)(1.0 - s / den);
            } else if (DISTANCE == VSOM_DIST_EUCLIDEAN) {
                d = (float)sqrt(s);
            } else {
                d = (float)s;
            }
        }
        nbr_idx[(long)k * MQ_NBR + n] = n < cnt ? nbr[n] : -1;
        nbr_dist[(long)k * MQ_NBR + n] = d;
        // the mean over the valid slots, summed in slot order in fp64 (lanes 0..7 of wave 0 hold the slots)
        double sum = 0.0;
#pragma unroll
        for (int m = 0; m < MQ_NBR; ++m) {
            const float dm = __shfl(d, m, 64);
            if (m < cnt) sum += (double)dm;
        }
        if (n == 0) u[k] = cnt > 0 ? (float)(sum / cnt) : 0.f;
    }
}

}  // namespace vsom

extern "C" {

int vsom_map_stats(const float* dist, const int64_t* bmu, long B, int K, const float* grid_positions, float adj_r2,
                   long first_ordinal, long long* hits, long long* qe_fix, long long* te, unsigned long long* nearest, int* bad,
                   int64_t* second, vsom_stream_t stream) {
    VSOM_REQUIRE(dist && bmu && grid_positions && hits && qe_fix && te && nearest && bad, VSOM_EINVAL, "map_stats: null pointer");
    VSOM_REQUIRE(B >= 0 && first_ordinal >= 0 && adj_r2 >= 0.f, VSOM_EINVAL, "map_stats: bad sizes (B=%ld first_ordinal=%ld)", B,
                 first_ordinal);
    VSOM_REQUIRE(K >= 2, VSOM_EINVAL, "map_stats: a map of K=%d units has no second-best unit", K);
    VSOM_REQUIRE(first_ordinal + B < (1L << 31), VSOM_EUNSUPPORTED, "map_stats: sample ordinals must stay below 2^31");
    if (B == 0) return VSOM_OK;
    const dim3 grid(vsom::cdiv(B, vsom::MQ_ROWS));
    auto* h = reinterpret_cast<unsigned long long*>(hits);
    auto* q = reinterpret_cast<unsigned long long*>(qe_fix);
    auto* t = reinterpret_cast<unsigned long long*>(te);
    if (K % 4 == 0 && vsom::aligned16(dist)) {
        VSOM_LAUNCH(vsom::map_stats_kernel<true>, grid, dim3(256), 0, stream, dist, bmu, B, K, grid_positions, adj_r2, first_ordinal, h,
                    q, t, nearest, bad, second);
    } else {
        VSOM_LAUNCH(vsom::map_stats_kernel<false>, grid, dim3(256), 0, stream, dist, bmu, B, K, grid_positions, adj_r2, first_ordinal, h,
                    q, t, nearest, bad, second);
    }
    return vsom::launch_status("map_stats_kernel");
}

int vsom_umatrix(const float* W, int K, int L, const float* grid_positions, float adj_r2, int distance, int* nbr_idx,
                 float* nbr_dist, float* u, int* status, vsom_stream_t stream) {
    VSOM_REQUIRE(W && grid_positions && nbr_idx && nbr_dist && u && status, VSOM_EINVAL, "umatrix: null pointer");
    VSOM_REQUIRE(K > 0 && L > 0 && adj_r2 >= 0.f, VSOM_EINVAL, "umatrix: bad sizes (K=%d L=%d)", K, L);
    VSOM_REQUIRE(distance == VSOM_DIST_COSINE || distance == VSOM_DIST_EUCLIDEAN || distance == VSOM_DIST_MANHATTAN, VSOM_EUNSUPPORTED,
                 "umatrix: unknown distance %d", distance);
    const bool vec = L % 4 == 0 && vsom::aligned16(W);
#define VSOM_UMATRIX(D, V) \
    VSOM_LAUNCH((vsom::umatrix_kernel<D, V>), dim3(K), dim3(256), 0, stream, W, K, L, grid_positions, adj_r2, nbr_idx, nbr_dist, u, status)
    if (distance == VSOM_DIST_COSINE) {
        if (vec) VSOM_UMATRIX(VSOM_DIST_COSINE, true); else VSOM_UMATRIX(VSOM_DIST_COSINE, false);
    } else if (distance == VSOM_DIST_EUCLIDEAN) {
        if (vec) VSOM_UMATRIX(VSOM_DIST_EUCLIDEAN, true); else VSOM_UMATRIX(VSOM_DIST_EUCLIDEAN, false);
    } else {
        if (vec) VSOM_UMATRIX(VSOM_DIST_MANHATTAN, true); else VSOM_UMATRIX(VSOM_DIST_MANHATTAN, false);
    }
#undef VSOM_UMATRIX
    return vsom::launch_status("umatrix_kernel");
}

}  // extern "C"
