// The linear probe (vit_som_amd/linear_probe.py; no counterpart in the reference): multinomial logistic regression fitted on
// the device by L-BFGS.  The two passes over X of an iteration are vsom_pca_project and vsom_pca_backproject, unchanged
// (pca.hip); this file holds everything else, none of which touches X:
//
//   vsom_probe_fold        B = A o invstd (fp64 -> f32, one rounding): the standardisation folded into the weights, and the
//                          three dot products W.W, W.A, A.A of the penalty along a search direction A
//   vsom_probe_residual    R = softmax(Z + b) - onehot(y) (fp64, rounded once), the summed cross-entropy, the column sums of R
//   vsom_probe_linesearch  the summed cross-entropy at Z + alpha_j Zp, alpha_j = alpha0 2^-j, for a whole ladder in one launch
//   vsom_probe_step        the Armijo choice from that ladder, then Z += alpha Zp, theta += alpha p, s = alpha p
//   vsom_probe_gradient    g = (Zt o invstd) / N + lam W, the intercept part, and y = g - g_prev
//   vsom_lbfgs_dots / _coeff / _combine   the library's L-BFGS pieces in dot-product-matrix form; they know nothing of the probe
//
// ROWS.  A logit row of C <= 256 values is held by L = min(64, 2^ceil(log2 C)) lanes, 64 / L rows to a wave, a lane holding
// the columns l, l + L, ... (at most four).  Row maximum, sum and argmax are xor butterflies inside the L lanes.
// ORDER.  No floating-point atomics.  A workgroup owns a run of rows (or of vector elements) that is a function of the shape
// alone; inside it every accumulator adds in ascending order, accumulators are added in slot / lane / wave order, and the
// per-workgroup partials are added in workgroup order by probe_reduce_kernel.  Every result is bitwise reproducible.
#include "common.h"

#include <math.h>

namespace vsom {
namespace {

constexpr int PROBE_MAX_C = 256;             // the contraction's widest basis (pca.hip)
constexpr int PROBE_MAX_STEPS = 16;          // ladder length
constexpr int PROBE_MAX_BLOCKS = 1024;
constexpr int LB_MAX_M = 16;
constexpr int LB_MAX_NV = 2 * LB_MAX_M + 3;
constexpr int LB_CHUNK = 1024;               // vector elements a workgroup takes at a time: 256 threads x 4
constexpr int LB_MAX_BLOCKS = 512;
constexpr int FOLD_MAX_BLOCKS = 512;
constexpr long PROBE_MAX_ROWS = 0x7fffffffL - 256;       // pca.hip's limit

// state record of the L-BFGS pieces: the first 16 doubles of `state`
enum { REC_ALPHA0 = 0, REC_GTP, REC_GG, REC_GMAX, REC_COUNT, REC_SKIPPED, REC_ACCEPTED, REC_SLOT, REC_HEAD,
       REC_STEP = 12, REC_LS_STATUS, REC_F, REC_J, REC_SIZE = 16 };

struct RowPlan { int L, slots, nblk; long rows_per; };
RowPlan row_plan(long N, int C) {
    RowPlan p;
    p.L = 2;
    while (p.L < C && p.L < 64) p.L <<= 1;
    p.slots = 256 / p.L;
    long nb = (N + 4L * p.slots - 1) / (4L * p.slots);          // four rows to a slot at least
    if (nb > PROBE_MAX_BLOCKS) nb = PROBE_MAX_BLOCKS;
    if (nb < 1) nb = 1;
    const Split rows = even_split(N, nb, p.slots);              // whole slots to a block
    p.rows_per = rows.per;
    p.nblk = rows.count;
    return p;
}

struct VecPlan { int nblk; long chunks_per; };
VecPlan vec_plan(long n, int max_blocks) {
    VecPlan p;
    long chunks = (n + LB_CHUNK - 1) / LB_CHUNK;
    if (chunks < 1) chunks = 1;                                 // an empty vector still gets its one block
    const Split s = even_split(chunks, chunks < max_blocks ? chunks : max_blocks);
    p.chunks_per = s.per;
    p.nblk = s.count;
    return p;
}

// a count or slot read from the caller's state record, forced into [lo, hi]: a state that was never zeroed indexes nothing
__device__ __forceinline__ int rec_int(double v, int lo, int hi) {
    return v >= (double)lo ? (v <= (double)hi ? (int)v : hi) : lo;          // a NaN gives lo
}
__device__ __forceinline__ double group_max(double v, int L) {
    for (int o = L >> 1; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double group_sum(double v, int L) {
    for (int o = L >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// out[i] = sum over the workgroups b ascending of part[b * width + i]; the last n_max entries take the maximum instead.
// Entries below n_a go to out_a, the others to out_b.
__global__ __launch_bounds__(256) void probe_reduce_kernel(const double* __restrict__ part, int nblk, int width, int n_max,
                                                           double* __restrict__ out_a, int n_a, double* __restrict__ out_b) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= width) return;
    double t = part[i];
    if (i >= width - n_max) {
        for (int b = 1; b < nblk; ++b) t = fmax(t, part[(long)b * width + i]);
    } else {
        for (int b = 1; b < nblk; ++b) t += part[(long)b * width + i];
    }
    if (i < n_a) out_a[i] = t;
    else out_b[i - n_a] = t;
}

// ---------------------------------------------------------------------------------------------- fold
// B[c][d] = (float)(A[c][d] * invstd[d]); with W: the workgroup's partial sums of W.W, W.A and A.A (fp64, its elements in
// ascending chunks, lanes by butterfly, waves in order).
__global__ __launch_bounds__(256) void probe_fold_kernel(const double* __restrict__ A, const double* __restrict__ invstd, long n, int D,
                                                         float* __restrict__ B, long ldb, const double* __restrict__ W,
                                                         long chunks_per, double* __restrict__ part) {
    __shared__ double sh[4][3];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double ww = 0.0, wa = 0.0, aa = 0.0;
    for (long ch = 0; ch < chunks_per; ++ch) {
        const long base = ((long)blockIdx.x * chunks_per + ch) * LB_CHUNK;
        if (base >= n) break;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long i = base + u * 256 + t;
            if (i < n) {
                const long c = i / D;
                const int d = (int)(i - c * D);
                const double a = A[i];
                B[c * ldb + d] = (float)(a * invstd[d]);
                if (W) {
                    const double w = W[i];
                    ww = fma(w, w, ww);
                    wa = fma(w, a, wa);
                    aa = fma(a, a, aa);
                }
            }
        }
    }
    if (!W) return;
    ww = wave_sum_f64(ww); wa = wave_sum_f64(wa); aa = wave_sum_f64(aa);
    if (lane == 0) { sh[wave][0] = ww; sh[wave][1] = wa; sh[wave][2] = aa; }
    __syncthreads();
    if (t < 3) part[(long)blockIdx.x * 3 + t] = ((sh[0][t] + sh[1][t]) + sh[2][t]) + sh[3][t];
}

// ---------------------------------------------------------------------------------------------- residual
__global__ __launch_bounds__(256) void probe_residual_kernel(const float* __restrict__ Z, long ldz, long N, int C, int L, long rows_per,
                                                             const double* __restrict__ b, const int64_t* __restrict__ y,
                                                             float* __restrict__ R, long ldr, int64_t* __restrict__ pred,
                                                             double* __restrict__ prob, int* __restrict__ status,
                                                             double* __restrict__ part) {
    __shared__ double sh[4 * (PROBE_MAX_C + 1)];         // slots x (C + 1) <= 4 x 257 (slots (L + 1) <= 384 below L = 64)
    const int t = threadIdx.x, slots = 256 / L, slot = t / L, l = t & (L - 1);
    const long r0 = (long)blockIdx.x * rows_per;
    double bias[4], acc_gb[4] = {0.0, 0.0, 0.0, 0.0}, acc_loss = 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e) bias[e] = (l + e * L < C && b) ? b[l + e * L] : 0.0;
    for (long it = 0; it < rows_per; it += slots) {
        const long row = r0 + it + slot;
        const bool in = row < N;
        const int64_t lab = in ? y[row] : -1;
        const bool ok = in && lab >= 0 && lab < C;       // a label outside [0, C) is counted and never used as an index
        if (in && !ok && l == 0) atomicAdd(status, 1);
        double z[4], zmax = -INFINITY;
        int arg = 0x7fffffff;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = l + e * L;
            z[e] = (in && c < C) ? (double)Z[row * ldz + c] + bias[e] : -INFINITY;
            if (z[e] > zmax) { zmax = z[e]; arg = c; }
        }
        // first index of the row maximum
        double best = zmax;
        for (int o = L >> 1; o > 0; o >>= 1) {
            const double ov = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(arg, o, 64);
            if (ov > best || (ov == best && oi < arg)) { best = ov; arg = oi; }
        }
        zmax = best;
        double ex[4], s = 0.0, zy = 0.0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = l + e * L;
            ex[e] = (in && c < C) ? exp(z[e] - zmax) : 0.0;
            s += ex[e];
            if (ok && c == (int)lab) zy = z[e];
        }
        s = group_sum(s, L);
        zy = group_sum(zy, L);                           // one lane holds the value, the others zero: exact
        if (ok && l == 0) acc_loss += (log(s) + zmax) - zy;
        if (in) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = l + e * L;
                if (c < C) {
                    const double pr = ex[e] / s;
                    const float rf = ok ? (float)(pr - (c == (int)lab ? 1.0 : 0.0)) : 0.f;
                    R[row * ldr + c] = rf;
                    acc_gb[e] += (double)rf;
                    if (prob) prob[row * C + c] = pr;
                }
            }
            if (pred && l == 0) pred[row] = arg;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (l + e * L < C) sh[slot * (C + 1) + l + e * L] = acc_gb[e];
    if (l == 0) sh[slot * (C + 1) + C] = acc_loss;
    __syncthreads();
    for (int i = t; i <= C; i += 256) {
        double v = sh[i];
        for (int s2 = 1; s2 < slots; ++s2) v += sh[s2 * (C + 1) + i];
        part[(long)blockIdx.x * (C + 1) + i] = v;
    }
}

// ---------------------------------------------------------------------------------------------- line search ladder
// part[b][j] = the workgroup's sum of CE(Z_i + a_j Zp_i + (b + a_j pb), y_i), a_j = alpha0 2^-j: each logit is
// fma(a_j, Zp, Z) + fma(a_j, pb, b) in fp64.  Rows with a label outside [0, C) contribute nothing.
__global__ __launch_bounds__(256) void probe_linesearch_kernel(const float* __restrict__ Z, const float* __restrict__ Zp, long ldz,
                                                               long N, int C, int L, long rows_per, const double* __restrict__ b,
                                                               const double* __restrict__ pb, const int64_t* __restrict__ y,
                                                               const double* __restrict__ alpha0, int nsteps,
                                                               double* __restrict__ part) {
    __shared__ double sh[128 * PROBE_MAX_STEPS];         // slots x 16, slots <= 128
    const int t = threadIdx.x, slots = 256 / L, slot = t / L, l = t & (L - 1);
    const long r0 = (long)blockIdx.x * rows_per;
    const double a0 = alpha0[0];
    double bias[4], pbias[4], acc[PROBE_MAX_STEPS];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        bias[e] = (l + e * L < C && b) ? b[l + e * L] : 0.0;
        pbias[e] = (l + e * L < C && pb) ? pb[l + e * L] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < PROBE_MAX_STEPS; ++j) acc[j] = 0.0;
    for (long it = 0; it < rows_per; it += slots) {
        const long row = r0 + it + slot;
        const bool in = row < N;
        const int64_t lab = in ? y[row] : -1;
        const bool ok = in && lab >= 0 && lab < C;
        double z0[4], zp[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = l + e * L;
            const bool have = in && c < C;
            z0[e] = have ? (double)Z[row * ldz + c] : 0.0;
            zp[e] = have ? (double)Zp[row * ldz + c] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < PROBE_MAX_STEPS; ++j) {
            if (j < nsteps) {
                const double a = ldexp(a0, -j);
                double z[4], zmax = -INFINITY, zy = 0.0, s = 0.0;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int c = l + e * L;
                    z[e] = (in && c < C) ? fma(a, zp[e], z0[e]) + fma(a, pbias[e], bias[e]) : -INFINITY;
                    zmax = fmax(zmax, z[e]);
                    if (ok && c == (int)lab) zy = z[e];
                }
                zmax = group_max(zmax, L);
#pragma unroll
                for (int e = 0; e < 4; ++e) s += (in && l + e * L < C) ? exp(z[e] - zmax) : 0.0;
                s = group_sum(s, L);
                zy = group_sum(zy, L);
                if (ok && l == 0) acc[j] += (log(s) + zmax) - zy;
            }
        }
    }
    if (l == 0) {
#pragma unroll
        for (int j = 0; j < PROBE_MAX_STEPS; ++j) sh[slot * PROBE_MAX_STEPS + j] = acc[j];
    }
    __syncthreads();
    if (t < nsteps) {
        double v = sh[t];
        for (int s2 = 1; s2 < slots; ++s2) v += sh[s2 * PROBE_MAX_STEPS + t];
        part[(long)blockIdx.x * nsteps + t] = v;
    }
}

// ---------------------------------------------------------------------------------------------- step
// Every workgroup makes the same choice from the same numbers (thread 0, plain fp64 without contraction), then applies it to
// its share of Z, theta and s.  F(a) = phi(a) / N + lam / 2 (W.W + 2 a W.P + a^2 P.P); the largest a_j with
// F(a_j) <= F(0) + c1 a_j g.p is taken.  No such step, or g.p >= 0: alpha = 0, nothing moves, rec says so.
__global__ __launch_bounds__(256) void probe_step_kernel(const double* __restrict__ phi, int nsteps, const double* __restrict__ alpha0,
                                                         const double* __restrict__ f0, const double* __restrict__ pen,
                                                         const double* __restrict__ gtp, double inv_n, double lam, double c1,
                                                         float* __restrict__ Z, const float* __restrict__ Zp, long ldz, long N,
                                                         int C, double* __restrict__ theta, const double* __restrict__ p,
                                                         double* __restrict__ s_new, long n, double* __restrict__ rec) {
    __shared__ double sh_alpha;
    if (threadIdx.x == 0) {
#pragma clang fp contract(off)
        const double a0 = alpha0[0], d = gtp[0];
        const double ww = pen[0], wp = pen[1], pp = pen[2];
        const double F0 = f0[0] * inv_n + 0.5 * lam * ww;
        double alpha = 0.0, Fa = F0;
        int jsel = -1, st = d < 0.0 ? 1 : 2;
        if (d < 0.0) {
            for (int j = 0; j < nsteps; ++j) {
                const double a = ldexp(a0, -j);
                const double F = phi[j] * inv_n + 0.5 * lam * (ww + 2.0 * a * wp + a * a * pp);
                if (F <= F0 + c1 * a * d) { alpha = a; Fa = F; jsel = j; st = 0; break; }
            }
        }
        sh_alpha = alpha;
        if (blockIdx.x == 0) {
            rec[REC_STEP] = alpha;
            rec[REC_LS_STATUS] = (double)st;
            rec[REC_F] = Fa;
            rec[REC_J] = (double)jsel;
        }
    }
    __syncthreads();
    const double alpha = sh_alpha;
    const long stride = (long)gridDim.x * 256, first = (long)blockIdx.x * 256 + threadIdx.x;
    for (long i = first; i < n; i += stride) {
        const double sv = alpha * p[i];
        s_new[i] = sv;
        if (alpha != 0.0) theta[i] = fma(alpha, p[i], theta[i]);
    }
    if (alpha == 0.0) return;
    const long total = N * C;
    for (long i = first; i < total; i += stride) {
        const long row = i / C;
        const long at = row * ldz + (i - row * C);
        Z[at] = (float)fma(alpha, (double)Zp[at], (double)Z[at]);
    }
}

// ---------------------------------------------------------------------------------------------- gradient
// g[c D + d] = Zt[c][d] invstd[d] inv_n + lam W[c][d];  g[C D + c] = gb[c] inv_n (absent without an intercept: n = C D);
// y_new = g - g_prev.
__global__ __launch_bounds__(256) void probe_gradient_kernel(const float* __restrict__ Zt, long ldz, const double* __restrict__ invstd,
                                                             const double* __restrict__ theta, const double* __restrict__ gb, int C,
                                                             int D, long n, double inv_n, double lam,
                                                             const double* __restrict__ g_prev, double* __restrict__ g,
                                                             double* __restrict__ y_new) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long nw = (long)C * D;
    double v;
    if (i < nw) {
        const long c = i / D;
        const int d = (int)(i - c * D);
        v = fma(lam, theta[i], ((double)Zt[c * ldz + d] * invstd[d]) * inv_n);
    } else {
        v = gb[i - nw] * inv_n;
    }
    g[i] = v;
    if (y_new) y_new[i] = v - g_prev[i];
}

// ---------------------------------------------------------------------------------------------- L-BFGS, dot-product-matrix form
// The vectors: S[0 .. m), Y[0 .. m) (ring slots, `count` of them held), g, and the new pair s_new, y_new -- NV = 2 m + 3 in
// this order.  part[b][k NV + v] = the workgroup's share of (s_new, y_new, g)[k] . vector v, part[b][3 NV] = its max |g|.
// One pass: a workgroup reads each element of each vector once.
__global__ __launch_bounds__(256) void lbfgs_dots_kernel(const double* __restrict__ S, const double* __restrict__ Y,
                                                         const double* __restrict__ g, const double* __restrict__ s_new,
                                                         const double* __restrict__ y_new, long n, int m, int has_new,
                                                         const double* __restrict__ state, long chunks_per,
                                                         double* __restrict__ part) {
    __shared__ double sh[4][3 * LB_MAX_NV + 1];
    const int NV = 2 * m + 3, W = 3 * NV + 1;
    const int count = has_new ? rec_int(state[REC_COUNT], 0, m) : 0;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int i = t; i < 4 * (3 * LB_MAX_NV + 1); i += 256) (&sh[0][0])[i] = 0.0;
    __syncthreads();
    double gmax = 0.0;
    for (long ch = 0; ch < chunks_per; ++ch) {
        const long base = ((long)blockIdx.x * chunks_per + ch) * LB_CHUNK;
        if (base >= n) break;
        double a[3][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long i = base + u * 256 + t;
            const bool ok = i < n;
            a[0][u] = (ok && has_new) ? s_new[i] : 0.0;
            a[1][u] = (ok && has_new) ? y_new[i] : 0.0;
            a[2][u] = ok ? g[i] : 0.0;
            gmax = fmax(gmax, fabs(a[2][u]));
        }
        for (int v = 0; v < NV; ++v) {
            const double* vec;
            if (v < m) vec = v < count ? S + (long)v * n : nullptr;
            else if (v < 2 * m) vec = v - m < count ? Y + (long)(v - m) * n : nullptr;
            else if (v == 2 * m) vec = g;
            else vec = has_new ? (v == 2 * m + 1 ? s_new : y_new) : nullptr;
            if (!vec) continue;
            double d0 = 0.0, d1 = 0.0, d2 = 0.0;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long i = base + u * 256 + t;
                const double x = i < n ? vec[i] : 0.0;
                d0 = fma(a[0][u], x, d0);
                d1 = fma(a[1][u], x, d1);
                d2 = fma(a[2][u], x, d2);
            }
            d0 = wave_sum_f64(d0); d1 = wave_sum_f64(d1); d2 = wave_sum_f64(d2);
            if (lane == 0) { sh[wave][v] += d0; sh[wave][NV + v] += d1; sh[wave][2 * NV + v] += d2; }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) gmax = fmax(gmax, __shfl_xor(gmax, o, 64));
    if (lane == 0) sh[wave][3 * NV] = gmax;
    __syncthreads();
    for (int i = t; i < W; i += 256) {
        const double v = i < 3 * NV ? ((sh[0][i] + sh[1][i]) + sh[2][i]) + sh[3][i]
                                    : fmax(fmax(sh[0][i], sh[1][i]), fmax(sh[2][i], sh[3][i]));
        part[(long)blockIdx.x * W + i] = v;
    }
}

// One thread: takes the new pair into the Gram matrix (or skips it when s.y <= 0), then runs the two-loop recursion on
// coefficients.  state = rec[16] | G[(2 m + 1)^2] | delta[2 m + 1]; Gram index: S slot i -> i, Y slot i -> m + i, g -> 2 m.
// The direction is p = sum_j delta[j] vector_j (vsom_lbfgs_combine).
__global__ void lbfgs_coeff_kernel(const double* __restrict__ dots, int m, int has_new, double* __restrict__ state) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int NG = 2 * m + 1, NV = 2 * m + 3, ig = 2 * m;
    double* rec = state;
    double* G = state + REC_SIZE;
    double* delta = G + NG * NG;
    const double *ds = dots, *dy = dots + NV, *dg = dots + 2 * NV;
    int count = rec_int(rec[REC_COUNT], 0, m), head = rec_int(rec[REC_HEAD], 0, m - 1), slot = -1, accepted = 0;
    double skipped = rec[REC_SKIPPED];
    const double gg = dg[ig], gmax = dots[3 * NV];
    if (!has_new) {
        count = 0; head = 0;
    } else {
        const double ss = ds[ig + 1], sy = ds[ig + 2], yy = dy[ig + 2];
        if (sy > 0.0 && yy > 0.0 && sy < INFINITY && yy < INFINITY) {
            slot = head;
            head = (head + 1) % m;
            if (count < m) ++count;
            accepted = 1;
            const int is = slot, iy = m + slot;
            for (int v = 0; v < count; ++v) {
                if (v == slot) continue;
                G[is * NG + v] = G[v * NG + is] = ds[v];
                G[iy * NG + v] = G[v * NG + iy] = dy[v];
                G[is * NG + m + v] = G[(m + v) * NG + is] = ds[m + v];
                G[iy * NG + m + v] = G[(m + v) * NG + iy] = dy[m + v];
            }
            G[is * NG + is] = ss;
            G[iy * NG + iy] = yy;
            G[is * NG + iy] = G[iy * NG + is] = sy;
        } else {
            skipped += 1.0;
        }
    }
    for (int v = 0; v < count; ++v) {
        G[ig * NG + v] = G[v * NG + ig] = v == slot ? dg[ig + 1] : dg[v];
        G[ig * NG + m + v] = G[(m + v) * NG + ig] = v == slot ? dg[ig + 2] : dg[m + v];
    }
    G[ig * NG + ig] = gg;

    // the two-loop recursion with q, r held as coefficients over (S slots, Y slots, g)
    for (int j = 0; j < NG; ++j) delta[j] = 0.0;
    delta[ig] = -1.0;
    double al[LB_MAX_M];
    auto row_dot = [&](int row) {
        double t = 0.0;
        for (int v = 0; v < count; ++v) t = fma(delta[v], G[row * NG + v], t);
        for (int v = 0; v < count; ++v) t = fma(delta[m + v], G[row * NG + m + v], t);
        return fma(delta[ig], G[row * NG + ig], t);
    };
    for (int k = 0; k < count; ++k) {                    // newest to oldest
        const int i = (head - 1 - k + 2 * m) % m;
        al[k] = row_dot(i) / G[i * NG + m + i];
        delta[m + i] -= al[k];
    }
    if (count) {
        const int i = (head - 1 + m) % m;
        const double gamma = G[i * NG + m + i] / G[(m + i) * NG + m + i];
        for (int j = 0; j < NG; ++j) delta[j] *= gamma;
    }
    for (int k = count - 1; k >= 0; --k) {               // oldest to newest
        const int i = (head - 1 - k + 2 * m) % m;
        const double beta = row_dot(m + i) / G[i * NG + m + i];
        delta[i] += al[k] - beta;
    }
    rec[REC_ALPHA0] = count ? 1.0 : (gg > 1.0 ? 1.0 / sqrt(gg) : 1.0);
    rec[REC_GTP] = row_dot(ig);
    rec[REC_GG] = gg;
    rec[REC_GMAX] = gmax;
    rec[REC_COUNT] = (double)count;
    rec[REC_SKIPPED] = skipped;
    rec[REC_ACCEPTED] = (double)accepted;
    rec[REC_SLOT] = (double)slot;
    rec[REC_HEAD] = (double)head;
}

// An accepted pair goes into its ring slot; p[i] = the fma chain of delta_j vector_j[i] over the S slots held, the Y slots
// held, then g.
__global__ __launch_bounds__(256) void lbfgs_combine_kernel(double* __restrict__ S, double* __restrict__ Y, const double* __restrict__ g,
                                                            const double* __restrict__ s_new, const double* __restrict__ y_new,
                                                            long n, int m, const double* __restrict__ state, double* __restrict__ p) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int count = rec_int(state[REC_COUNT], 0, m), slot = rec_int(state[REC_SLOT], -1, m - 1);
    const int accepted = slot >= 0 && state[REC_ACCEPTED] == 1.0;
    const double* delta = state + REC_SIZE + (2 * m + 1) * (2 * m + 1);
    double sv = 0.0, yv = 0.0;
    if (accepted) {
        sv = s_new[i]; yv = y_new[i];
        S[(long)slot * n + i] = sv;
        Y[(long)slot * n + i] = yv;
    }
    double t = 0.0;
    for (int v = 0; v < count; ++v) t = fma(delta[v], (accepted && v == slot) ? sv : S[(long)v * n + i], t);
    for (int v = 0; v < count; ++v) t = fma(delta[m + v], (accepted && v == slot) ? yv : Y[(long)v * n + i], t);
    p[i] = fma(delta[2 * m], g[i], t);
}

int check_rows(const char* who, long N, int C) {
    VSOM_REQUIRE(N >= 1 && C >= 1, VSOM_EINVAL, "%s: non-positive size N=%ld C=%d", who, N, C);
    VSOM_REQUIRE(C >= 2 && C <= PROBE_MAX_C, VSOM_EUNSUPPORTED, "%s: C=%d classes outside [2, %d]", who, C, PROBE_MAX_C);
    VSOM_REQUIRE(N >= 2 && N <= PROBE_MAX_ROWS, VSOM_EUNSUPPORTED, "%s: N=%ld rows outside [2, %ld]", who, N, PROBE_MAX_ROWS);
    return VSOM_OK;
}

int check_weights(const char* who, int C, int D) {
    VSOM_REQUIRE(C >= 1 && D >= 1, VSOM_EINVAL, "%s: non-positive size C=%d D=%d", who, C, D);
    VSOM_REQUIRE(C >= 2 && C <= PROBE_MAX_C && C <= D, VSOM_EUNSUPPORTED, "%s: C=%d classes outside [2, min(%d, D=%d)]", who, C,
                 PROBE_MAX_C, D);
    return VSOM_OK;
}

int check_part(const char* who, const double* part, long n_part, long need) {
    VSOM_REQUIRE(part && n_part >= need, VSOM_EWORKSPACE, "%s: partial buffer null or too small (%ld < %ld doubles)", who, n_part, need);
    return VSOM_OK;
}

}  // namespace
}  // namespace vsom

using namespace vsom;

extern "C" {

long vsom_probe_parts(long N, int C) {
    if (N <= 0 || C < 2 || C > PROBE_MAX_C || N > PROBE_MAX_ROWS) return 0;
    return (long)row_plan(N, C).nblk * (C + 1 > PROBE_MAX_STEPS ? C + 1 : PROBE_MAX_STEPS);
}

long vsom_probe_fold_parts(int C, int D) {
    if (C <= 0 || D <= 0) return 0;
    return 3L * vec_plan((long)C * D, FOLD_MAX_BLOCKS).nblk;
}

int vsom_probe_fold(const double* A, const double* invstd, int C, int D, float* B, long ldb, const double* W, double* pen,
                    double* part, long n_part, vsom_stream_t stream) {
    VSOM_REQUIRE(A && invstd && B, VSOM_EINVAL, "probe_fold: null pointer");
    VSOM_REQUIRE((W == nullptr) == (pen == nullptr), VSOM_EINVAL, "probe_fold: W and pen go together");
    if (int rc = check_weights("probe_fold", C, D)) return rc;
    VSOM_REQUIRE(ldb >= D, VSOM_EINVAL, "probe_fold: row stride below the row length (ldb=%ld)", ldb);
    const long n = (long)C * D;
    const VecPlan p = vec_plan(n, FOLD_MAX_BLOCKS);
    if (W)
        if (int rc = check_part("probe_fold", part, n_part, 3L * p.nblk)) return rc;
    VSOM_LAUNCH(probe_fold_kernel, dim3(p.nblk), dim3(256), 0, stream, A, invstd, n, D, B, ldb, W, p.chunks_per, part);
    if (W) VSOM_LAUNCH(probe_reduce_kernel, dim3(1), dim3(256), 0, stream, (const double*)part, p.nblk, 3, 0, pen, 3, pen);
    return launch_status("probe_fold_kernel");
}

int vsom_probe_residual(const float* Z, long ldz, long N, int C, const double* b, const int64_t* y, float* R, long ldr, double* loss,
                        double* gb, int64_t* pred, double* prob, int* status, double* part, long n_part, vsom_stream_t stream) {
    VSOM_REQUIRE(Z && y && R && loss && gb && status, VSOM_EINVAL, "probe_residual: null pointer");
    if (int rc = check_rows("probe_residual", N, C)) return rc;
    VSOM_REQUIRE(ldz >= C && ldr >= C, VSOM_EINVAL, "probe_residual: row stride below the row length (ldz=%ld ldr=%ld)", ldz, ldr);
    const RowPlan p = row_plan(N, C);
    if (int rc = check_part("probe_residual", part, n_part, (long)p.nblk * (C + 1))) return rc;
    VSOM_LAUNCH(probe_residual_kernel, dim3(p.nblk), dim3(256), 0, stream, Z, ldz, N, C, p.L, p.rows_per, b, y, R, ldr, pred, prob,
                status, part);
    VSOM_LAUNCH(probe_reduce_kernel, dim3(cdiv(C + 1, 256)), dim3(256), 0, stream, (const double*)part, p.nblk, C + 1, 0, gb, C, loss);
    return launch_status("probe_residual_kernel");
}

int vsom_probe_linesearch(const float* Z, const float* Zp, long ldz, long N, int C, const double* b, const double* pb,
                          const int64_t* y, const double* alpha0, int nsteps, double* phi, double* part, long n_part,
                          vsom_stream_t stream) {
    VSOM_REQUIRE(Z && Zp && y && alpha0 && phi, VSOM_EINVAL, "probe_linesearch: null pointer");
    VSOM_REQUIRE((b == nullptr) == (pb == nullptr), VSOM_EINVAL, "probe_linesearch: b and pb go together");
    if (int rc = check_rows("probe_linesearch", N, C)) return rc;
    VSOM_REQUIRE(ldz >= C, VSOM_EINVAL, "probe_linesearch: row stride below the row length (ldz=%ld)", ldz);
    VSOM_REQUIRE(nsteps >= 1 && nsteps <= PROBE_MAX_STEPS, VSOM_EUNSUPPORTED, "probe_linesearch: %d steps outside [1, %d]", nsteps,
                 PROBE_MAX_STEPS);
    const RowPlan p = row_plan(N, C);
    if (int rc = check_part("probe_linesearch", part, n_part, (long)p.nblk * nsteps)) return rc;
    VSOM_LAUNCH(probe_linesearch_kernel, dim3(p.nblk), dim3(256), 0, stream, Z, Zp, ldz, N, C, p.L, p.rows_per, b, pb, y, alpha0, nsteps,
                part);
    VSOM_LAUNCH(probe_reduce_kernel, dim3(1), dim3(256), 0, stream, (const double*)part, p.nblk, nsteps, 0, phi, nsteps, phi);
    return launch_status("probe_linesearch_kernel");
}

int vsom_probe_step(const double* phi, int nsteps, const double* alpha0, const double* f0, const double* pen, const double* gtp,
                    double lam, double c1, float* Z, const float* Zp, long ldz, long N, int C, double* theta, const double* p,
                    double* s_new, long n, double* rec, vsom_stream_t stream) {
    VSOM_REQUIRE(phi && alpha0 && f0 && pen && gtp && Z && Zp && theta && p && s_new && rec, VSOM_EINVAL, "probe_step: null pointer");
    if (int rc = check_rows("probe_step", N, C)) return rc;
    VSOM_REQUIRE(ldz >= C && n >= 1, VSOM_EINVAL, "probe_step: bad sizes ldz=%ld n=%ld", ldz, n);
    VSOM_REQUIRE(nsteps >= 1 && nsteps <= PROBE_MAX_STEPS, VSOM_EUNSUPPORTED, "probe_step: %d steps outside [1, %d]", nsteps,
                 PROBE_MAX_STEPS);
    const long most = N * C > n ? N * C : n;
    int grid = cdiv(most, 256);
    if (grid > 2048) grid = 2048;
    VSOM_LAUNCH(probe_step_kernel, dim3(grid), dim3(256), 0, stream, phi, nsteps, alpha0, f0, pen, gtp, 1.0 / (double)N, lam, c1, Z, Zp,
                ldz, N, C, theta, p, s_new, n, rec);
    return launch_status("probe_step_kernel");
}

int vsom_probe_gradient(const float* Zt, long ldz, const double* invstd, const double* theta, const double* gb, int C, int D,
                        int intercept, long N, double lam, const double* g_prev, double* g, double* y_new, vsom_stream_t stream) {
    VSOM_REQUIRE(Zt && invstd && theta && g, VSOM_EINVAL, "probe_gradient: null pointer");
    VSOM_REQUIRE(!intercept || gb, VSOM_EINVAL, "probe_gradient: an intercept needs gb");
    VSOM_REQUIRE((g_prev == nullptr) == (y_new == nullptr), VSOM_EINVAL, "probe_gradient: g_prev and y_new go together");
    if (int rc = check_weights("probe_gradient", C, D)) return rc;
    VSOM_REQUIRE(ldz >= D && N >= 1, VSOM_EINVAL, "probe_gradient: bad sizes ldz=%ld N=%ld", ldz, N);
    const long n = (long)C * D + (intercept ? C : 0);
    VSOM_LAUNCH(probe_gradient_kernel, dim3(cdiv(n, 256)), dim3(256), 0, stream, Zt, ldz, invstd, theta, gb, C, D, n, 1.0 / (double)N, lam,
                g_prev, g, y_new);
    return launch_status("probe_gradient_kernel");
}

long vsom_lbfgs_state_doubles(int m) {
    if (m < 1 || m > LB_MAX_M) return 0;
    return REC_SIZE + (long)(2 * m + 1) * (2 * m + 1) + (2 * m + 1);
}

long vsom_lbfgs_parts(long n, int m) {
    if (n <= 0 || m < 1 || m > LB_MAX_M) return 0;
    return (long)vec_plan(n, LB_MAX_BLOCKS).nblk * (3 * (2 * m + 3) + 1);
}

int vsom_lbfgs_dots(const double* S, const double* Y, const double* g, const double* s_new, const double* y_new, long n, int m,
                    int has_new, const double* state, double* dots, double* part, long n_part, vsom_stream_t stream) {
    VSOM_REQUIRE(S && Y && g && state && dots, VSOM_EINVAL, "lbfgs_dots: null pointer");
    VSOM_REQUIRE(!has_new || (s_new && y_new), VSOM_EINVAL, "lbfgs_dots: a new pair needs s_new and y_new");
    VSOM_REQUIRE(n >= 1, VSOM_EINVAL, "lbfgs_dots: n=%ld", n);
    VSOM_REQUIRE(m >= 1 && m <= LB_MAX_M, VSOM_EUNSUPPORTED, "lbfgs_dots: memory m=%d outside [1, %d]", m, LB_MAX_M);
    const VecPlan p = vec_plan(n, LB_MAX_BLOCKS);
    const int W = 3 * (2 * m + 3) + 1;
    if (int rc = check_part("lbfgs_dots", part, n_part, (long)p.nblk * W)) return rc;
    VSOM_LAUNCH(lbfgs_dots_kernel, dim3(p.nblk), dim3(256), 0, stream, S, Y, g, s_new, y_new, n, m, has_new ? 1 : 0, state, p.chunks_per,
                part);
    VSOM_LAUNCH(probe_reduce_kernel, dim3(1), dim3(256), 0, stream, (const double*)part, p.nblk, W, 1, dots, W, dots);
    return launch_status("lbfgs_dots_kernel");
}

int vsom_lbfgs_coeff(const double* dots, int m, int has_new, double* state, vsom_stream_t stream) {
    VSOM_REQUIRE(dots && state, VSOM_EINVAL, "lbfgs_coeff: null pointer");
    VSOM_REQUIRE(m >= 1 && m <= LB_MAX_M, VSOM_EUNSUPPORTED, "lbfgs_coeff: memory m=%d outside [1, %d]", m, LB_MAX_M);
    VSOM_LAUNCH(lbfgs_coeff_kernel, dim3(1), dim3(64), 0, stream, dots, m, has_new ? 1 : 0, state);
    return launch_status("lbfgs_coeff_kernel");
}

int vsom_lbfgs_combine(double* S, double* Y, const double* g, const double* s_new, const double* y_new, long n, int m,
                       const double* state, double* p, vsom_stream_t stream) {
    VSOM_REQUIRE(S && Y && g && state && p, VSOM_EINVAL, "lbfgs_combine: null pointer");
    VSOM_REQUIRE(n >= 1, VSOM_EINVAL, "lbfgs_combine: n=%ld", n);
    VSOM_REQUIRE(m >= 1 && m <= LB_MAX_M, VSOM_EUNSUPPORTED, "lbfgs_combine: memory m=%d outside [1, %d]", m, LB_MAX_M);
    // s_new / y_new are read only when the record says a pair was accepted; a caller without one passes has_new = 0 to
    // vsom_lbfgs_coeff, which clears that flag
    VSOM_LAUNCH(lbfgs_combine_kernel, dim3(cdiv(n, 256)), dim3(256), 0, stream, S, Y, g, s_new, y_new, n, m, state, p);
    return launch_status("lbfgs_combine_kernel");
}

}  // extern "C"
