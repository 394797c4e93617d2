// Attention rollout (Abnar and Zuidema 2020, with the head fusion of the vit-explain recipe): one query row of the
// product of the blocks' residual-mixed attention matrices, as a vector-matrix chain.  vsom_attention_rollout_step is one
// link: v_out[b, :] = v_in[b, :] A_b, with A_b [N, N] never held anywhere -- a wave forms four rows of it at a time in
// registers and folds them into the column sums at once.
//
//   P_h[i, j] = softmax_j(scale q_i . k_j), the row's own maximum subtracted and its own sum dividing (attn_probs_kernel's
//               arithmetic, instruction for instruction; the saved log-sum-exp is not read, for the reason given there)
//   F[i, j]   = mean / max / min over the heads of P_h[i, j]
//   A[i, j]   = (alpha F[i, j] + (1 - alpha) [i == j]) / (alpha sum_j F[i, j] + (1 - alpha))
//
// A workgroup owns one sample and RO_ROWS = 16 query rows, four to a wave.  Per head it stages that head's K (N rows at a
// pitch of hd | 1 floats: lanes are keys, so the odd pitch spreads a column of K over the banks) and its own 16 rows of Q
// in LDS, with 4-byte loads and no alignment-dependent path.  A wave then runs d outermost over a register tile of
// 4 rows x NCH key chunks: 4 broadcast reads of Q and NCH reads of K feed 4 NCH fma chains, each in ascending d.  The
// softmax of a row stays in those registers; F is a second register tile that the heads fold into.  After the last head the
// wave adds v_in[i] A[i, :] of its rows, in ascending i, into NCH accumulators per lane; the four waves' accumulators meet
// in LDS and are added in wave order; the workgroup writes one partial [N] to the workspace.  rollout_sum_kernel adds a
// sample's partials in block order, in fp64, and rounds once.  No atomics, no grid-wide barrier, no spin-wait, every loop
// bounded by the shape.  The minimum over the heads is taken of the logarithms, log P_h = (s - max) - log(sum), and leaves
// them only relative to the fused row's own largest entry: where two saturated heads disagree every min_h P_h[i, j] is
// below the smallest float (the row's sum came out as 0 and alpha = 1 divided by it), while the row normalisation needs
// only their ratios.  With alpha < 1 the row's scale exp(max) returns as one factor; with alpha = 1 it cancels.
// The bits depend on (N, H, hd, fusion, alpha) and the sample's own data alone -- not on B, not on
// the sample's place in the batch.
#include "common.h"

namespace vsom {
namespace {

constexpr int RO_THREADS = 256;                          // four waves
constexpr int RO_WAVES = RO_THREADS / 64;
constexpr int RO_RPW = 4;                                // query rows in a wave's register tile
constexpr int RO_ROWS = RO_WAVES * RO_RPW;               // query rows of a workgroup
constexpr int RO_STAGE = 8;                              // K elements a thread loads before it stores the first
constexpr int RO_MAX_CHUNKS = 5;                         // key chunks of 64 lanes: N <= 320
constexpr size_t RO_MAX_LDS = 160 * 1024;

enum { RO_MEAN = 0, RO_MAX = 1, RO_MIN = 2 };

inline int ro_pitch(int hd) { return hd | 1; }
inline int ro_chunks(int N) { return (N + 63) / 64; }
inline int ro_blocks(int N) { return (N + RO_ROWS - 1) / RO_ROWS; }
// K of one head, the workgroup's rows of Q, the waves' accumulators
inline size_t ro_lds_bytes(int N, int hd) {
    return ((size_t)N * ro_pitch(hd) + (size_t)RO_ROWS * hd + (size_t)RO_WAVES * ro_chunks(N) * 64) * sizeof(float);
}

template <int NCH>
__global__ __launch_bounds__(RO_THREADS) void rollout_rows_kernel(const float* __restrict__ qkv, const float* __restrict__ v_in,
                                                                  float* __restrict__ parts, int blocks, int N, int H, int hd,
                                                                  int fusion, float alpha, float scale) {
    extern __shared__ float ro_lds[];
    const int pitch = hd | 1;
    float* Ks = ro_lds;                                  // [N][pitch]
    float* Qs = Ks + (size_t)N * pitch;                  // [RO_ROWS][hd]
    float* Cs = Qs + RO_ROWS * hd;                       // [RO_WAVES][NCH * 64]

    const int b = blockIdx.x / blocks, rb = blockIdx.x % blocks;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int E = H * hd, E3 = 3 * E;
    const float* base = qkv + (long)b * N * E3;
    const int row0 = rb * RO_ROWS + wave * RO_RPW;       // the wave's first query row

    int kj[NCH];                                         // the lane's keys, clamped into the staged rows
#pragma unroll
    for (int c = 0; c < NCH; ++c) kj[c] = min(c * 64 + lane, N - 1) * pitch;

    float F[RO_RPW][NCH];
    for (int h = 0; h < H; ++h) {
        __syncthreads();                                 // the previous head's K and Q are read out
        // (j, d) walks the head's K in steps of RO_THREADS elements without a division per element; RO_STAGE loads are
        // in flight before the first of them is stored (one load, one store at a time left the workgroup waiting on memory)
        {
            const int dstep = RO_THREADS % hd, jstep = RO_THREADS / hd;
            int j = tid / hd, d = tid % hd;
            const float* kh = base + E + h * hd;
            while (j < N) {
                float kv[RO_STAGE];
                int at[RO_STAGE];
#pragma unroll
                for (int u = 0; u < RO_STAGE; ++u) {
                    at[u] = (j < N) ? j * pitch + d : -1;
                    kv[u] = (j < N) ? kh[(long)j * E3 + d] : 0.f;
                    d += dstep;
                    j += jstep;
                    if (d >= hd) { d -= hd; ++j; }
                }
#pragma unroll
                for (int u = 0; u < RO_STAGE; ++u)
                    if (at[u] >= 0) Ks[at[u]] = kv[u];
            }
            const float* qh = base + h * hd;
            for (int t = tid; t < RO_ROWS * hd; t += RO_THREADS) {
                const int r = t / hd, dd = t % hd;
                const int i = min(rb * RO_ROWS + r, N - 1);          // a row past N repeats the last one and is never used
                Qs[t] = qh[(long)i * E3 + dd];
            }
        }
        __syncthreads();
        if (row0 >= N) continue;                         // a wave without a row (the last block) stages and waits, nothing more

        float s[RO_RPW][NCH];
#pragma unroll
        for (int r = 0; r < RO_RPW; ++r)
#pragma unroll
            for (int c = 0; c < NCH; ++c) s[r][c] = 0.f;
        const float* qw = Qs + wave * RO_RPW * hd;
#pragma unroll 4
        for (int d = 0; d < hd; ++d) {
            float q[RO_RPW], k[NCH];
#pragma unroll
            for (int r = 0; r < RO_RPW; ++r) q[r] = qw[r * hd + d];
#pragma unroll
            for (int c = 0; c < NCH; ++c) k[c] = Ks[kj[c] + d];
#pragma unroll
            for (int r = 0; r < RO_RPW; ++r)
#pragma unroll
                for (int c = 0; c < NCH; ++c) s[r][c] = fmaf(q[r], k[c], s[r][c]);
        }
#pragma unroll
        for (int r = 0; r < RO_RPW; ++r) {
            float m = -INFINITY;
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                s[r][c] = __fmul_rn(s[r][c], scale);           // rounded here, as attn_probs_kernel's store does: never fused into s - m
                if (c * 64 + lane < N) m = fmaxf(m, s[r][c]);
            }
            m = wave_max(m);
            float z = 0.f, dl[NCH];
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const bool valid = c * 64 + lane < N;
                dl[c] = valid ? s[r][c] - m : -INFINITY;
                s[r][c] = valid ? __expf(dl[c]) : 0.f;
                z += s[r][c];
            }
            const float zs = wave_sum(z);
            if (fusion == RO_MIN) {                      // the logarithms: see the note on the minimum above the kernel
                const float lz = logf(zs);
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    const float l = dl[c] - lz;
                    F[r][c] = (h == 0) ? l : fminf(F[r][c], l);
                }
            } else {
                const float inv = 1.0f / zs;
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    const float p = s[r][c] * inv;
                    if (h == 0) F[r][c] = p;
                    else if (fusion == RO_MEAN) F[r][c] += p;
                    else F[r][c] = fmaxf(F[r][c], p);
                }
            }
        }
    }

    // v_in[i] A[i, :] of the wave's rows, ascending i; a key past N holds F = 0 and is never the diagonal
    float acc[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) acc[c] = 0.f;
    const float rest = 1.0f - alpha;
#pragma unroll
    for (int r = 0; r < RO_RPW; ++r) {
        const int i = row0 + r;
        if (i < N) {                                     // uniform in the wave: the shuffles are whole
            float g = (fusion == RO_MEAN) ? 1.0f / (float)H : 1.0f;      // F holds g^-1 times the fused row
            if (fusion == RO_MIN) {
                float M = -INFINITY;
#pragma unroll
                for (int c = 0; c < NCH; ++c) M = fmaxf(M, F[r][c]);
                M = wave_max(M);
#pragma unroll
                for (int c = 0; c < NCH; ++c) F[r][c] = (c * 64 + lane < N) ? __expf(F[r][c] - M) : 0.f;
                g = (rest == 0.f) ? 1.0f : __expf(M);    // alpha = 1: the scale cancels, so it is never formed
            }
            float t = 0.f;
#pragma unroll
            for (int c = 0; c < NCH; ++c) t += F[r][c];
            const float ag = alpha * g;
            const float den = fmaf(ag, wave_sum(t), rest);
            const float w = v_in[(long)b * N + i] / den;
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const float a = fmaf(ag, F[r][c], (c * 64 + lane == i) ? rest : 0.f);
                acc[c] = fmaf(w, a, acc[c]);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < NCH; ++c) Cs[wave * NCH * 64 + c * 64 + lane] = acc[c];
    __syncthreads();
    float* out = parts + (long)blockIdx.x * N;
    for (int j = tid; j < N; j += RO_THREADS) {
        float t = Cs[j];
#pragma unroll
        for (int w = 1; w < RO_WAVES; ++w) t += Cs[w * NCH * 64 + j];
        out[j] = t;
    }
}

// v_out[b, j] = the partials of sample b at column j, added in block order in fp64, rounded once
__global__ __launch_bounds__(256) void rollout_sum_kernel(const float* __restrict__ parts, float* __restrict__ v_out, long BN, int N,
                                                          int blocks) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= BN) return;
    const long b = t / N;
    const int j = (int)(t - b * N);
    const float* p = parts + b * blocks * N + j;
    double sum = 0.0;
    for (int k = 0; k < blocks; ++k) sum += (double)p[(long)k * N];
    v_out[t] = (float)sum;
}

inline bool ro_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + nb && y < x + na;
}

inline bool ro_fits(int N, int hd) { return ro_chunks(N) <= RO_MAX_CHUNKS && ro_lds_bytes(N, hd) <= RO_MAX_LDS; }

template <int NCH>
int rollout_launch(const float* qkv, const float* v_in, float* parts, float* v_out, int B, int N, int H, int hd, int fusion, float alpha,
                   size_t lds, hipStream_t stream) {
    static const int attr_rc = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(rollout_rows_kernel<NCH>),
                                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)RO_MAX_LDS);
    VSOM_REQUIRE(attr_rc == 0, VSOM_EUNSUPPORTED, "attention_rollout_step: cannot reserve %d bytes of LDS", (int)RO_MAX_LDS);
    const int blocks = ro_blocks(N);
    VSOM_LAUNCH(rollout_rows_kernel<NCH>, dim3((unsigned)((long)B * blocks)), dim3(RO_THREADS), lds, stream, qkv, v_in, parts, blocks, N, H, hd, fusion, alpha,
                1.0f / sqrtf((float)hd));
    if (int rc = launch_status("rollout_rows_kernel")) return rc;
    const long BN = (long)B * N;
    VSOM_LAUNCH(rollout_sum_kernel, dim3(cdiv(BN, 256)), dim3(256), 0, stream, (const float*)parts, v_out, BN, N, blocks);
    return launch_status("rollout_sum_kernel");
}

}  // namespace
}  // namespace vsom

using namespace vsom;

extern "C" {

long vsom_attention_rollout_ws_size(int B, int N, int H, int hd) {
    if (B < 1 || N < 1 || H < 1 || hd < 1 || !ro_fits(N, hd)) return 0;
    return (long)B * ro_blocks(N) * N * (long)sizeof(float);
}

int vsom_attention_rollout_step(const float* qkv, const float* v_in, float* v_out, int B, int N, int H, int hd, int fusion, float alpha,
                                void* ws, long ws_size, vsom_stream_t stream) {
    VSOM_REQUIRE(qkv && v_in && v_out, VSOM_EINVAL, "attention_rollout_step: null pointer");
    VSOM_REQUIRE(B > 0 && N > 0 && H > 0 && hd > 0, VSOM_EINVAL, "attention_rollout_step: bad shape B=%d N=%d H=%d hd=%d", B, N, H, hd);
    VSOM_REQUIRE(fusion == RO_MEAN || fusion == RO_MAX || fusion == RO_MIN, VSOM_EINVAL,
                 "attention_rollout_step: fusion = %d (0 mean, 1 max, 2 min)", fusion);
    VSOM_REQUIRE(alpha > 0.f && alpha <= 1.f, VSOM_EINVAL, "attention_rollout_step: alpha = %g (wants 0 < alpha <= 1)", (double)alpha);
    const size_t vbytes = (size_t)B * N * sizeof(float);
    VSOM_REQUIRE(!ro_overlap(v_out, vbytes, v_in, vbytes), VSOM_EINVAL, "attention_rollout_step: v_out overlaps v_in");
    const size_t lds = ro_lds_bytes(N, hd);
    VSOM_REQUIRE(ro_fits(N, hd), VSOM_EUNSUPPORTED,
                 "attention_rollout_step: N=%d hd=%d needs %zu B of LDS and %d key chunks (limits: 160 KiB, %d chunks, N <= %d)", N, hd, lds,
                 ro_chunks(N), RO_MAX_CHUNKS, RO_MAX_CHUNKS * 64);
    VSOM_REQUIRE((long)B * ro_blocks(N) <= 0x7fffffffL, VSOM_EUNSUPPORTED, "attention_rollout_step: B = %d is too many samples a call", B);
    const long need = vsom_attention_rollout_ws_size(B, N, H, hd);
    VSOM_REQUIRE(ws != nullptr && ws_size >= need, VSOM_EWORKSPACE, "attention_rollout_step: workspace too small or null (%ld < %ld bytes)",
                 ws ? ws_size : 0L, need);
    float* parts = static_cast<float*>(ws);
    switch (ro_chunks(N)) {
        case 1: return rollout_launch<1>(qkv, v_in, parts, v_out, B, N, H, hd, fusion, alpha, lds, stream);
        case 2: return rollout_launch<2>(qkv, v_in, parts, v_out, B, N, H, hd, fusion, alpha, lds, stream);
        case 3: return rollout_launch<3>(qkv, v_in, parts, v_out, B, N, H, hd, fusion, alpha, lds, stream);
        case 4: return rollout_launch<4>(qkv, v_in, parts, v_out, B, N, H, hd, fusion, alpha, lds, stream);
        default: return rollout_launch<5>(qkv, v_in, parts, v_out, B, N, H, hd, fusion, alpha, lds, stream);
    }
}

}  // extern "C"
