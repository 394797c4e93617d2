// LDS layout of the attention kernels (attention.hip), written once for the kernels, which take their pointers from it,
// and for the host, which takes the launches' byte counts and the launch plan's bounds from it.  Plain C++: a host-only
// program can include it.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define VSOM_HOST_DEVICE __host__ __device__
#else
#define VSOM_HOST_DEVICE
#endif

namespace vsom {

enum AttnLds : int {
    ATTN_LDS_FWD,      // K, V                         token-0 partial of a wave: o[hdp], m, l
    ATTN_LDS_DQ,       // K, V                                                    gq[hdp]
    ATTN_LDS_DKV,      // Q, dO + row statistics                                  gk | gv
    ATTN_LDS_FUSED,    // K, V, Q, dO + row statistics                            gq | gk | gv
};

// The regions, in this order, as positions of type Pos counted in floats: the kernels build it on the start of dynamic LDS
// (Pos = float*: the members are their pointers), the host on 0 (Pos = size_t: offsets, and end = the floats to request).
//   Y0 .. Y3   the [nrows][hdp + 4] slice images (two or four; a row is a multiple of 16 bytes, see ACfg),
//   L0, L1     the row statistics [nrp] (log-sum-exp, D) where the kernel stages them,
//   X0, X1     two [hdp] vectors of token 0 where the kernel keeps them aside,
//   PA         the tile waves' token-0 partials, `paw` floats per wave.
// A region the kind does not have is empty (its position is the next region's).  Every region that is read as 16-byte
// vectors (Y*, X*) starts at a multiple of 4 floats: nrows (hdp + 4), nrp and hdp all are.
// attn_bwd_shared_kernel is the one kernel that does not build this struct: its LDS is the ATTN_LDS_FUSED layout followed by
// two [hdp] vectors, carved by hand (see there).
template <class Pos>
struct AttnLayout {
    int ntile, nrows, nrp;                      // 16-row tiles, staged rows, rows padded to 4 (the statistics' length)
    int paw;                                    // token-0 partial floats per wave
    Pos Y0, Y1, Y2, Y3, L0, L1, X0, X1, PA, end;

    VSOM_HOST_DEVICE AttnLayout(Pos base, int N, int hdp, bool extra, int nwaves, AttnLds kind) {
        const bool four = kind == ATTN_LDS_FUSED;
        const bool stats = four || kind == ATTN_LDS_DKV;
        const bool vecs = !four;                                      // (the fused kernel reads row 0 of its slices)
        ntile = extra ? (N - 1) >> 4 : (N + 15) >> 4;
        nrows = extra ? N : ntile << 4;
        nrp = (nrows + 3) & ~3;
        paw = kind == ATTN_LDS_FWD ? hdp + 2 : kind == ATTN_LDS_DQ ? hdp : kind == ATTN_LDS_DKV ? 2 * hdp : 3 * hdp;
        const long slice = (long)nrows * (hdp + 4);
        Y0 = base;
        Y1 = Y0 + slice;
        Y2 = Y1 + slice;
        Y3 = Y2 + (four ? slice : 0);
        L0 = Y3 + (four ? slice : 0);
        L1 = L0 + (stats ? nrp : 0);
        X0 = L1 + (stats ? nrp : 0);
        X1 = X0 + (vecs ? hdp : 0);
        PA = X1 + (vecs ? hdp : 0);
        end = PA + nwaves * paw;
    }
};

}  // namespace vsom
