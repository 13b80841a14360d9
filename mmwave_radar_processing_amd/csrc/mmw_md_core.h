// What the partial-DFT kernels over one antenna's [S][C] slab share (mmw_micro_doppler.h, mmw_sar.h): the column tiling, the LDS
// budget and the choice of the rows in flight, and the complex multiply-add whose rounding both rest on.  Inline code only: each
// kernel header is still included by exactly one translation unit.
#pragma once
#include "mmw_ctx.h"

namespace mmw {

constexpr int MD_COLS = 128;        // chirp columns of one pass of a workgroup: two per lane
constexpr int MD_LDS_MAX = 160 * 1024;

// dynamic LDS of k_micro_doppler<KT>: the partial sums of waves 1..3, the chunk's rows Z[C][KT], W_C and the running maxima
inline size_t md_lds_bytes(int KT, int C) {
    return (size_t)3 * KT * MD_COLS * sizeof(float2) + (size_t)C * KT * sizeof(float2) + (size_t)C * sizeof(float2) +
           (size_t)C * sizeof(unsigned);
}

// Rows of the window a workgroup carries at once (4, 8 or 16).  A chunk of KT rows costs one pass over the slab and the window is
// padded to whole chunks, so the choice weighs the padded rows against the passes: the KT with the least KP + 2 * passes among
// those the LDS holds at this C, the larger one on a tie (fitted to the measured sweeps of DESIGN.md 4.16: 17 rows run fastest
// as 3 x 8, 25 rows as 2 x 16).  forced: the MMW_MD_KT experiment switch.  0: no kernel fits the LDS.
inline int md_pick_kt(int K, int C, int forced) {
    if (forced == 4 || forced == 8 || forced == 16) return md_lds_bytes(forced, C) <= (size_t)MD_LDS_MAX ? forced : 0;
    int best = 0;
    long best_cost = 0;
    for (int kt : {16, 8, 4}) {
        if (md_lds_bytes(kt, C) > (size_t)MD_LDS_MAX) continue;
        const long passes = ((long)K + kt - 1) / kt, cost = passes * kt + 2 * passes;
        if (!best || cost < best_cost) best = kt, best_cost = cost;
    }
    return best;
}

// acc += a b as four fused multiply-adds in a fixed order: what the compiler contracts does not depend on the instantiation, so
// the rows in flight (KT) do not change a bit of the result
__device__ __forceinline__ void md_cmac(float2 &acc, const float2 a, const float2 b) {
    acc.x = fmaf(a.x, b.x, acc.x);
    acc.y = fmaf(a.x, b.y, acc.y);
    acc.x = fmaf(-a.y, b.y, acc.x);
    acc.y = fmaf(a.y, b.x, acc.y);
}

}  // namespace mmw
