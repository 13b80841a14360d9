// Batched RangeDetector (mmw_range_detect): the 1-D CFAR of the float64 range profile of every frame and its ordered hit list.
//
// RangeDetector.process (processors/range_detector.py:59-83) is RangeProcessor.process -> cfar_detector.detect -> the indices.
// The profile is made by the existing range-profile kernels (range_profile_impl<double>, the code of mmw_range_profile_f64);
// k_range_detect then does what k_cfar1d, a mask and a compaction would do in three launches: one workgroup per frame evaluates
// cfar1d_threshold (the code of k_cfar1d, so thresholds and decisions are bit-identical to mmw_cfar1d) for every cell, keeps
// the flags in the LDS and has wave 0 append the set ones in ascending order (wave_append_row, as k_seq_rows does).
#pragma once
#include "mmw_seq.h"

namespace mmw {

constexpr int RANGE_DETECT_MAX_S = 48 * 1024;       // one flag byte per cell in the LDS

// prof[F][L] -> thr[F][L] (if given), dets[F][cap] (the first min(counts[f], cap) entries: cells with prof > thr, ascending),
// counts[F] (exact also past cap)
__global__ __launch_bounds__(256) void k_range_detect(Cfar1dArgs p, int32_t *dets, int32_t *counts, int cap) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint8_t *hit = reinterpret_cast<uint8_t *>(smem);               // [L]
    const int L = p.L;
    const long f = blockIdx.x;
    const double *x = p.x + f * L;
    for (int i = threadIdx.x; i < L; i += 256) {
        double est;
        const double thr = cfar1d_threshold(p, x, i, &est);
        if (p.thr) p.thr[f * L + i] = thr;
        hit[i] = x[i] > thr ? 1 : 0;
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        int32_t *out = dets + f * cap;
        const int n = wave_append_row(hit, L, 0, [&](int pos, int i) {
            if (pos < cap) out[pos] = i;
        });
        if (threadIdx.x == 0) counts[f] = n;
    }
}

}  // namespace mmw
