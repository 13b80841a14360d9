// Batched Doppler beam sharpening (mmw_dbs_sharpen): the sharpened range-azimuth image straight from the range-Doppler cube.
//
// perform_dbs_sharpen (processors/range_angle_resp_dbs_enhanced.py:216-263) keeps, per output angle i, the column
// [angle bin a_i, :, Doppler bin k_i] of |compute_3d_windowed_fft| (:137-198).  One such value is a SINGLE bin of the angle
// FFT of one range-Doppler cell:
//   out[f][s][i] = | sum_j hann(n)[j] RD[f][rx[j]][s][k_i] W_A^(j b_i) |,   b_i = (a_i - A/2) mod A  (the fftshift undone),
// so the [A][S][C] cube behind it is never formed: n complex reads and n complex multiply-adds per pixel.
#pragma once
#include "mmw_ctx.h"

namespace mmw {

struct DbsArgs {
    const float2 *rd;       // [nf][V][S][C] range-Doppler cubes of the launch's frames
    const int2 *tab;        // [nf][n_out] (b_i, k_i) of the launch's frames
    const float2 *tw;       // W_A^m = exp(-2 pi i m / A), m < A
    float *out;             // [nf][S][n_out]
    int V, S, C, A, n_out;
    int j0, n_eff;          // the antennas of non-zero window weight are the positions j0 .. j0 + n_eff - 1 of the list
    int ant[MAX_ANT];       // their planes rx[j0 + q] ...
    float w[MAX_ANT];       // ... and weights hann(n)[j0 + q]
};

// One lane per output pixel (s, i) of frame blockIdx.y, pixels in the order they are stored.  The lanes of a wave are
// neighbouring output angles of one to three range rows, so the n_eff loads of a wave each fall into as many 8 C-byte rows of the
// cube (neighbouring angles share a Doppler bin or sit a few bins apart).  The expectation -- argued, not measured: no variant that
// stages the rows in the LDS was built, no cache counter read -- is that every 128-byte line of a row is fetched once, by the wave
// that owns the row, so that a staging copy would add a pass without removing a fetch.  Measured is the family time only
// (DESIGN.md 4.15).
// W_A lives in the LDS (TW_LDS; a table too large for it is read through the L1): 8-byte reads at (j b_i) mod A, which for
// A = 64 span two bank rows -- entries m and m + 32 share a bank, so by the bank rule an instruction costs at most one extra LDS
// cycle per half wave (even j only: for odd j, 32 neighbouring b_i give 32 different banks); the conflict counter was not read.
// The two end antennas of np.hanning(n) weigh exactly zero and are not read (they are not in ant[]); n_eff == 0 (n == 2)
// stores zeros, as the reference's all-zero window does.
template <bool TW_LDS>
__global__ __launch_bounds__(256) void k_dbs_sharpen(DbsArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2 *tws = reinterpret_cast<float2 *>(smem);
    if (TW_LDS) {
        for (int m = threadIdx.x; m < a.A; m += 256) tws[m] = a.tw[m];
        __syncthreads();
    }
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.S * a.n_out) return;
    const long f = blockIdx.y;
    const int s = p / a.n_out, i = p - s * a.n_out;
    const int2 t = a.tab[f * a.n_out + i];
    const long plane = (long)a.S * a.C;
    const float2 *src = a.rd + (f * a.V * a.S + s) * (long)a.C + t.y;
    int m = (int)(((long)a.j0 * t.x) % a.A);
    float re = 0.f, im = 0.f;
#pragma unroll 4
    for (int q = 0; q < a.n_eff; ++q) {
        const float2 x = src[a.ant[q] * plane];
        const float2 w = TW_LDS ? tws[m] : a.tw[m];
        const float wr = a.w[q] * w.x, wi = a.w[q] * w.y;
        re += x.x * wr - x.y * wi;
        im += x.x * wi + x.y * wr;
        m += t.x;
        if (m >= a.A) m -= a.A;
    }
    a.out[f * a.S * a.n_out + p] = sqrtf(re * re + im * im);
}

}  // namespace mmw
