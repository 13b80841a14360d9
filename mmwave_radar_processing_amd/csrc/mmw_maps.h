// Kernels of the range / Doppler-azimuth maps that are not FFTs: the mean over range rows, the DBS gather and the direct zoom
// transforms (the chirp-z forms are in mmw_czt.h).  (mmw_tu_maps.hip)
#pragma once
#include "mmw_ctx.h"

namespace mmw {

// out[f][c][a] = mean over range rows s in [s_lo, s_hi) of mag[f][a][s][c]
// (DopplerAzimuthProcessor.process: np.mean(resp, axis=0), processors/doppler_azimuth_resp.py:489)
__global__ __launch_bounds__(256) void k_mean_over_range(const float *mag, float *out, int F, int A, int S, int C,
                                                          int s_lo, int s_hi) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (long)F * A * C) return;
    const int c = (int)(gid % C);
    const int a = (int)((gid / C) % A);
    const long f = gid / ((long)C * A);
    const float *src = mag + ((f * A + a) * S) * (long)C + c;
    float acc = 0.f;
    for (int s = s_lo; s < s_hi; ++s) acc += src[(long)s * C];
    out[(f * C + c) * A + a] = acc / (float)(s_hi - s_lo);
}

// out[f][s][i] = mag[f][ang_idx[i]][s][vel_idx[i]]   (perform_dbs_sharpen,
// processors/range_angle_resp_dbs_enhanced.py:216-263: one [angle bin, :, Doppler bin] column per output angle)
__global__ __launch_bounds__(256) void k_dbs_gather(const float *mag, const int *ang_idx, const int *vel_idx, float *out,
                                                     int F, int A, int S, int C, int n_out) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (long)F * S * n_out) return;
    const int i = (int)(gid % n_out);
    const int s = (int)((gid / n_out) % S);
    const long f = gid / ((long)n_out * S);
    out[gid] = mag[((f * A + ang_idx[i]) * S + s) * (long)C + vel_idx[i]];
}

// Zoom DFT: out[row][k] = sum_n win[n] x[row][n] exp(-j 2 pi n (f0 + k df)), frequencies in cycles/sample.
// This is what scipy.signal.ZoomFFT evaluates (by Bluestein) for RangeProcessor.zoom_fft
// (processors/range_resp.py:59-102); n and m are a few hundred, so the direct sum in float64 phase is enough.
// One workgroup per row, the windowed row staged in LDS, thread k owns output bins k, k+256, ...
__global__ __launch_bounds__(256) void k_zoom_dft(const float2 *x, long row_stride, long elem_stride, const float *win,
                                                   float2 *out, int n, int m, double f0, double df) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2 *xs = reinterpret_cast<float2 *>(smem);
    const float2 *src = x + (long)blockIdx.x * row_stride;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float2 v = src[(long)i * elem_stride];
        const float w = win ? win[i] : 1.f;
        xs[i] = make_float2(v.x * w, v.y * w);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < m; k += 256) {
        const double f = f0 + (double)k * df;
        double re = 0.0, im = 0.0;
        for (int i = 0; i < n; ++i) {
            double turns = f * (double)i;
            turns -= rint(turns);
            double sn, cs;
            sincospi(-2.0 * turns, &sn, &cs);
            re += (double)xs[i].x * cs - (double)xs[i].y * sn;
            im += (double)xs[i].x * sn + (double)xs[i].y * cs;
        }
        out[(long)blockIdx.x * m + k] = make_float2((float)re, (float)im);
    }
}

// Doppler zoom transform of DopplerAzimuthProcessor.zoom_fft (processors/doppler_azimuth_resp.py:130-163):
// k_zoom_table  Z[i][k] = exp(-j 2 pi i f[k]) with the phase reduced in float64 (f in cycles per chirp; NaN marks
//               a bin the reference fills with zeros, :267/:285);
// k_zoom_rows   out[row][k] = sum_{i<n} x[row][i] Z[i][k] for the rows (frame*antenna, kept range bin) of the
//               range-FFT cube: RB rows staged in LDS per workgroup, thread k owns one zoom bin.
__global__ __launch_bounds__(256) void k_zoom_table(const double *freq, float2 *Z, int n, int m) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (long)n * m) return;
    const int k = (int)(gid % m), i = (int)(gid / m);
    const double f = freq[k];
    float2 z = make_float2(0.f, 0.f);
    if (f == f) {
        double turns = f * (double)i;
        turns -= rint(turns);
        double sn, cs;
        sincospi(-2.0 * turns, &sn, &cs);
        z = make_float2((float)cs, (float)sn);
    }
    Z[gid] = z;
}

template <int RB>
__global__ __launch_bounds__(256) void k_zoom_rows(const float2 *x, const float2 *Z, float2 *out, int S, int C, int s_lo,
                                                    int s_keep, int n, int m, long total_rows) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2 *xs = reinterpret_cast<float2 *>(smem);           // [RB][n]
    const long row0 = (long)blockIdx.x * RB;
    for (int e = threadIdx.x; e < RB * n; e += 256) {
        const int r = e / n, i = e - r * n;
        const long row = row0 + r;
        float2 v = make_float2(0.f, 0.f);
        if (row < total_rows) {
            const long fv = row / s_keep;
            const int s = s_lo + (int)(row - fv * s_keep);
            v = x[(fv * S + s) * (long)C + i];
        }
        xs[e] = v;
    }
    __syncthreads();
    const int k = blockIdx.y * 256 + threadIdx.x;
    if (k >= m) return;
    float2 acc[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) acc[r] = make_float2(0.f, 0.f);
    for (int i = 0; i < n; ++i) {
        const float2 z = Z[(long)i * m + k];
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const float2 v = xs[r * n + i];
            acc[r].x = fmaf(v.x, z.x, fmaf(-v.y, z.y, acc[r].x));
            acc[r].y = fmaf(v.x, z.y, fmaf(v.y, z.x, acc[r].y));
        }
    }
#pragma unroll
    for (int r = 0; r < RB; ++r)
        if (row0 + r < total_rows) out[(row0 + r) * m + k] = acc[r];
}

}  // namespace mmw
