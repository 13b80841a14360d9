// Self-calibration of the synthetic array against targets of opportunity (mmw_synth_array_calibrate): the stage
// between two contractions of mmw_synth_array.h.  Per output frame, with X[S][E] the window, P[3][E] its geometry, d the directions:
//   spectra   Fq[r][e] = hamming(E)[e] sum_s X[s][e] exp(-2 pi i r s / S)           (no Hann over s), float64
//   range     avg[r] = mean_e 20 log10 |Fq[r][e]|; strict interior local maxima with value >= 0, the three largest, strongest first
//   azimuth   u[a] = |10 log10 |img[r][a n_el]||; the first maximum among the local maxima of u; a row without one drops its target
//   phases    z[e] = Fq[r][e] exp(2 pi i d[:, a, 0].P[:, e] / lambda); Phi[e] = angle(z[e + 1]) - angle(z[e]) wrapped as np.unwrap does
//   solve     delta[:, e] = pinv((2 pi / lambda) d[0:2] of the three targets) Phi[:, e];  Pcal[0:2, 1:] = P[0:2, 1:] - cumsum(delta)
// The decisions and the solve are __host__ __device__ functions: k_sac_frame and the host-only entry
// mmw_diag_synth_array_calib_host call the same code.  A comparison whose operands lie inside the error band of its inputs is
// not decided here: the frame is flagged (status -1) and the caller calibrates it on the host.
//
// A column of a resident frame has ONE spectrum whatever windows it is an element of, and hamming(E)[e] only scales it, so
//   E avg[r] = sum_e 20 log10 hamming(E)[e] + sum_h L[frame of slot h][r],   L[f][r] = sum_j 20 log10 |sum_s x_f[s][j k] W^(r s)|
// k_sac_spectra makes L once per resident frame (float64 direct sums, read in place from the cubes); the window is applied by the
// slot arithmetic of AWindow written out for one element per thread -- slot h = e / Cv, chirp j = e - h Cv, resident frame
// frames[i] - H + 1 + h -- and a slot before the buffer is never read (all zeros: log10(0), a non-finite avg, "no suitable targets").
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "../../include/mmwgpu.h"

namespace mmw {

constexpr int SAC_RUNNING = 0, SAC_STOPPED = 1, SAC_FLAGGED = 2;       // state of a frame inside one call
// why a frame was flagged (bits; info[1] of the host entry)
constexpr int SAC_WHY_RANGE = 1, SAC_WHY_AZIMUTH = 2, SAC_WHY_WRAP = 4, SAC_WHY_COND = 8;
constexpr double SAC_COND_MAX = 1e6;
constexpr double SAC_PI = 3.14159265358979323846;
constexpr int SAC_MAX_S = 3584;          // avg[S] and its error live in the LDS of k_sac_frame

// ------------------------------------------------------------------ step 3: range rows
// avg[r] with |avg[r] - exact| <= err[r].  Returns 3 (rows filled, strongest first), 0 (fewer than three peaks or a non-finite
// value: no suitable targets) or -1 (a comparison inside the band).  With err == 0 everywhere every comparison is decided, equal
// neighbours are a plateau (scipy's _local_maxima_1d: one peak at (first + last) / 2); with err > 0 equal values are inside the band.
__host__ __device__ inline bool sac_close(double a, double b, double band) { return fabs(a - b) <= band && !(band == 0.0 && a == b); }

__host__ __device__ inline int sac_range_rows(const double *avg, const double *err, int S, int rows[3]) {
    rows[0] = rows[1] = rows[2] = -1;
    for (int r = 0; r < S; ++r)
        if (!(fabs(avg[r]) <= DBL_MAX)) return 0;
    for (int r = 0; r + 1 < S; ++r)
        if (sac_close(avg[r], avg[r + 1], err[r] + err[r + 1])) return -1;
    double tv[4] = {0, 0, 0, 0}, te[4] = {0, 0, 0, 0};
    int ti[4] = {-1, -1, -1, -1}, n = 0;
    const int last = S - 1;
    for (int i = 1; i < last; ++i) {
        const double v = avg[i];
        if (!(avg[i - 1] < v)) continue;
        int ahead = i + 1;
        while (ahead < last && avg[ahead] == v) ++ahead;
        if (!(avg[ahead] < v)) continue;
        const int p = (i + ahead - 1) / 2;
        i = ahead;
        if (fabs(v) <= err[p] && !(err[p] == 0.0)) return -1;       // height = 0
        if (!(v >= 0.0)) continue;
        // insertion into the four largest (a later equal value goes behind: decided by the band test below, not by this order)
        int at = n < 4 ? n : 4;
        while (at > 0 && v > tv[at - 1]) --at;
        if (at >= 4) continue;
        for (int q = (n < 4 ? n : 3); q > at; --q) tv[q] = tv[q - 1], te[q] = te[q - 1], ti[q] = ti[q - 1];
        tv[at] = v, te[at] = err[p], ti[at] = p;
        if (n < 4) ++n;
    }
    if (n < 3) return 0;
    // the ranking: neighbours of the sorted four must be ordered for certain (equal values: numpy's argsort order is not a rule)
    for (int q = 0; q + 1 < n; ++q)
        if (tv[q] == tv[q + 1] || fabs(tv[q] - tv[q + 1]) <= te[q] + te[q + 1]) return -1;
    rows[0] = ti[0], rows[1] = ti[1], rows[2] = ti[2];
    return 3;
}

// ------------------------------------------------------------------ step 4: azimuth of one row
// |log a| against |log b| for magnitudes a, b > 0 known to +-band: -1, 0, +1, or 2 when not decided.  No logarithm: on the same
// side of 1 the magnitudes themselves order the values, on opposite sides their product against 1 does.
__host__ __device__ inline int sac_cmp_abslog(double a, double b, double band) {
    if (band > 0.0 && (fabs(a - 1.0) <= band || fabs(b - 1.0) <= band)) return 2;
    const bool ha = a >= 1.0, hb = b >= 1.0;
    if (ha == hb) {
        if (band > 0.0 && fabs(a - b) <= 2.0 * band) return 2;
        if (a == b) return 0;
        return ((a > b) == ha) ? 1 : -1;
    }
    const double p = a * b;
    if (band > 0.0 && fabs(p - 1.0) <= band * (a + b + band) + 4.0 * DBL_EPSILON * p) return 2;
    if (p == 1.0) return 0;
    return ((p > 1.0) == ha) ? 1 : -1;
}

// The line u[a] = |10 log10 m(a)|, a < n: index of the first maximum among its strict interior local maxima (plateau: middle
// sample), -1 for none, -2 when the answer is not certain or a magnitude is zero or not finite.  With band > 0 only the comparisons
// the answer depends on must be certain: the pick is a sample certainly above both neighbours, and every other sample that MAY be
// a local maximum (neither neighbour certainly above it) is certainly below the pick -- an undecided pair of small values
// elsewhere on the line cannot change the answer.
template <class Line> __host__ __device__ inline int sac_azimuth(const Line &m, int n, double band) {
    for (int a = 0; a < n; ++a) {
        const double v = m(a);
        if (!(v > 0.0 && v <= DBL_MAX)) return -2;
    }
    if (n < 3) return -1;
    if (band > 0.0) {
        int best = -1;
        for (int i = 1; i + 1 < n; ++i) {
            if (sac_cmp_abslog(m(i - 1), m(i), band) != -1 || sac_cmp_abslog(m(i + 1), m(i), band) != -1) continue;
            if (best >= 0) {
                const int c = sac_cmp_abslog(m(i), m(best), band);
                if (c == 2) return -2;
                if (c <= 0) continue;
            }
            best = i;
        }
        for (int i = 1; i + 1 < n; ++i) {
            if (i == best || sac_cmp_abslog(m(i - 1), m(i), band) == 1 || sac_cmp_abslog(m(i + 1), m(i), band) == 1) continue;
            if (best < 0 || sac_cmp_abslog(m(i), m(best), band) != -1) return -2;
        }
        return best;
    }
    int best = -1;
    const int last = n - 1;
    for (int i = 1; i < last; ++i) {
        const double v = m(i);
        const int c0 = sac_cmp_abslog(m(i - 1), v, band);
        if (c0 == 2) return -2;
        if (c0 >= 0) continue;
        int ahead = i + 1, c1 = 0;
        for (;;) {
            c1 = sac_cmp_abslog(m(ahead), v, band);
            if (c1 == 2) return -2;
            if (c1 != 0 || ahead >= last) break;
            ++ahead;
        }
        if (c1 >= 0) {          // not below: the run rises, or a plateau reaches the end of the line
            i = ahead - 1;
            continue;
        }
        const int p = (i + ahead - 1) / 2;
        i = ahead;
        if (best < 0) best = p;
        else {
            const int c = sac_cmp_abslog(v, m(best), band);
            if (c == 2) return -2;
            if (c > 0) best = p;
        }
    }
    return best;
}

struct SacLine {            // magnitudes kept in memory
    const double *p;
    long stride;
    __host__ __device__ double operator()(int i) const { return p[(long)i * stride]; }
};
struct SacImageLine {       // |img[r][a n_el]| of a complex64 image row, widened first
    const float2 *p;
    int n_el;
    __host__ __device__ double operator()(int i) const {
        const float2 v = p[(long)i * n_el];
        return hypot((double)v.x, (double)v.y);
    }
};

// ------------------------------------------------------------------ step 5: one phase step
// angle(z[e + 1]) - angle(z[e]) as np.diff(np.unwrap(.)) leaves it: steps of less than pi stay, the others are taken modulo 2 pi
// into [-pi, pi), and -pi becomes +pi when the raw step is positive.  *near: |raw step| lies within `band` of pi.
__host__ __device__ inline double sac_phase_step(double a0, double a1, double band, bool *near) {
    const double dd = a1 - a0;
    if (band > 0.0 && fabs(fabs(dd) - SAC_PI) <= band) *near = true;
    if (fabs(dd) < SAC_PI) return dd;
    double m = fmod(dd + SAC_PI, 2.0 * SAC_PI);
    if (m < 0.0) m += 2.0 * SAC_PI;         // numpy's mod has the sign of the divisor
    m -= SAC_PI;
    if (m == -SAC_PI && dd > 0.0) m = SAC_PI;
    return m;
}

// ------------------------------------------------------------------ step 6: the 2 x 3 pseudo-inverse
// D[3][2] -> pinv[2][3] by one one-sided Jacobi rotation (two columns: it converges in one), singular values below
// 3 eps sigma_max dropped (numpy's rcond=None: the minimum-norm solution).  Returns sigma_max / sigma_min (HUGE_VAL: rank deficient).
__host__ __device__ inline double sac_pinv(const double D[3][2], double pinv[2][3]) {
    double a[3] = {D[0][0], D[1][0], D[2][0]}, b[3] = {D[0][1], D[1][1], D[2][1]};
    const double al = a[0] * a[0] + a[1] * a[1] + a[2] * a[2], be = b[0] * b[0] + b[1] * b[1] + b[2] * b[2];
    const double ga = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
    double c = 1.0, s = 0.0;
    if (ga != 0.0) {
        const double zeta = (be - al) / (2.0 * ga);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        c = 1.0 / sqrt(1.0 + t * t);
        s = c * t;
    }
    double u[2][3], sig[2] = {0.0, 0.0};
    for (int i = 0; i < 3; ++i) {
        u[0][i] = c * a[i] - s * b[i];
        u[1][i] = s * a[i] + c * b[i];
    }
    const double V[2][2] = {{c, s}, {-s, c}};       // V[row][k]: column k belongs to u[k]
    for (int k = 0; k < 2; ++k) sig[k] = sqrt(u[k][0] * u[k][0] + u[k][1] * u[k][1] + u[k][2] * u[k][2]);
    const double smax = fmax(sig[0], sig[1]), smin = fmin(sig[0], sig[1]);
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 3; ++j) pinv[i][j] = 0.0;
    for (int k = 0; k < 2; ++k) {
        if (!(sig[k] > 3.0 * DBL_EPSILON * smax)) continue;
        const double inv = 1.0 / (sig[k] * sig[k]);
        for (int i = 0; i < 2; ++i)
            for (int j = 0; j < 3; ++j) pinv[i][j] += V[i][k] * u[k][j] * inv;
    }
    return smin > 3.0 * DBL_EPSILON * smax ? smax / smin : HUGE_VAL;
}

// hamming(E)[e] as np.hamming
__host__ __device__ inline double sac_hamming(int e, int E) { return E > 1 ? 0.54 - 0.46 * cos(2.0 * SAC_PI * e / (E - 1)) : 1.0; }

// Error bounds.  A float64 direct sum of S products errs by at most (S + 4) 2^-52 times the L1 norm of its terms;
// in dB of one element that is 20 / ln 10 times the relative error.
__host__ __device__ inline double sac_sum_eps(int S) { return (double)(S + 4) * 2.220446049250313e-16; }
// The float32 image against the host's float64 one, in units of 2^-24 times the L1 norm of the window:
//   (E + 4) + (S + 4) + 16   contraction over E (bf16 x 3 or float32 products, float32 accumulation), Hann, FFT over S: the count
//                            rd_error_ulps books for such a chain (4 per window product, n + 4 per direct sum, 4 log2 n <= n + 4
//                            per radix axis)
//   7                        the steering weights: a float32 Hamming table times v_sin_f32 / v_cos_f32 (or the polynomial) of a
//                            phase reduced in float64 -- 4e-7 of |W| <= 1, twice what mmw_beamform.h documents for them, and it
//                            enters every term of the sum, so it multiplies the same L1 norm
//   1                        the host's own image (float64 products, pocketfft): (E + S) 2^-52, far below one unit
__host__ __device__ inline double sac_image_eps(int S, int E) { return (double)((E + 4) + (S + 4) + 16 + 7 + 1) * 5.9604644775390625e-08; }

}  // namespace mmw
