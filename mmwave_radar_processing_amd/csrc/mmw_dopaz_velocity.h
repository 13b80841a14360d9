// RANSAC regression of the Doppler-azimuth velocity estimator's peaks (mmw_doppler_azimuth_ransac): the third
// stage of the reference's ADC-cube ego-velocity loop (processors/velocity_estimator.py: estimate_ego_vx_velocity and
// lsq_fit_ego_vy_ransac), on the index tables mmw_doppler_azimuth_peaks leaves in HBM.
//
//   dzv_pair          the rule for one (group, frame), ONE __host__ __device__ implementation parameterised on how a "wave" of 64
//                     lanes is realised: DzvWaveDevice (ballot, prefix count, shuffle tree) in the kernel, DzvWaveHost (the 64
//                     lanes as a loop) in mmw_diag_doppler_azimuth_ransac_host.  Every sum is a lane-strided partial in index
//                     order followed by the same halving tree, so the two produce bit-identical rows and flags.
//   k_dopaz_ransac    one wavefront per (group, frame), four to a workgroup.  The ordered peak list (y, H) of a pair lives in the
//                     wave's own slice of the LDS, written once after the compaction and read by its own lanes only: the waves of
//                     a workgroup never meet, so there is no workgroup barrier, only a wavefront fence behind the list's stores.
//
// scikit-learn's RANSACRegressor(LinearRegression(fit_intercept=False), min_samples=10, max_trials=20, random_state=42) with one
// column: a fit is sum(h y) / sum(h h) here and an SVD solve there.  A decision that this difference could turn is not taken:
// the pair is FLAGGED (MMW_DOPAZ_FLAG_*), its row zeroed, and the caller lets scikit-learn decide.  The bands are derived in
// DESIGN.md 4.23.  Nothing random and nothing transcendental runs here: subsets, trial caps, cos, sin and the angles are tables.
// This unit is compiled with -ffp-contract=off: every product and difference below is one round-to-nearest operation.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "../../include/mmwgpu.h"

namespace mmw {

constexpr int DZV_TRIALS = 20;            // max_trials
constexpr int DZV_MIN_SAMPLES = 10;       // min_samples
constexpr int DZV_LANES = 64;
constexpr double DZV_U = 1.1102230246251565e-16;   // 2^-53
constexpr int DZV_PEAK_UNDECIDED = -2;    // mmw_dopaz_peaks.h: DZP_UNDECIDED

// offset of the trial caps of N points in the table: rows of N + 1 entries for N = 10, 11, ...
__host__ __device__ inline long dzv_trials_off(int N) {
    return ((long)N * (N + 1) - (long)DZV_MIN_SAMPLES * (DZV_MIN_SAMPLES + 1)) / 2;
}

struct DzvArgs {
    const int32_t *row_peak;     // [G][F][n_rows]
    const int32_t *zero;         // [G][F]
    const int32_t *m;            // [F] rows of each frame, or null: n_rows
    const double *vel;           // [n_rows], or [F][vel_stride]
    long vel_frame_stride;       // 0: one table for all frames
    const double *cos_t, *sin_t, *theta;   // [n_cols]
    const int32_t *subsets;      // [n_tab][DZV_TRIALS][DZV_MIN_SAMPLES]: row N - 10 serves N points
    const int32_t *trials;       // the trial caps of N points at dzv_trials_off(N)
    int G, F, n_rows, n_cols, n_tab, g_az, g_el, mode;
    double thr_standard, thr_small_vx, r2_thr, share_thr;
    double *out;                 // [G][F][4]
    int32_t *flags;              // [G][F]
};

struct DzvSum {
    __host__ __device__ static double op(double a, double b) { return a + b; }
};
struct DzvMax {
    __host__ __device__ static double op(double a, double b) { return a > b ? a : b; }
};

// The 64 lanes as a loop: fn(lane, acc) fills the lane's partials, the halving tree joins them in the order of the device's
// shuffle tree (lane l takes lane l + off for off = 32, 16, ... 1; lane 0 holds the total).
struct DzvWaveHost {
    template <int K, class Op, class Fn> void reduce(double (&tot)[K], Fn fn) const {
        double v[DZV_LANES][K];
        for (int l = 0; l < DZV_LANES; ++l) {
            for (int k = 0; k < K; ++k) v[l][k] = tot[k];
            fn(l, v[l]);
        }
        for (int off = DZV_LANES / 2; off > 0; off >>= 1)
            for (int l = 0; l < off; ++l)
                for (int k = 0; k < K; ++k) v[l][k] = Op::op(v[l][k], v[l + off][k]);
        for (int k = 0; k < K; ++k) tot[k] = v[0][k];
    }
    // rows r < n with keep(r), in row order: emit(r, position); returns their number
    template <class Keep, class Emit> int compact(int n, Keep keep, Emit emit) const {
        int cnt = 0;
        for (int r = 0; r < n; ++r)
            if (keep(r)) emit(r, cnt++);
        return cnt;
    }
    void sync() const {}
    template <class Fn> void lane0(Fn fn) const { fn(); }
};

#if defined(__HIPCC__)
struct DzvWaveDevice {
    int lane;
    template <int K, class Op, class Fn> __device__ void reduce(double (&tot)[K], Fn fn) const {
        fn(lane, tot);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double v = tot[k];
            for (int off = DZV_LANES / 2; off > 0; off >>= 1) v = Op::op(v, __shfl_down(v, off));
            tot[k] = __shfl(v, 0);
        }
    }
    template <class Keep, class Emit> __device__ int compact(int n, Keep keep, Emit emit) const {
        int cnt = 0;
        for (int base = 0; base < n; base += DZV_LANES) {
            const int r = base + lane;
            const bool k = r < n && keep(r);
            const unsigned long long mask = __ballot(k);
            if (k) emit(r, cnt + __popcll(mask & ((1ull << lane) - 1ull)));
            cnt += __popcll(mask);
        }
        return cnt;
    }
    // the list's LDS stores of all lanes are complete and visible before any lane's loads behind this point
    __device__ void sync() const {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    template <class Fn> __device__ void lane0(Fn fn) const {
        if (lane == 0) fn();
    }
};
#endif

// band on a single-column fit's coefficient against an SVD solve of the same n points: |c| and |y| / |h| in 2-norms
__host__ __device__ inline double dzv_band_coef(int n, double c, double syy, double shh) {
    return 8.0 * (n + 8) * DZV_U * (fabs(c) + (shh > 0.0 ? sqrt(syy / shh) : 0.0));
}

// R^2 = 1 - a / b with r2_score's conventions (a == 0: 1; b == 0: 0) and its band from the bands of a and b;
// *loose: the denominator is not clearly non-zero
__host__ __device__ inline double dzv_r2(double a, double b, double da, double db, double *band, bool *loose) {
    *loose = !(b > 4.0 * db);
    *band = 0.0;
    if (a == 0.0) return 1.0;
    if (b == 0.0) return 0.0;
    *band = 2.0 * (da + (a / b) * db) / b;
    return 1.0 - a / b;
}

// c = sum(h y) / sum(h h), or 0 for h == 0 (the minimum-norm solution of the SVD solve); *bad: a sum too small or too large
// to be trusted
__host__ __device__ inline double dzv_coef(double shy, double shh, bool *bad) {
    if (shh == 0.0) return 0.0;
    if (!(shh >= 1e-200 && shh <= 1e200)) *bad = true;
    return shy / shh;
}

// One (group, frame).  hc / yc: room for n_rows doubles each, the wave's own.  Every branch below is taken by the whole wave.
template <class Wave>
__host__ __device__ inline void dzv_pair(const Wave &w, const DzvArgs &a, int g, int f, double *hc, double *yc) {
    const long gf = (long)g * a.F + f;
    const int m = a.m ? a.m[f] : a.n_rows;
    const double *vel = a.vel + (long)f * a.vel_frame_stride;
    int flags = 0, status = MMW_DOPAZ_STATUS_OK, inliers = 0;
    double res[4] = {0.0, 0.0, 0.0, 0.0};            // vx, vy, R^2, share

    // vx: estimate_ego_vx_velocity on the zero-azimuth entries, in NumPy's operation order
    double vx = 0.0;
    {
        const int za = a.zero[(long)a.g_az * a.F + f];
        const int ze = a.g_el >= 0 ? a.zero[(long)a.g_el * a.F + f] : -1;
        if (za == DZV_PEAK_UNDECIDED || ze == DZV_PEAK_UNDECIDED) flags |= MMW_DOPAZ_FLAG_UNDECIDED;
        else if (za < -1 || ze < -1 || za >= m || ze >= m) flags |= MMW_DOPAZ_FLAG_TABLES;
        else if (za >= 0 && ze >= 0) vx = (-1.0 * (vel[za] + vel[ze])) / 2.0;
        else if (za >= 0) vx = -1.0 * vel[za];
        else if (ze >= 0) vx = -1.0 * vel[ze];
        if (!(fabs(vx) <= DBL_MAX)) flags |= MMW_DOPAZ_FLAG_NONFINITE;
    }
    res[0] = vx;
    const bool standard = vx >= MMW_DOPAZ_VX_BRANCH;
    const double thr = standard ? a.thr_standard : a.thr_small_vx;

    if (!(a.mode & MMW_DOPAZ_RANSAC_VX_ONLY) && flags == 0) {
        const int32_t *rp = a.row_peak + gf * a.n_rows;
        // the ordered peak list: y and H of the rows with an entry, in row order
        const int n_cols = a.n_cols;
        const int N = w.compact(
            m, [&](int r) { return rp[r] >= 0 && rp[r] < n_cols; },
            [&](int r, int pos) {
                const int c = rp[r];
                const double v = vel[r];
                if (standard) {
                    yc[pos] = (-1.0 * v) - (vx * a.cos_t[c]);
                    hc[pos] = a.sin_t[c];
                } else {
                    yc[pos] = a.theta[c];
                    hc[pos] = v - vx;
                }
            });
        w.sync();
        double st[4] = {0.0, 0.0, 0.0, 0.0};          // max |y|, max |h|, non-finite entries, entries that are no index
        w.template reduce<4, DzvMax>(st, [&](int lane, double *acc) {
            for (int r = lane; r < m; r += DZV_LANES) {
                if (rp[r] == DZV_PEAK_UNDECIDED) acc[3] = 2.0;
                else if (rp[r] < -1 || rp[r] >= n_cols) acc[3] = acc[3] > 1.0 ? acc[3] : 1.0;
            }
            for (int j = lane; j < N; j += DZV_LANES) {
                const double ay = fabs(yc[j]), ah = fabs(hc[j]);
                if (!(ay + ah <= DBL_MAX)) acc[2] = 1.0;
                else {
                    acc[0] = ay > acc[0] ? ay : acc[0];
                    acc[1] = ah > acc[1] ? ah : acc[1];
                }
            }
        });
        const double ymax = st[0], hmax = st[1];
        if (st[2] != 0.0) flags |= MMW_DOPAZ_FLAG_NONFINITE;
        if (st[3] == 2.0) flags |= MMW_DOPAZ_FLAG_UNDECIDED;
        else if (st[3] == 1.0) flags |= MMW_DOPAZ_FLAG_TABLES;
        if (N >= DZV_MIN_SAMPLES && N - DZV_MIN_SAMPLES >= a.n_tab) flags |= MMW_DOPAZ_FLAG_TABLES;

        if (N == 0) status = MMW_DOPAZ_STATUS_EMPTY;
        else if (N < DZV_MIN_SAMPLES) status = MMW_DOPAZ_STATUS_FAILED;
        else if (flags == 0) {
            const int32_t *sub = a.subsets + (long)(N - DZV_MIN_SAMPLES) * DZV_TRIALS * DZV_MIN_SAMPLES;
            const int32_t *tab = a.trials + dzv_trials_off(N);
            int max_trials = DZV_TRIALS, n_trials = 0, n_best = 1;
            double score_best = -HUGE_VAL, band_best = 0.0, cb = 0.0;
            bool found = false;
            while (flags == 0 && n_trials < max_trials) {
                const int t = n_trials++;
                // the subset's fit: every lane computes the same ten-point sums
                double shy = 0.0, shh = 0.0, syy = 0.0;
                for (int k = 0; k < DZV_MIN_SAMPLES; ++k) {
                    const int i = sub[t * DZV_MIN_SAMPLES + k];
                    if ((unsigned)i >= (unsigned)N) {
                        flags |= MMW_DOPAZ_FLAG_TABLES;
                        break;
                    }
                    const double h = hc[i], y = yc[i];
                    shy += h * y;
                    shh += h * h;
                    syy += y * y;
                }
                if (flags) break;
                bool bad = false;
                const double c = dzv_coef(shy, shh, &bad);
                if (bad) {
                    flags |= MMW_DOPAZ_FLAG_NONFINITE;
                    break;
                }
                const double band_c = dzv_band_coef(DZV_MIN_SAMPLES, c, syy, shh);
                const double band_r = hmax * band_c + 8.0 * DZV_U * (ymax + hmax * fabs(c));
                // residuals of all points: inlier count, sum of y, of r^2 and of |r| over the inliers, residuals inside the band
                double s1[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
                w.template reduce<5, DzvSum>(s1, [&](int lane, double *acc) {
                    for (int j = lane; j < N; j += DZV_LANES) {
                        const double r = fabs(yc[j] - hc[j] * c);
                        if (fabs(r - thr) <= band_r) acc[4] += 1.0;
                        if (r <= thr) {
                            acc[0] += 1.0;
                            acc[1] += yc[j];
                            acc[2] += r * r;
                            acc[3] += r;
                        }
                    }
                });
                if (s1[4] != 0.0) {
                    flags |= MMW_DOPAZ_FLAG_RESIDUAL;
                    break;
                }
                const int mi = (int)s1[0];
                if (mi < n_best) continue;               // fewer inliers: skipped before it is scored
                double score = NAN, band_s = 0.0;
                if (mi >= 2) {                           // r2_score of fewer than two samples is nan
                    const double ybar = s1[1] / mi;
                    double s2[1] = {0.0};
                    w.template reduce<1, DzvSum>(s2, [&](int lane, double *acc) {
                        for (int j = lane; j < N; j += DZV_LANES)
                            if (fabs(yc[j] - hc[j] * c) <= thr) {
                                const double dv = yc[j] - ybar;
                                acc[0] += dv * dv;
                            }
                    });
                    const double e = 2.0 * (mi + 4) * DZV_U * ymax;
                    const double da = 2.0 * band_r * s1[3] + mi * band_r * band_r + (mi + 4) * DZV_U * s1[2];
                    const double db = 2.0 * e * sqrt(mi * s2[0]) + mi * e * e + (mi + 4) * DZV_U * s2[0];
                    bool loose;
                    score = dzv_r2(s1[2], s2[0], da, db, &band_s, &loose);
                    if (loose) band_s = HUGE_VAL;
                }
                if (mi == n_best && found && fabs(score - score_best) <= band_s + band_best) {
                    // tied within rounding: immaterial when both trials select the same inliers (the refit sees the same points)
                    double df[1] = {0.0};
                    w.template reduce<1, DzvSum>(df, [&](int lane, double *acc) {
                        for (int j = lane; j < N; j += DZV_LANES)
                            if ((fabs(yc[j] - hc[j] * c) <= thr) != (fabs(yc[j] - hc[j] * cb) <= thr)) acc[0] += 1.0;
                    });
                    if (df[0] != 0.0) {
                        flags |= MMW_DOPAZ_FLAG_SCORE_TIE;
                        break;
                    }
                    continue;
                }
                if (mi == n_best && score < score_best) continue;
                n_best = mi;
                score_best = score;
                band_best = band_s;
                cb = c;
                found = true;
                const int dyn = tab[mi];
                max_trials = dyn < max_trials ? dyn : max_trials;
            }

            if (flags == 0 && !found) status = MMW_DOPAZ_STATUS_FAILED;      // no accepted trial: the class's ValueError path
            if (flags == 0 && found) {
                // refit on the best trial's inliers (the same residual arithmetic gives the same mask)
                double s3[5] = {0.0, 0.0, 0.0, 0.0, 0.0};                      // sum hy, hh, yy, count, sum y
                w.template reduce<5, DzvSum>(s3, [&](int lane, double *acc) {
                    for (int j = lane; j < N; j += DZV_LANES)
                        if (fabs(yc[j] - hc[j] * cb) <= thr) {
                            const double h = hc[j], y = yc[j];
                            acc[0] += h * y;
                            acc[1] += h * h;
                            acc[2] += y * y;
                            acc[3] += 1.0;
                            acc[4] += y;
                        }
                });
                const int mi = (int)s3[3];
                inliers = mi;
                bool bad = false;
                const double c = dzv_coef(s3[0], s3[1], &bad);
                if (bad) flags |= MMW_DOPAZ_FLAG_NONFINITE;
                const double band_c = dzv_band_coef(mi, c, s3[2], s3[1]);
                const double share = (double)mi / (double)N;
                if (fabs(share - a.share_thr) <= 4.0 * DZV_U) flags |= MMW_DOPAZ_FLAG_SHARE;
                double r2 = 0.0;
                if (!standard && mi < 2) flags |= MMW_DOPAZ_FLAG_R2;             // model.score of one sample: nan
                else if (!standard || mi > 3) {
                    const double band_r = hmax * band_c + 8.0 * DZV_U * (ymax + hmax * fabs(c));
                    const double ybar = s3[4] / mi;
                    double s4[3] = {0.0, 0.0, 0.0};                             // sum r^2, sum |r|, sum (y - ybar)^2 over the inliers
                    w.template reduce<3, DzvSum>(s4, [&](int lane, double *acc) {
                        for (int j = lane; j < N; j += DZV_LANES)
                            if (fabs(yc[j] - hc[j] * cb) <= thr) {
                                const double r = fabs(yc[j] - hc[j] * c);
                                const double dv = yc[j] - ybar;
                                acc[0] += r * r;
                                acc[1] += r;
                                acc[2] += dv * dv;
                            }
                    });
                    const double e = 2.0 * (mi + 4) * DZV_U * ymax;
                    const double da = 2.0 * band_r * s4[1] + mi * band_r * band_r + (mi + 4) * DZV_U * s4[0];
                    const double db = 2.0 * e * sqrt(mi * s4[2]) + mi * e * e + (mi + 4) * DZV_U * s4[2];
                    double band;
                    bool loose;
                    r2 = dzv_r2(s4[0], s4[2], da, db, &band, &loose);
                    if ((loose && ymax != 0.0) || fabs(r2 - a.r2_thr) <= band) flags |= MMW_DOPAZ_FLAG_R2;
                }
                double vy = c;
                if (!standard) {
                    if (ymax != 0.0 && fabs(c) <= band_c) flags |= MMW_DOPAZ_FLAG_A_ZERO;   // y == 0 throughout: a is 0 there as here
                    vy = c != 0.0 ? -1.0 / c : 0.0;
                }
                res[1] = vy;
                res[2] = r2;
                res[3] = share;
            }
        }
    }
    if (flags != 0) {
        res[0] = res[1] = res[2] = res[3] = 0.0;
        status = MMW_DOPAZ_STATUS_OK;
        inliers = 0;
    }
    w.lane0([&]() {                                                  // plain vector stores of one lane
        double *out = a.out + gf * 4;
        out[0] = res[0];
        out[1] = res[1];
        out[2] = res[2];
        out[3] = res[3];
        a.flags[gf] = flags | (status << MMW_DOPAZ_STATUS_SHIFT) | (inliers << MMW_DOPAZ_INLIERS_SHIFT);
    });
}

inline size_t dopaz_ransac_lds(int n_rows) { return (size_t)4 * 2 * (n_rows > 0 ? n_rows : 1) * sizeof(double); }

#if defined(__HIPCC__)
// grid ceil(G * F / 4), 256 threads, dopaz_ransac_lds(n_rows) bytes of dynamic LDS; wave w of block b fits pair 4 b + w.
__global__ __launch_bounds__(256) void k_dopaz_ransac(DzvArgs a) {
    extern __shared__ __attribute__((aligned(16))) char dzv_smem[];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long pair = (long)blockIdx.x * 4 + wave;
    if (pair >= (long)a.G * a.F) return;
    double *hc = reinterpret_cast<double *>(dzv_smem) + (long)wave * 2 * a.n_rows;
    const int g = (int)(pair / a.F), f = (int)(pair - (long)g * a.F);
    dzv_pair(DzvWaveDevice{(int)(threadIdx.x & 63)}, a, g, f, hc, hc + a.n_rows);
}
#endif

}  // namespace mmw
