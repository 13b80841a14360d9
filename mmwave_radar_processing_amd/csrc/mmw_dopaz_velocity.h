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
// The trial loop, the bands and the wavefront reduction are mmw_lsq_core.h's, shared with the other estimators; this header holds
// the two waves, the one-column model, the peak list, the refit and the flags.
// This unit is compiled with -ffp-contract=off: every product and difference below is one round-to-nearest operation.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "../../include/mmwgpu.h"
#include "mmw_dopaz_codes.h"              // DZP_UNDECIDED
#include "mmw_lsq_core.h"

namespace mmw {

constexpr int DZV_TRIALS = 20;            // max_trials
constexpr int DZV_MIN_SAMPLES = 10;       // min_samples
constexpr int DZV_LANES = 64;

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

// The 64 lanes as a loop: fn(lane, acc) fills the lane's partials, the halving tree joins them in the order of the device's
// shuffle tree (lane l takes lane l + off for off = 32, 16, ... 1; lane 0 holds the total).
struct DzvWaveHost {
    static constexpr int width = DZV_LANES;
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
    static constexpr int width = DZV_LANES;
    int lane;
    template <int K, class Op, class Fn> __device__ void reduce(double (&tot)[K], Fn fn) const {
        fn(lane, tot);
        lsq_wave_reduce<K, Op>(tot);
    }
    template <class Keep, class Emit> __device__ int compact(int n, Keep keep, Emit emit) const {
        int cnt = 0;
        for (int base = 0; base < n; base += DZV_LANES) {
            const int r = base + lane;
            const bool k = r < n && keep(r);
            int kept;
            const int slot = lsq_wave_slot(k, lane, &kept);
            if (k) emit(r, cnt + slot);
            cnt += kept;
        }
        return cnt;
    }
    // the list's LDS stores of all lanes are complete and visible before any lane's loads behind this point
    __device__ void sync() const { lsq_wave_sync(); }
    template <class Fn> __device__ void lane0(Fn fn) const {
        if (lane == 0) fn();
    }
};
#endif

// The model of lsq_ransac_trials with one column h: c = sum(h y) / sum(h h) against an SVD solve of the same points
struct DzvModel {
    const double *hc, *ys;
    double ymax, hmax, c, band_c, band_r;
    struct Sums {
        double hy, hh, yy;
    };
    __host__ __device__ void add(Sums &s, int i) const {
        const double h = hc[i], y = ys[i];
        s.hy += h * y;
        s.hh += h * h;
        s.yy += y * y;
    }
    // c is 0 for h == 0 (the minimum-norm solution of the SVD solve); its band takes |c| and |y| / |h| in 2-norms (the condition
    // number of one column is 1); not trusted: a sum(h h) too small or too large
    __host__ __device__ bool solve(const Sums &s, int n) {
        c = s.hh == 0.0 ? 0.0 : s.hy / s.hh;
        band_c = lsq_band_coef(n, 1.0, fabs(c) + (s.hh > 0.0 ? sqrt(s.yy / s.hh) : 0.0));
        band_r = lsq_band_residual(band_c, hmax, ymax, fabs(c));
        return s.hh == 0.0 || (s.hh >= 1e-200 && s.hh <= 1e200);
    }
    __host__ __device__ double residual(int i) const { return fabs(ys[i] - hc[i] * c); }
};

__host__ __device__ inline int dzv_stop_flag(LsqStop stop) {
    return stop == LSQ_STOP_RESIDUAL ? MMW_DOPAZ_FLAG_RESIDUAL : stop == LSQ_STOP_SCORE_TIE ? MMW_DOPAZ_FLAG_SCORE_TIE
         : stop == LSQ_STOP_FIT ? MMW_DOPAZ_FLAG_NONFINITE : stop == LSQ_STOP_TABLE ? MMW_DOPAZ_FLAG_TABLES : 0;
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
        if (za == DZP_UNDECIDED || ze == DZP_UNDECIDED) flags |= MMW_DOPAZ_FLAG_UNDECIDED;
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
        w.template reduce<4, LsqMax>(st, [&](int lane, double *acc) {
            for (int r = lane; r < m; r += DZV_LANES) {
                if (rp[r] == DZP_UNDECIDED) acc[3] = 2.0;
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
            DzvModel best{hc, yc, ymax, hmax, 0.0, 0.0, 0.0};
            bool found;
            flags |= dzv_stop_flag(lsq_ransac_trials(w, N, thr, ymax, sub, DZV_MIN_SAMPLES, DZV_TRIALS, tab, &best, &found));

            if (flags == 0 && !found) status = MMW_DOPAZ_STATUS_FAILED;      // no accepted trial: the class's ValueError path
            if (flags == 0 && found) {
                // refit on the best trial's inliers (the same residual arithmetic gives the same mask)
                double s3[5] = {0.0, 0.0, 0.0, 0.0, 0.0};                      // sum hy, hh, yy, count, sum y
                w.template reduce<5, LsqSum>(s3, [&](int lane, double *acc) {
                    for (int j = lane; j < N; j += DZV_LANES)
                        if (best.residual(j) <= thr) {
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
                DzvModel fit = best;
                if (!fit.solve(DzvModel::Sums{s3[0], s3[1], s3[2]}, mi)) flags |= MMW_DOPAZ_FLAG_NONFINITE;
                const double c = fit.c;
                const double share = (double)mi / (double)N;
                if (fabs(share - a.share_thr) <= 4.0 * LSQ_U) flags |= MMW_DOPAZ_FLAG_SHARE;
                double r2 = 0.0;
                if (!standard && mi < 2) flags |= MMW_DOPAZ_FLAG_R2;             // model.score of one sample: nan
                else if (!standard || mi > 3) {
                    const double ybar = s3[4] / mi;
                    double s4[3] = {0.0, 0.0, 0.0};                             // sum r^2, sum |r|, sum (y - ybar)^2 over the inliers
                    w.template reduce<3, LsqSum>(s4, [&](int lane, double *acc) {
                        for (int j = lane; j < N; j += DZV_LANES)
                            if (best.residual(j) <= thr) {
                                const double r = fit.residual(j);
                                const double dv = yc[j] - ybar;
                                acc[0] += r * r;
                                acc[1] += r;
                                acc[2] += dv * dv;
                            }
                    });
                    double band;
                    bool loose;
                    r2 = lsq_r2_of_sums(mi, ymax, fit.band_r, s4[0], s4[1], s4[2], &band, &loose);
                    if ((loose && ymax != 0.0) || fabs(r2 - a.r2_thr) <= band) flags |= MMW_DOPAZ_FLAG_R2;
                }
                double vy = c;
                if (!standard) {
                    if (ymax != 0.0 && fabs(c) <= fit.band_c) flags |= MMW_DOPAZ_FLAG_A_ZERO;   // y == 0 throughout: a is 0 there as here
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
