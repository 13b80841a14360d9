// Device point clouds and batched ego-velocity RANSAC (FramePipeline.point_clouds_device / ego_velocities).
//
//   k_point_cloud   one lane per detection slot: (range bin, Doppler bin, azimuth bin, elevation bin) -> float64 (x, y, z, v)
//                   from host-made float64 tables, in the product order of FramePipeline.point_clouds(): every product is one
//                   round-to-nearest multiply, so the buffer downloads to the host's values bit for bit.
//   k_ego_ransac    one workgroup per frame: scikit-learn's RANSACRegressor(LinearRegression(fit_intercept=False), min_samples=10,
//                   residual_threshold=thr, max_trials=20, random_state=42).fit on y = -v, H = p / |p|, followed by the refit on the
//                   best inlier set and its R^2.  The workgroup walks the trials in scikit-learn's order and stops where its loop
//                   stops (an integer lookup in a host-made table of _dynamic_max_trials).  Nothing random and nothing
//                   transcendental runs here: the 20 x 10 subset indices come from a host-made table.
//
// The fits are dim x dim normal equations (dim = 2, 3) solved by the adjugate; scikit-learn solves by SVD.  A frame whose
// decisions could differ from scikit-learn's by rounding is FLAGGED (EgoFlag) and recomputed by the caller; the band behind
// every flag is derived in DESIGN.md 4.14 and computed from the fit's own condition bound.  The trial loop, the solve, the bands
// and the reductions are mmw_lsq_core.h's, shared with the other estimators; this header holds the model, the refit and the flags.
// This unit is compiled with -ffp-contract=off: every product, sum and quotient is one round-to-nearest operation.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mmw_lsq_core.h"

namespace mmw {

constexpr int EGO_TRIALS = 20;            // max_trials
constexpr int EGO_MIN_SAMPLES = 10;       // min_samples

enum EgoFlag {
    EGO_FLAG_RESIDUAL = 1,     // a residual within the band of thr in a trial
    EGO_FLAG_SCORE_TIE = 2,    // equal inlier counts, scores within the band, different inlier sets
    EGO_FLAG_R2 = 4,           // the refit's R^2 within the band of r2_thr, or an R^2 whose denominator is not clearly non-zero
    EGO_FLAG_COND = 8,         // a subset / inlier Gram matrix beyond LSQ_COND_CAP (or not positive definite)
    EGO_FLAG_NONFINITE = 16,   // a non-finite H or y (a point at range 0)
    EGO_FLAG_TABLES = 32,      // the frame's table row does not serve its point count (caller error; nothing computed)
};

struct PointCloudArgs {
    const int32_t *dets, *counts;        // [F][cap][2] (range bin, Doppler bin), [F]
    const int32_t *az, *el;              // [F][cap] angle bins, or nullptr: angle 0
    const double *range_bins, *vel_bins; // [S], [C]
    const double *cos_a, *sin_a;         // [A]: np.cos / np.sin of angle_bins
    double *points;                      // [F][cap][4]; slots past the count are zeroed
    int cap, S, C, A;
};

__global__ __launch_bounds__(256) void k_point_cloud(PointCloudArgs a) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const long f = blockIdx.y;
    if (j >= a.cap) return;
    int n = a.counts[f];
    n = n < 0 ? 0 : (n > a.cap ? a.cap : n);
    double x = 0.0, y = 0.0, z = 0.0, v = 0.0;
    if (j < n) {
        const long s = f * (long)a.cap + j;
        int r = a.dets[2 * s], d = a.dets[2 * s + 1];
        r = (unsigned)r < (unsigned)a.S ? r : 0;
        d = (unsigned)d < (unsigned)a.C ? d : 0;
        double ca = 1.0, sa = 0.0, ce = 1.0, se = 0.0;          // cos(0), sin(0): a missing antenna list
        if (a.az) {
            int i = a.az[s];
            i = (unsigned)i < (unsigned)a.A ? i : 0;
            ca = a.cos_a[i];
            sa = a.sin_a[i];
        }
        if (a.el) {
            int i = a.el[s];
            i = (unsigned)i < (unsigned)a.A ? i : 0;
            ce = a.cos_a[i];
            se = a.sin_a[i];
        }
        const double rng = a.range_bins[r];
        const double rc = __dmul_rn(rng, ce);                    // rng * cos_el * cos(az): left to right
        x = __dmul_rn(rc, ca);
        y = __dmul_rn(rc, sa);
        z = __dmul_rn(rng, se);
        v = a.vel_bins[d];
    }
    double4 *out = reinterpret_cast<double4 *>(a.points) + (f * (long)a.cap + j);
    *out = make_double4(x, y, z, v);
}

struct EgoArgs {
    const double *points;        // [F][cap][4]
    const int32_t *counts;       // [F]
    const int32_t *subsets;      // [n_rows][EGO_TRIALS][EGO_MIN_SAMPLES]
    const int32_t *subset_row;   // [F]: the frame's row of subsets / trials_off (any value for N < EGO_MIN_SAMPLES)
    const int32_t *trials_tab;   // [tab_len]: row r holds min(20, _dynamic_max_trials(k, N)) for k = 0 .. N at trials_off[r]
    const int32_t *trials_off;   // [n_rows]
    double *out;                 // [F][dim + 2]: coefficients, R^2 of the refit on its inliers, inlier share
    int32_t *flags;              // [F] EgoFlag bits
    uint8_t *inlier_mask;        // nullptr, or [F][cap]
    int cap, dim, n_rows, tab_len;
    double thr, r2_thr;
};

// The workgroup's 256 threads as the group of lsq_ransac_trials: wavefront totals joined pairwise; red: [4][EGO_RED] doubles
struct EgoGroup {
    static constexpr int width = 256;
    int tid;
    double *red;
    template <int K, class Op, class Fn> __device__ void reduce(double (&tot)[K], Fn fn) const {
        fn(tid, tot);
        lsq_block_reduce<K, Op, 4, LSQ_JOIN_PAIRWISE>(tot, red);
    }
};

// The model of lsq_ransac_trials with dim = 2, 3 columns on the unit rows H (hmax = 1): c from the Gram sums, trusted while the
// Gram matrix's condition bound stays below LSQ_COND_CAP
struct EgoModel {
    const double *hx, *hy, *hz, *ys;
    int dim;
    double ymax, c[3], band_r;
    struct Sums {
        double g[6], b[3];
    };
    __device__ void add(Sums &s, int i) const { lsq_gram_add(s.g, s.b, hx[i], hy[i], hz[i], ys[i]); }
    // c holds a fit over n points whose Gram matrix is conditioned no worse than cond: its residual band, and whether to trust it
    __device__ bool trust(int n, double cond) {
        const double c1 = lsq_abs1(c);
        band_r = lsq_band_residual(lsq_band_coef(n, cond, ymax + c1), 1.0, ymax, c1);
        return cond <= LSQ_COND_CAP;
    }
    __device__ bool solve(const double *g, const double *b, int n) {
        double cond;
        lsq_gram_solve(dim, g, b, c, &cond);
        return trust(n, cond);
    }
    __device__ bool solve(const Sums &s, int n) { return solve(s.g, s.b, n); }
    __device__ double residual(int i) const { return fabs(lsq_residual(hx[i], hy[i], hz[i], ys[i], c)); }
};

__device__ __forceinline__ int ego_stop_flag(LsqStop stop) {
    return stop == LSQ_STOP_RESIDUAL ? EGO_FLAG_RESIDUAL : stop == LSQ_STOP_SCORE_TIE ? EGO_FLAG_SCORE_TIE
         : stop == LSQ_STOP_FIT ? EGO_FLAG_COND : stop == LSQ_STOP_TABLE ? EGO_FLAG_TABLES : 0;
}

__global__ __launch_bounds__(256) void k_ego_ransac(EgoArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int cap = a.cap, dim = a.dim, tid = threadIdx.x;
    double *hx = reinterpret_cast<double *>(smem);   // [cap] each
    double *hy = hx + cap, *hz = hy + cap, *ys = hz + cap;
    const EgoGroup w{tid, ys + cap};                 // red: [4][EGO_RED]
    const long f = blockIdx.x;
    int N = a.counts[f];
    N = N < 0 ? 0 : (N > cap ? cap : N);
    double *out = a.out + f * (dim + 2);
    uint8_t *mask = a.inlier_mask ? a.inlier_mask + f * (long)cap : nullptr;
    if (mask)
        for (int i = tid; i < cap; i += 256) mask[i] = 0;
    int flags = 0;
    double res[5] = {0.0, 0.0, 0.0, 0.0, 0.0};       // c[0..2], R^2, share

    if (N >= EGO_MIN_SAMPLES) {
        EgoModel best{hx, hy, hz, ys, dim, 0.0, {0.0, 0.0, 0.0}, 0.0};
        const double4 *p = reinterpret_cast<const double4 *>(a.points) + f * (long)cap;
        if (lsq_load_unit_rows<4, LSQ_JOIN_PAIRWISE>(p, N, dim, true, hx, hy, hz, ys, w.red, &best.ymax))   // y = -v
            flags |= EGO_FLAG_NONFINITE;
        const double ymax = best.ymax;
        const int row = a.subset_row[f];
        int off = 0;
        if ((unsigned)row >= (unsigned)a.n_rows) {
            flags |= EGO_FLAG_TABLES;
        } else {
            off = a.trials_off[row];
            if (off < 0 || (long)off + N + 1 > a.tab_len) flags |= EGO_FLAG_TABLES;
        }
        const int32_t *tab = a.trials_tab + off;
        const int32_t *sub = a.subsets + (long)(row < 0 ? 0 : row) * EGO_TRIALS * EGO_MIN_SAMPLES;

        bool found = false;
        if (flags == 0)
            flags |= ego_stop_flag(lsq_ransac_trials(w, N, a.thr, ymax, sub, EGO_MIN_SAMPLES, EGO_TRIALS, tab, &best, &found));

        if (flags == 0 && found) {
            // refit on the best trial's inliers (the same residual arithmetic gives the same mask)
            double s3[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // g[6], b[3], count, sum y
            w.reduce<12, LsqSum>(s3, [&](int rank, double *acc) {
                for (int i = rank; i < N; i += EgoGroup::width) {
                    const bool in = best.residual(i) <= a.thr;
                    if (mask) mask[i] = in ? 1 : 0;
                    if (in) {
                        lsq_gram_add(acc, acc + 6, hx[i], hy[i], hz[i], ys[i]);
                        acc[9] += 1.0;
                        acc[10] += ys[i];
                    }
                }
            });
            const int m = (int)s3[9];
            EgoModel fit = best;
            bool ok;
            if (m == 1) {                            // one equation: the minimum-norm solution h y / (h . h), as the SVD gives
                const double hh = s3[0] + s3[2] + s3[5];
                fit.c[0] = s3[6] / hh;
                fit.c[1] = s3[7] / hh;
                fit.c[2] = s3[8] / hh;
                ok = fit.trust(1, hh > 0.0 ? 1.0 : __builtin_huge_val());
            } else {
                ok = fit.solve(s3, s3 + 6, m);
            }
            if (!ok) {
                flags |= EGO_FLAG_COND;
            } else {
                res[0] = fit.c[0];
                res[1] = fit.c[1];
                res[2] = fit.c[2];
                res[4] = (double)m / (double)N;
                if (m > 3) {
                    const double ybar = s3[10] / m;
                    double s4[3] = {0, 0, 0};                       // sum r^2, sum |r|, sum (y - ybar)^2 over the inliers
                    w.reduce<3, LsqSum>(s4, [&](int rank, double *acc) {
                        for (int i = rank; i < N; i += EgoGroup::width)
                            if (best.residual(i) <= a.thr) {
                                const double r = fit.residual(i);
                                const double dv = ys[i] - ybar;
                                acc[0] += r * r;
                                acc[1] += r;
                                acc[2] += dv * dv;
                            }
                    });
                    double band;
                    bool loose;
                    res[3] = lsq_r2_of_sums(m, ymax, fit.band_r, s4[0], s4[1], s4[2], &band, &loose);
                    if (loose || fabs(res[3] - a.r2_thr) <= band) flags |= EGO_FLAG_R2;
                }
            }
        }
    }
    if (flags != 0) {
        res[0] = res[1] = res[2] = res[3] = res[4] = 0.0;
        if (mask) {
            __syncthreads();
            for (int i = tid; i < cap; i += 256) mask[i] = 0;
        }
    }
    if (tid == 0) {
        for (int k = 0; k < dim; ++k) out[k] = res[k];
        out[dim] = res[3];
        out[dim + 1] = res[4];
        a.flags[f] = flags;
    }
}

constexpr int EGO_RED = 12;                      // widest reduce of k_ego_ransac
inline size_t ego_lds_bytes(int cap) { return ((size_t)4 * cap + 4 * EGO_RED) * sizeof(double); }

}  // namespace mmw
