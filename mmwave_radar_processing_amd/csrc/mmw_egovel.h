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
// every flag is derived in DESIGN.md 4.14 and computed here from the fit's own condition bound.
// This unit is compiled with -ffp-contract=off, and the arithmetic that must equal the host's uses explicit _rn intrinsics.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mmw {

constexpr int EGO_TRIALS = 20;            // max_trials
constexpr int EGO_MIN_SAMPLES = 10;       // min_samples
constexpr double EGO_COND_CAP = 1e6;      // largest accepted bound tr(G)^dim / det(G) >= cond(G) of a Gram matrix
constexpr double EGO_U = 1.1102230246251565e-16;   // 2^-53

enum EgoFlag {
    EGO_FLAG_RESIDUAL = 1,     // a residual within the band of thr in a trial
    EGO_FLAG_SCORE_TIE = 2,    // equal inlier counts, scores within the band, different inlier sets
    EGO_FLAG_R2 = 4,           // the refit's R^2 within the band of r2_thr, or an R^2 whose denominator is not clearly non-zero
    EGO_FLAG_COND = 8,         // a subset / inlier Gram matrix beyond EGO_COND_CAP (or not positive definite)
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

struct EgoSum {
    __device__ static double op(double a, double b) { return __dadd_rn(a, b); }
};
struct EgoMax {
    __device__ static double op(double a, double b) { return a > b ? a : b; }
};

// every thread of the 256 gets the same K totals (fixed order: lanes by shuffle tree, then waves 0..3); red: [4][K] doubles
template <int K, typename Op> __device__ __forceinline__ void ego_reduce(double (&v)[K], double *red) {
#pragma unroll
    for (int k = 0; k < K; ++k)
        for (int off = 32; off > 0; off >>= 1) v[k] = Op::op(v[k], __shfl_down(v[k], off));
    const int wave = threadIdx.x >> 6;
    __syncthreads();                                             // the previous totals have been read
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < K; ++k) red[wave * K + k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = Op::op(Op::op(red[k], red[K + k]), Op::op(red[2 * K + k], red[3 * K + k]));
}

// G c = b for the symmetric dim x dim G (g: xx, xy, yy, xz, yz, zz) by the adjugate; cond: tr(G)^dim / det(G) >= cond_2(G)
// for a positive definite G, +inf when det <= 0.
__device__ __forceinline__ void ego_solve(int dim, const double *g, const double *b, double *c, double *cond) {
    double det, tr;
    if (dim == 2) {
        det = g[0] * g[2] - g[1] * g[1];
        tr = g[0] + g[2];
        c[0] = (g[2] * b[0] - g[1] * b[1]) / det;
        c[1] = (g[0] * b[1] - g[1] * b[0]) / det;
        c[2] = 0.0;
        *cond = tr * tr / det;
    } else {
        const double a00 = g[2] * g[5] - g[4] * g[4], a01 = g[3] * g[4] - g[1] * g[5], a02 = g[1] * g[4] - g[3] * g[2];
        const double a11 = g[0] * g[5] - g[3] * g[3], a12 = g[1] * g[3] - g[0] * g[4], a22 = g[0] * g[2] - g[1] * g[1];
        det = g[0] * a00 + g[1] * a01 + g[3] * a02;
        tr = g[0] + g[2] + g[5];
        c[0] = (a00 * b[0] + a01 * b[1] + a02 * b[2]) / det;
        c[1] = (a01 * b[0] + a11 * b[1] + a12 * b[2]) / det;
        c[2] = (a02 * b[0] + a12 * b[1] + a22 * b[2]) / det;
        *cond = tr * tr * tr / det;
    }
    if (!(det > 0.0) || !(*cond == *cond)) *cond = __builtin_huge_val();
}

// band on a fit's coefficients (2-norm of the difference to scikit-learn's SVD solution) for n fitted points
__device__ __forceinline__ double ego_band_coef(int n, double cond, double ymax, const double *c) {
    return 8.0 * (n + 8) * EGO_U * cond * (ymax + fabs(c[0]) + fabs(c[1]) + fabs(c[2]));
}

__device__ __forceinline__ double ego_residual(const double *hx, const double *hy, const double *hz, const double *ys, int i,
                                               const double *c) {
    const double p = __dadd_rn(__dadd_rn(__dmul_rn(hx[i], c[0]), __dmul_rn(hy[i], c[1])), __dmul_rn(hz[i], c[2]));
    return fabs(__dadd_rn(ys[i], -p));
}

// R^2 = 1 - a / b with r2_score's conventions (a == 0: 1; b == 0: 0) and its band from the bands of a and b;
// *loose: the denominator is not clearly non-zero
__device__ __forceinline__ double ego_r2(double a, double b, double da, double db, double *band, bool *loose) {
    *loose = !(b > 4.0 * db);
    *band = 0.0;
    if (a == 0.0) return 1.0;
    if (b == 0.0) return 0.0;
    *band = 2.0 * (da + (a / b) * db) / b;
    return 1.0 - a / b;
}

__global__ __launch_bounds__(256) void k_ego_ransac(EgoArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int cap = a.cap, dim = a.dim, tid = threadIdx.x;
    double *hx = reinterpret_cast<double *>(smem);   // [cap] each
    double *hy = hx + cap, *hz = hy + cap, *ys = hz + cap;
    double *red = ys + cap;                          // [4][EGO_RED]
    const long f = blockIdx.x;
    int N = a.counts[f];
    N = N < 0 ? 0 : (N > cap ? cap : N);
    double *out = a.out + f * (dim + 2);
    uint8_t *mask = a.inlier_mask ? a.inlier_mask + f * (long)cap : nullptr;
    if (mask)
        for (int i = tid; i < cap; i += 256) mask[i] = 0;
    int flags = 0;
    double res[5] = {0.0, 0.0, 0.0, 0.0, 0.0};       // c[0..2], R^2, share
    bool found = false;
    double cb[3] = {0.0, 0.0, 0.0};

    if (N >= EGO_MIN_SAMPLES) {
        // y = -v, H = p / |p| (the norm: sqrt of the left-to-right sum of squares, as np.linalg.norm(axis=1))
        double st[2] = {0.0, 0.0};                   // max |y|, non-finite entries
        const double *p = a.points + f * (long)cap * 4;
        for (int i = tid; i < N; i += 256) {
            const double4 q = reinterpret_cast<const double4 *>(p)[i];
            double ss = __dadd_rn(__dmul_rn(q.x, q.x), __dmul_rn(q.y, q.y));
            if (dim == 3) ss = __dadd_rn(ss, __dmul_rn(q.z, q.z));
            const double nrm = __dsqrt_rn(ss);
            const double x = __ddiv_rn(q.x, nrm), y = __ddiv_rn(q.y, nrm), z = dim == 3 ? __ddiv_rn(q.z, nrm) : 0.0;
            const double yv = -q.w;
            hx[i] = x;
            hy[i] = y;
            hz[i] = z;
            ys[i] = yv;
            const double s = fabs(x) + fabs(y) + fabs(z) + fabs(yv);
            if (!(s <= 1.7976931348623157e308)) st[1] = 1.0;
            else if (fabs(yv) > st[0]) st[0] = fabs(yv);
        }
        ego_reduce<2, EgoMax>(st, red);
        const double ymax = st[0];
        if (st[1] != 0.0) flags |= EGO_FLAG_NONFINITE;
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

        int max_trials = EGO_TRIALS, n_trials = 0, n_best = 1;
        double score_best = -__builtin_huge_val(), band_best = 0.0;
        while (flags == 0 && n_trials < max_trials) {
            const int t = n_trials++;
            // the subset's fit: every thread computes the same 10-point sums
            double g[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0}, c[3], cond;
            for (int k = 0; k < EGO_MIN_SAMPLES; ++k) {
                const int i = sub[t * EGO_MIN_SAMPLES + k];
                if ((unsigned)i >= (unsigned)N) {
                    flags |= EGO_FLAG_TABLES;
                    break;
                }
                const double x = hx[i], y = hy[i], z = hz[i], yv = ys[i];
                g[0] += x * x;
                g[1] += x * y;
                g[2] += y * y;
                g[3] += x * z;
                g[4] += y * z;
                g[5] += z * z;
                b[0] += x * yv;
                b[1] += y * yv;
                b[2] += z * yv;
            }
            if (flags) break;
            ego_solve(dim, g, b, c, &cond);
            if (!(cond <= EGO_COND_CAP)) {
                flags |= EGO_FLAG_COND;
                break;
            }
            const double band_c = ego_band_coef(EGO_MIN_SAMPLES, cond, ymax, c);
            const double band_r = band_c + 8.0 * EGO_U * (ymax + fabs(c[0]) + fabs(c[1]) + fabs(c[2]));
            // residuals of all points: inlier count, sum of y, of r^2 and of |r| over the inliers, residuals inside the band
            double s1[5] = {0, 0, 0, 0, 0};
            for (int i = tid; i < N; i += 256) {
                const double r = ego_residual(hx, hy, hz, ys, i, c);
                if (fabs(r - a.thr) <= band_r) s1[4] += 1.0;
                if (r <= a.thr) {
                    s1[0] += 1.0;
                    s1[1] += ys[i];
                    s1[2] += r * r;
                    s1[3] += r;
                }
            }
            ego_reduce<5, EgoSum>(s1, red);
            if (s1[4] != 0.0) {
                flags |= EGO_FLAG_RESIDUAL;
                break;
            }
            const int m = (int)s1[0];
            if (m < n_best) continue;                // fewer inliers: skipped before it is scored
            double score = __builtin_nan(""), band_s = 0.0;
            if (m >= 2) {                            // r2_score of fewer than two samples is nan
                const double ybar = s1[1] / m;
                double s2[1] = {0.0};
                for (int i = tid; i < N; i += 256) {
                    const double r = ego_residual(hx, hy, hz, ys, i, c);
                    if (r <= a.thr) {
                        const double dv = ys[i] - ybar;
                        s2[0] += dv * dv;
                    }
                }
                ego_reduce<1, EgoSum>(s2, red);
                const double e = 2.0 * (m + 4) * EGO_U * ymax;
                const double da = 2.0 * band_r * s1[3] + m * band_r * band_r + (m + 4) * EGO_U * s1[2];
                const double db = 2.0 * e * sqrt(m * s2[0]) + m * e * e + (m + 4) * EGO_U * s2[0];
                bool loose;
                score = ego_r2(s1[2], s2[0], da, db, &band_s, &loose);
                if (loose) band_s = __builtin_huge_val();
            }
            if (m == n_best && found && fabs(score - score_best) <= band_s + band_best) {
                // tied within rounding: immaterial when both trials select the same inliers (the refit sees the same points)
                double df[1] = {0.0};
                for (int i = tid; i < N; i += 256)
                    if ((ego_residual(hx, hy, hz, ys, i, c) <= a.thr) != (ego_residual(hx, hy, hz, ys, i, cb) <= a.thr)) df[0] += 1.0;
                ego_reduce<1, EgoSum>(df, red);
                if (df[0] != 0.0) {
                    flags |= EGO_FLAG_SCORE_TIE;
                    break;
                }
                continue;
            }
            if (m == n_best && score < score_best) continue;
            n_best = m;
            score_best = score;
            band_best = band_s;
            cb[0] = c[0];
            cb[1] = c[1];
            cb[2] = c[2];
            found = true;
            const int dyn = tab[m];
            max_trials = dyn < max_trials ? dyn : max_trials;
        }

        if (flags == 0 && found) {
            // refit on the best trial's inliers (the same residual arithmetic gives the same mask)
            double s3[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // g[6], b[3], count, sum y
            for (int i = tid; i < N; i += 256) {
                const bool in = ego_residual(hx, hy, hz, ys, i, cb) <= a.thr;
                if (mask) mask[i] = in ? 1 : 0;
                if (in) {
                    const double x = hx[i], y = hy[i], z = hz[i], yv = ys[i];
                    s3[0] += x * x;
                    s3[1] += x * y;
                    s3[2] += y * y;
                    s3[3] += x * z;
                    s3[4] += y * z;
                    s3[5] += z * z;
                    s3[6] += x * yv;
                    s3[7] += y * yv;
                    s3[8] += z * yv;
                    s3[9] += 1.0;
                    s3[10] += yv;
                }
            }
            ego_reduce<12, EgoSum>(s3, red);
            const int m = (int)s3[9];
            double c[3], cond;
            if (m == 1) {                            // one equation: the minimum-norm solution h y / (h . h), as the SVD gives
                const double hh = s3[0] + s3[2] + s3[5];
                c[0] = s3[6] / hh;
                c[1] = s3[7] / hh;
                c[2] = s3[8] / hh;
                cond = hh > 0.0 ? 1.0 : __builtin_huge_val();
            } else {
                ego_solve(dim, s3, s3 + 6, c, &cond);
            }
            if (!(cond <= EGO_COND_CAP)) {
                flags |= EGO_FLAG_COND;
            } else {
                res[0] = c[0];
                res[1] = c[1];
                res[2] = c[2];
                res[4] = __ddiv_rn((double)m, (double)N);
                if (m > 3) {
                    const double band_c = ego_band_coef(m, cond, ymax, c);
                    const double band_r = band_c + 8.0 * EGO_U * (ymax + fabs(c[0]) + fabs(c[1]) + fabs(c[2]));
                    const double ybar = s3[10] / m;
                    double s4[3] = {0, 0, 0};                       // sum r^2, sum |r|, sum (y - ybar)^2 over the inliers
                    for (int i = tid; i < N; i += 256) {
                        if (ego_residual(hx, hy, hz, ys, i, cb) <= a.thr) {
                            const double r = ego_residual(hx, hy, hz, ys, i, c);
                            const double dv = ys[i] - ybar;
                            s4[0] += r * r;
                            s4[1] += r;
                            s4[2] += dv * dv;
                        }
                    }
                    ego_reduce<3, EgoSum>(s4, red);
                    const double e = 2.0 * (m + 4) * EGO_U * ymax;
                    const double da = 2.0 * band_r * s4[1] + m * band_r * band_r + (m + 4) * EGO_U * s4[0];
                    const double db = 2.0 * e * sqrt(m * s4[2]) + m * e * e + (m + 4) * EGO_U * s4[2];
                    double band;
                    bool loose;
                    res[3] = ego_r2(s4[0], s4[2], da, db, &band, &loose);
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

constexpr int EGO_RED = 12;                      // widest ego_reduce
inline size_t ego_lds_bytes(int cap) { return ((size_t)4 * cap + 4 * EGO_RED) * sizeof(double); }

}  // namespace mmw
