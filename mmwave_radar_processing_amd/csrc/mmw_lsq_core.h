// Least squares and RANSAC shared by the three device velocity estimators (mmw_egovel.h, mmw_dopaz_velocity.h,
// mmw_vehicle_vel.h): the rounding bands of DESIGN.md 4.14, each written once, the reductions that fix the summation order,
// the unit-row loader, and scikit-learn's RANSACRegressor trial loop as one template over a group and a model.
//
// Include this header ONLY from translation units built with -ffp-contract=off (Makefile): every product, sum and quotient below
// is meant as one round-to-nearest operation, in the kernels as in the host-only entry, and the bands count them that way.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

namespace mmw {

constexpr double LSQ_U = 1.1102230246251565e-16;   // 2^-53, the rounding unit of float64
constexpr double LSQ_COND_CAP = 1e6;               // largest accepted bound tr(G)^dim / det(G) >= cond(G) of a Gram matrix

struct LsqSum {
    __host__ __device__ static double op(double a, double b) { return a + b; }
};
struct LsqMax {
    __host__ __device__ static double op(double a, double b) { return a > b ? a : b; }
};

// one unit row (x, y, z) with its value v joins the Gram sums g (xx, xy, yy, xz, yz, zz) and b = H^T y
__host__ __device__ inline void lsq_gram_add(double *g, double *b, double x, double y, double z, double v) {
    g[0] += x * x, g[1] += x * y, g[2] += y * y, g[3] += x * z, g[4] += y * z, g[5] += z * z;
    b[0] += x * v, b[1] += y * v, b[2] += z * v;
}

// G c = b for the symmetric dim x dim G (g: xx, xy, yy, xz, yz, zz) by the adjugate; cond: tr(G)^dim / det(G) >= cond_2(G) for a
// positive definite G, +inf when det <= 0.
__host__ __device__ inline void lsq_gram_solve(int dim, const double *g, const double *b, double *c, double *cond) {
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

__host__ __device__ inline double lsq_abs1(const double *c) { return fabs(c[0]) + fabs(c[1]) + fabs(c[2]); }

// v - H c of one unit row
__host__ __device__ inline double lsq_residual(double x, double y, double z, double v, const double *c) {
    return v - ((x * c[0] + y * c[1]) + z * c[2]);
}

// band on the coefficients of a fit over n points (2-norm of the difference to the host's SVD / inv(H^T H) solve of the same
// points); cond: the Gram matrix's condition bound, scale: |y| / |h| + |c|
__host__ __device__ inline double lsq_band_coef(int n, double cond, double scale) {
    return 8.0 * ((double)n + 8.0) * LSQ_U * cond * scale;
}

// band on a residual from the band of its coefficients: hmax = max |h| (1 for unit rows)
__host__ __device__ inline double lsq_band_residual(double band_c, double hmax, double ymax, double c1) {
    return hmax * band_c + 8.0 * LSQ_U * (ymax + hmax * c1);
}

// band on a squared residual r * r whose residual is known to band_r
__host__ __device__ inline double lsq_band_sq(double r, double band_r) {
    return 2.0 * fabs(r) * band_r + band_r * band_r + 4.0 * LSQ_U * r * r;
}

// the same for the sum of m of them, summed in any order: sr = sum |r|, sr2 = sum r^2
__host__ __device__ inline double lsq_band_sum_sq(int m, double band_r, double sr, double sr2) {
    return 2.0 * band_r * sr + m * band_r * band_r + (m + 4) * LSQ_U * sr2;
}

// R^2 = 1 - a / b with r2_score's conventions (a == 0: 1; b == 0: 0) and its band from the bands of a and b;
// *loose: the denominator is not clearly non-zero
__host__ __device__ inline double lsq_r2(double a, double b, double da, double db, double *band, bool *loose) {
    *loose = !(b > 4.0 * db);
    *band = 0.0;
    if (a == 0.0) return 1.0;
    if (b == 0.0) return 0.0;
    *band = 2.0 * (da + (a / b) * db) / b;
    return 1.0 - a / b;
}

// R^2 of m points from sr2 = sum r^2, sr = sum |r| (residuals known to band_r) and syy = sum (y - ybar)^2 (|y| <= ymax)
__host__ __device__ inline double lsq_r2_of_sums(int m, double ymax, double band_r, double sr2, double sr, double syy, double *band,
                                                 bool *loose) {
    const double e = 2.0 * (m + 4) * LSQ_U * ymax;
    const double db = 2.0 * e * sqrt(m * syy) + m * e * e + (m + 4) * LSQ_U * syy;
    return lsq_r2(sr2, syy, lsq_band_sum_sq(m, band_r, sr, sr2), db, band, loose);
}

// Why RANSACRegressor's loop stopped without a decision the host is sure to share; every caller has flag bits of its own for these.
enum LsqStop {
    LSQ_DECIDED = 0,
    LSQ_STOP_RESIDUAL,     // a residual within the band of the threshold
    LSQ_STOP_SCORE_TIE,    // equal inlier counts, scores within their bands, different inlier sets
    LSQ_STOP_FIT,          // a subset's fit the model does not trust
    LSQ_STOP_TABLE,        // a subset index that is no point of the list
};

// scikit-learn's RANSACRegressor(LinearRegression(fit_intercept=False), min_samples, max_trials).fit on points 0 .. N - 1, up to
// the choice of the best trial (the refit on its inliers is the caller's).
//   Group   width lanes that walk the points together: reduce<K, Op>(tot, fn) calls fn(rank, acc) for every rank < width -- fn
//           strides by width -- and gives every lane the K totals.  Every branch below is taken by the whole group.
//   Model   Sums, add(sums, i): point i joins a subset's sums; solve(sums, n): coefficients and the residual band band_r of a fit
//           over n points, false when the fit is not to be trusted; residual(i): |y - H c| of point i; ys: the values y.  A copy
//           is a fit.
//   sub     [max_trials][min_samples] subset indices; tab[k]: min(max_trials, _dynamic_max_trials(k inliers of N))
// *best is the winning trial's fit when *found; neither means anything behind a stop.
template <class Group, class Model>
__host__ __device__ inline LsqStop lsq_ransac_trials(const Group &w, int N, double thr, double ymax, const int32_t *sub, int min_samples,
                                                     int max_trials, const int32_t *tab, Model *best, bool *found) {
    Model m = *best;
    int n_trials = 0, n_best = 1;
    double score_best = -__builtin_huge_val(), band_best = 0.0;
    *found = false;
    while (n_trials < max_trials) {
        const int32_t *idx = sub + (long)(n_trials++) * min_samples;
        // the subset's fit: every lane computes the same sums
        typename Model::Sums sums{};
        for (int k = 0; k < min_samples; ++k) {
            if ((unsigned)idx[k] >= (unsigned)N) return LSQ_STOP_TABLE;
            m.add(sums, idx[k]);
        }
        if (!m.solve(sums, min_samples)) return LSQ_STOP_FIT;
        // residuals of all points: inlier count, sum of y, of r^2 and of |r| over the inliers, residuals inside the band
        double s1[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        w.template reduce<5, LsqSum>(s1, [&](int rank, double *acc) {
            for (int j = rank; j < N; j += Group::width) {
                const double r = m.residual(j);
                if (fabs(r - thr) <= m.band_r) acc[4] += 1.0;
                if (r <= thr) {
                    acc[0] += 1.0;
                    acc[1] += m.ys[j];
                    acc[2] += r * r;
                    acc[3] += r;
                }
            }
        });
        if (s1[4] != 0.0) return LSQ_STOP_RESIDUAL;
        const int mi = (int)s1[0];
        if (mi < n_best) continue;                       // fewer inliers: skipped before it is scored
        double score = __builtin_nan(""), band_s = 0.0;
        if (mi >= 2) {                                   // r2_score of fewer than two samples is nan
            const double ybar = s1[1] / mi;
            double s2[1] = {0.0};
            w.template reduce<1, LsqSum>(s2, [&](int rank, double *acc) {
                for (int j = rank; j < N; j += Group::width)
                    if (m.residual(j) <= thr) {
                        const double dv = m.ys[j] - ybar;
                        acc[0] += dv * dv;
                    }
            });
            bool loose;
            score = lsq_r2_of_sums(mi, ymax, m.band_r, s1[2], s1[3], s2[0], &band_s, &loose);
            if (loose) band_s = __builtin_huge_val();
        }
        if (mi == n_best && *found && fabs(score - score_best) <= band_s + band_best) {
            // tied within rounding: immaterial when both trials select the same inliers (the refit sees the same points)
            double df[1] = {0.0};
            w.template reduce<1, LsqSum>(df, [&](int rank, double *acc) {
                for (int j = rank; j < N; j += Group::width)
                    if ((m.residual(j) <= thr) != (best->residual(j) <= thr)) acc[0] += 1.0;
            });
            if (df[0] != 0.0) return LSQ_STOP_SCORE_TIE;
            continue;
        }
        if (mi == n_best && score < score_best) continue;
        n_best = mi;
        score_best = score;
        band_best = band_s;
        *best = m;
        *found = true;
        const int dyn = tab[mi];
        max_trials = dyn < max_trials ? dyn : max_trials;
    }
    return LSQ_DECIDED;
}

#if defined(__HIPCC__)
// every lane of the wavefront gets the K totals: lane partials joined by the halving tree, lane 0's result broadcast
template <int K, class Op> __device__ __forceinline__ void lsq_wave_reduce(double (&v)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double t = v[k];
        for (int off = 32; off > 0; off >>= 1) t = Op::op(t, __shfl_down(t, off));
        v[k] = __shfl(t, 0);
    }
}

// A float64 sum depends on the order its terms are joined in, and each kernel's order is part of its recorded results: the
// ego-velocity kernel joins its wavefront totals as a tree, (r0 + r1) + (r2 + r3), the vehicle kernel one after the other.
enum LsqJoin { LSQ_JOIN_PAIRWISE, LSQ_JOIN_IN_ORDER };

// every thread of the NW wavefronts gets the K totals (lanes by the halving tree, then the wavefronts as JOIN says); red: [NW][K]
template <int K, class Op, int NW, LsqJoin JOIN> __device__ __forceinline__ void lsq_block_reduce(double (&v)[K], double *red) {
#pragma unroll
    for (int k = 0; k < K; ++k)
        for (int off = 32; off > 0; off >>= 1) v[k] = Op::op(v[k], __shfl_down(v[k], off));
    const int wave = threadIdx.x >> 6;
    __syncthreads();                                             // the previous totals have been read
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < K; ++k) red[wave * K + k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double t[NW];
        t[0] = red[k];
        if (JOIN == LSQ_JOIN_IN_ORDER) {
            for (int w = 1; w < NW; ++w) t[0] = Op::op(t[0], red[w * K + k]);
        } else {
            for (int w = 1; w < NW; ++w) t[w] = red[w * K + k];
            for (int s = 1; s < NW; s <<= 1)
                for (int w = 0; w + s < NW; w += 2 * s) t[w] = Op::op(t[w], t[w + s]);
        }
        v[k] = t[0];
    }
}

// the LDS stores of all lanes of the wavefront are complete and visible before any lane's loads behind this point
__device__ __forceinline__ void lsq_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the slot of a keeping lane among the wavefront's keeping lanes, in lane order; *kept: their number
__device__ __forceinline__ int lsq_wave_slot(bool keep, int lane, int *kept) {
    const unsigned long long mask = __ballot(keep);
    *kept = __popcll(mask);
    return __popcll(mask & ((1ull << lane) - 1ull));
}

// H = p / |p| (the norm: sqrt of the left-to-right sum of squares, as np.linalg.norm(axis=1)) and y = v or -v of a frame's N
// points (x, y, z, v), by the NW * 64 threads of the workgroup; *ymax: max |y|.  Returns whether an entry is not finite.
template <int NW, LsqJoin JOIN>
__device__ __forceinline__ bool lsq_load_unit_rows(const double4 *p, int N, int dim, bool negate, double *hx, double *hy, double *hz,
                                                   double *ys, double *red, double *ymax) {
    double st[2] = {0.0, 0.0};                                   // max |y|, non-finite entries
    for (int i = threadIdx.x; i < N; i += NW * 64) {
        const double4 q = p[i];
        double ss = q.x * q.x + q.y * q.y;
        if (dim == 3) ss = ss + q.z * q.z;
        const double nrm = __dsqrt_rn(ss);
        const double x = q.x / nrm, y = q.y / nrm, z = dim == 3 ? q.z / nrm : 0.0, v = negate ? -q.w : q.w;
        hx[i] = x;
        hy[i] = y;
        hz[i] = z;
        ys[i] = v;
        const double s = fabs(x) + fabs(y) + fabs(z) + fabs(v);
        if (!(s <= DBL_MAX)) st[1] = 1.0;
        else if (fabs(v) > st[0]) st[0] = fabs(v);
    }
    lsq_block_reduce<2, LsqMax, NW, JOIN>(st, red);
    *ymax = st[0];
    return st[1] != 0.0;
}
#endif

}  // namespace mmw
