// Batched RANSAC of the vehicle velocity estimator (mmw_vehicle_velocity_ransac, FramePipeline.vehicle_fits):
// point_cloud_processing/vehicle_vel_estimator.py's estimate_ego_vel for every frame of a resident [F][cap][4] point buffer.
//
//   k_vehicle_ransac<NW>   one workgroup of NW wavefronts per frame (a grid-stride loop over the frames).  H = p / |p| and y = v
//                          of the frame go to the LDS once; the static filter (an initial estimate given) compacts them in
//                          place, in order; the max_iters iterations are independent and are dealt to the wavefronts round
//                          robin, each one striding the points over its 64 lanes and joining the lanes' partial sums by a
//                          shuffle tree; every iteration leaves (error, band, subset fit, refit) in the LDS and the
//                          workgroup picks the smallest error, the lowest iteration among equals (the class's strict <).
//                          Batch launches use NW = 4.  A chained launch is ONE workgroup of NW = 16 that walks the frames in
//                          order and hands the last estimate it found to the next frame as its initial estimate.
//
// The class fits by inv(H^T H) (LAPACK), the kernel by the adjugate of the same dim x dim Gram matrix, and the two sum in
// different orders.  A decision that this difference could turn is not taken: the frame is FLAGGED (MMW_VEHICLE_FLAG_*), its row
// zeroed, and the caller lets the host class decide.  The bands are derived in DESIGN.md 4.25.  Nothing random and nothing
// transcendental runs here: the draws are a host-made table.  The solve, the bands, the reductions and the unit-row loader are
// mmw_lsq_core.h's, shared with the other estimators; the iteration loop is the class's own and lives here.
// This unit is compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "../../include/mmwgpu.h"
#include "mmw_lsq_core.h"

namespace mmw {

constexpr int VV_GRID_MAX = 2048;                   // workgroups of a batch launch; more frames are walked in further passes
constexpr int VV_WAVES_BATCH = 4, VV_WAVES_CHAIN = 16;
constexpr int VV_REC = 9;                           // doubles an iteration leaves: error, band, subset fit [3], refit [3], its band
constexpr int VV_RED = 11;                          // widest reduction
constexpr int VV_MISC = 16;                         // carried estimate [3], its presence, N, the wavefronts' flag words, its band

struct VvArgs {
    const double *points;        // [F][cap][4]
    const int32_t *counts;       // [F]
    const double *init;          // nullptr, [F][dim], or (chain) [1][dim]; a NaN in a row: no estimate
    const int32_t *draws;        // [n_tab][max_iters][ppf]: row N - ppf serves N points
    double *out;                 // [F][dim + 2]: ego velocity, mean squared error, points behind the static filter
    int32_t *status;             // [F]: 1 an estimate, 0 the class's empty array
    int32_t *flags;              // [F] MMW_VEHICLE_FLAG_* bits
    int F, cap, dim, ppf, max_iters, ncp, n_tab, chain;
    double fit_thr, static_thr;
};

inline size_t vehicle_lds_bytes(int cap, int max_iters) {
    return ((size_t)4 * (size_t)cap + (size_t)VV_REC * (size_t)max_iters + (size_t)VV_WAVES_CHAIN * VV_RED + VV_MISC) * sizeof(double);
}

#if defined(__HIPCC__)
__device__ __forceinline__ bool vv_drawn(const int32_t *dr, int ppf, int j) {
    bool in = false;
    for (int k = 0; k < ppf; ++k) in |= dr[k] == j;
    return in;
}

struct VvFrame {
    const double *hx, *hy, *hz, *ys;
    double thr;
    int ppf;
    // point j belongs to the refit of an iteration: drawn, or within the threshold of the drawn points' fit c
    __device__ __forceinline__ bool member(const int32_t *dr, const double *c, int j) const {
        if (vv_drawn(dr, ppf, j)) return true;
        const double r = lsq_residual(hx[j], hy[j], hz[j], ys[j], c);
        return r * r < thr;
    }
};

// grid min(F, VV_GRID_MAX) (chain: 1), NW * 64 threads, vehicle_lds_bytes(cap, max_iters) bytes of dynamic LDS
template <int NW> __global__ __launch_bounds__(NW * 64) void k_vehicle_ransac(VvArgs a) {
    extern __shared__ __attribute__((aligned(16))) char vv_smem[];
    const int cap = a.cap, dim = a.dim, ppf = a.ppf, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    double *hx = reinterpret_cast<double *>(vv_smem);             // [cap] each
    double *hy = hx + cap, *hz = hy + cap, *ys = hz + cap;
    double *rec = ys + cap;                                       // [max_iters][VV_REC]
    double *red = rec + (size_t)a.max_iters * VV_REC;             // [NW][VV_RED]
    double *misc = red + VV_WAVES_CHAIN * VV_RED;                 // [VV_MISC]
    int *wfl = reinterpret_cast<int *>(misc + 5);                 // [NW] <= 16 words
    const VvFrame fr{hx, hy, hz, ys, a.fit_thr, ppf};

    if (a.chain) {
        if (tid == 0) {
            bool has = a.init != nullptr;
            for (int k = 0; k < 3; ++k) {
                misc[k] = has && k < dim ? a.init[k] : 0.0;
                if (misc[k] != misc[k]) has = false;
            }
            misc[3] = has ? 1.0 : 0.0;
            misc[13] = 0.0;                                       // the seed is the caller's own value: no band
        }
        __syncthreads();
    }

    for (long f = blockIdx.x; f < a.F; f += gridDim.x) {
        int flags = 0;
        int N0 = a.counts[f];
        N0 = N0 < 0 ? 0 : (N0 > cap ? cap : N0);
        double ini[3] = {0.0, 0.0, 0.0};
        bool has_init = false;
        double ini_band = 0.0;                                    // how far the host chain's estimate may lie from the carried one
        if (a.chain) {
            has_init = misc[3] != 0.0;
            ini_band = misc[13];
            ini[0] = misc[0], ini[1] = misc[1], ini[2] = misc[2];
        } else if (a.init) {
            has_init = true;
            for (int k = 0; k < dim; ++k) {
                ini[k] = a.init[f * dim + k];
                if (ini[k] != ini[k]) has_init = false;
            }
        }
        if (has_init && !(lsq_abs1(ini) <= DBL_MAX)) flags |= MMW_VEHICLE_FLAG_NONFINITE;

        double ymax;                                              // H = p / |p|, y = v
        const double4 *p = reinterpret_cast<const double4 *>(a.points) + f * (long)cap;
        if (lsq_load_unit_rows<NW, LSQ_JOIN_IN_ORDER>(p, N0, dim, false, hx, hy, hz, ys, red, &ymax))
            flags |= MMW_VEHICLE_FLAG_NONFINITE;

        // the static filter: points whose speed the initial estimate explains, kept in order (one wavefront compacts in place);
        // a frame below num_close_pts points is empty before the filter is asked
        int N = N0;
        if (has_init && flags == 0 && N0 >= a.ncp) {
            if (wave == 0) {
                const double band_r = lsq_band_residual(ini_band, 1.0, ymax, lsq_abs1(ini));
                const double neg_ini[3] = {-ini[0], -ini[1], -ini[2]};   // the estimate is the vehicle's velocity, the fit its negative
                int cnt = 0;
                bool near = false;
                for (int base = 0; base < N0; base += 64) {
                    const int j = base + lane;
                    double x = 0.0, y = 0.0, z = 0.0, v = 0.0;
                    bool keep = false, nr = false;
                    if (j < N0) {
                        x = hx[j], y = hy[j], z = hz[j], v = ys[j];
                        const double r = lsq_residual(x, y, z, v, neg_ini);
                        const double e = r * r;
                        nr = fabs(e - a.static_thr) <= lsq_band_sq(r, band_r);
                        keep = e < a.static_thr;
                    }
                    int kept;
                    const int pos = cnt + lsq_wave_slot(keep, lane, &kept);
                    near = near || __ballot(nr) != 0ull;
                    lsq_wave_sync();       // every lane holds its point in registers before any lane stores (at or below its own slot)
                    if (keep) hx[pos] = x, hy[pos] = y, hz[pos] = z, ys[pos] = v;
                    lsq_wave_sync();
                    cnt += kept;
                }
                if (lane == 0) {
                    misc[4] = (double)cnt;
                    wfl[0] = near ? MMW_VEHICLE_FLAG_STATIC : 0;
                }
            }
            __syncthreads();
            N = (int)misc[4];
            flags |= wfl[0];
            __syncthreads();                                     // wfl is written again below
        }

        const bool fit = flags == 0 && N >= a.ncp;
        if (fit && (long)N - ppf >= a.n_tab) flags |= MMW_VEHICLE_FLAG_TABLES;
        int wf = 0;
        if (fit && flags == 0) {
            const int32_t *tab = a.draws + (long)(N - ppf) * a.max_iters * ppf;
            for (int it = wave; it < a.max_iters; it += NW) {       // no workgroup barrier inside: the wavefronts run apart
                const int32_t *dr = tab + (long)it * ppf;
                bool bad = false;
                for (int k = 0; k < ppf; ++k) {
                    const int i = dr[k];
                    bad |= (unsigned)i >= (unsigned)N;
                    for (int k2 = 0; k2 < k; ++k2) bad |= dr[k2] == i;
                }
                if (bad) {
                    wf |= MMW_VEHICLE_FLAG_TABLES;
                    break;
                }
                // the drawn points' fit: every lane computes the same sums
                double g[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0}, c[3], cond;
                for (int k = 0; k < ppf; ++k) lsq_gram_add(g, b, hx[dr[k]], hy[dr[k]], hz[dr[k]], ys[dr[k]]);
                lsq_gram_solve(dim, g, b, c, &cond);
                if (!(cond <= LSQ_COND_CAP)) {
                    wf |= MMW_VEHICLE_FLAG_COND;
                    break;
                }
                const double c1 = lsq_abs1(c);
                const double band_r = lsq_band_residual(lsq_band_coef(ppf, cond, ymax + c1), 1.0, ymax, c1);
                // the refit's members: count, residuals inside the band of the threshold, their Gram sums
                double s[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
                for (int j = lane; j < N; j += 64) {
                    const double x = hx[j], y = hy[j], z = hz[j], v = ys[j];
                    bool in = vv_drawn(dr, ppf, j);
                    if (!in) {
                        const double r = lsq_residual(x, y, z, v, c);
                        const double e = r * r;
                        if (fabs(e - a.fit_thr) <= lsq_band_sq(r, band_r)) s[1] += 1.0;
                        in = e < a.fit_thr;
                    }
                    if (in) {
                        s[0] += 1.0;
                        lsq_gram_add(s + 2, s + 8, x, y, z, v);
                    }
                }
                lsq_wave_reduce<11, LsqSum>(s);
                if (s[1] != 0.0) {
                    wf |= MMW_VEHICLE_FLAG_RESIDUAL;
                    break;
                }
                const int m = (int)s[0];
                double mse = __builtin_huge_val(), band = 0.0, band_c2 = 0.0, c2[3] = {0.0, 0.0, 0.0};
                if (m > a.ncp) {                                    // consensus: refit on every member, their mean squared error
                    double cond2;
                    lsq_gram_solve(dim, s + 2, s + 8, c2, &cond2);
                    if (!(cond2 <= LSQ_COND_CAP)) {
                        wf |= MMW_VEHICLE_FLAG_COND;
                        break;
                    }
                    const double c21 = lsq_abs1(c2);
                    band_c2 = lsq_band_coef(m, cond2, ymax + c21);
                    const double band_r2 = lsq_band_residual(band_c2, 1.0, ymax, c21);
                    double q[2] = {0.0, 0.0};                       // sum r^2, sum |r|
                    for (int j = lane; j < N; j += 64)
                        if (fr.member(dr, c, j)) {
                            const double r = lsq_residual(hx[j], hy[j], hz[j], ys[j], c2);
                            q[0] += r * r;
                            q[1] += fabs(r);
                        }
                    lsq_wave_reduce<2, LsqSum>(q);
                    mse = q[0] / m;
                    band = lsq_band_sum_sq(m, band_r2, q[1], q[0]) / m + 2.0 * LSQ_U * mse;
                }
                if (lane == 0) {
                    double *rc = rec + (size_t)it * VV_REC;
                    rc[0] = mse, rc[1] = band;
                    rc[2] = c[0], rc[3] = c[1], rc[4] = c[2];
                    rc[5] = c2[0], rc[6] = c2[1], rc[7] = c2[2];
                    rc[8] = band_c2;
                }
            }
        }
        if (lane == 0) wfl[wave] = wf;
        __syncthreads();
        for (int w = 0; w < NW; ++w) flags |= wfl[w];

        // the smallest error, the lowest iteration among equals; an error within the bands of it from other members: not decided
        int best = -1;
        double err = __builtin_huge_val();
        if (fit && flags == 0) {
            for (int it = 0; it < a.max_iters; ++it) {
                const double e = rec[(size_t)it * VV_REC];
                if (e < err) err = e, best = it;
            }
            if (best >= 0) {
                const int32_t *tab = a.draws + (long)(N - ppf) * a.max_iters * ppf;
                const double *rb = rec + (size_t)best * VV_REC;
                for (int it = 0; it < a.max_iters && flags == 0; ++it) {
                    const double *rc = rec + (size_t)it * VV_REC;
                    if (it == best || !(rc[0] <= DBL_MAX) || rc[0] - err > rc[1] + rb[1]) continue;
                    // the same error and refit to the last bit (equal member sets always are): either choice is this result
                    if (rc[0] == err && rc[5] == rb[5] && rc[6] == rb[6] && rc[7] == rb[7]) continue;
                    double df[1] = {0.0};
                    for (int j = tid; j < N; j += NW * 64)
                        if (fr.member(tab + (long)it * ppf, rc + 2, j) != fr.member(tab + (long)best * ppf, rb + 2, j)) df[0] += 1.0;
                    lsq_block_reduce<1, LsqSum, NW, LSQ_JOIN_IN_ORDER>(df, red);
                    if (df[0] != 0.0) flags |= MMW_VEHICLE_FLAG_ERROR_TIE;
                }
            }
        }

        const bool found = flags == 0 && best >= 0;
        if (tid == 0) {                                           // plain vector stores of one lane
            double *out = a.out + f * (dim + 2);
            for (int k = 0; k < dim; ++k) out[k] = found ? -rec[(size_t)best * VV_REC + 5 + k] : 0.0;
            out[dim] = found ? err : 0.0;
            out[dim + 1] = flags == 0 ? (double)N : 0.0;
            a.status[f] = found ? 1 : 0;
            a.flags[f] = flags;
        }
        __syncthreads();                                          // rec has been read: the carried estimate and the LDS may change
        if (a.chain) {
            if (flags != 0) {                                     // the chain ends here: the frames behind it are not reached
                for (long g = f + 1 + tid; g < a.F; g += NW * 64) {
                    for (int k = 0; k < dim + 2; ++k) a.out[g * (dim + 2) + k] = 0.0;
                    a.status[g] = 0;
                    a.flags[g] = MMW_VEHICLE_FLAG_CHAIN;
                }
                return;
            }
            if (found && tid == 0) {
                for (int k = 0; k < 3; ++k) misc[k] = k < dim ? -rec[(size_t)best * VV_REC + 5 + k] : 0.0;
                misc[3] = 1.0;
                misc[13] = rec[(size_t)best * VV_REC + 8];
            }
            __syncthreads();
        }
    }
}
#endif

}  // namespace mmw
