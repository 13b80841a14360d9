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
// transcendental runs here: the draws are a host-made table.  This unit is compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "../../include/mmwgpu.h"

namespace mmw {

constexpr double VV_COND_CAP = 1e6;                 // largest accepted bound tr(G)^dim / det(G) >= cond(G) of a Gram matrix
constexpr double VV_U = 1.1102230246251565e-16;     // 2^-53
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
struct VvSum {
    __device__ static double op(double a, double b) { return a + b; }
};
struct VvMax {
    __device__ static double op(double a, double b) { return a > b ? a : b; }
};

// every lane of the wavefront gets the K totals: lane partials joined by the halving tree, lane 0's result broadcast
template <int K> __device__ __forceinline__ void vv_wave_sum(double (&v)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double t = v[k];
        for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off);
        v[k] = __shfl(t, 0);
    }
}

// every thread of the NW wavefronts gets the K totals (lanes by the halving tree, then the wavefronts in order); red: [NW][K]
template <int K, typename Op, int NW> __device__ __forceinline__ void vv_block_reduce(double (&v)[K], double *red) {
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
        double t = red[k];
        for (int w = 1; w < NW; ++w) t = Op::op(t, red[w * K + k]);
        v[k] = t;
    }
}

// G c = b for the symmetric dim x dim G (g: xx, xy, yy, xz, yz, zz) by the adjugate; cond: tr(G)^dim / det(G) >= cond_2(G) for a
// positive definite G, +inf when det <= 0.
__device__ __forceinline__ void vv_solve(int dim, const double *g, const double *b, double *c, double *cond) {
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

__device__ __forceinline__ double vv_abs1(const double *c) { return fabs(c[0]) + fabs(c[1]) + fabs(c[2]); }

// band on the coefficients of a fit over n unit rows against the class's inv(H^T H) solve of the same points
__device__ __forceinline__ double vv_band_coef(int n, double cond, double scale) {
    return 8.0 * ((double)n + 8.0) * VV_U * cond * scale;
}

// band on a squared residual r * r whose residual is known to band_r
__device__ __forceinline__ double vv_band_sq(double r, double band_r) {
    return 2.0 * fabs(r) * band_r + band_r * band_r + 4.0 * VV_U * r * r;
}

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
        const double r = ys[j] - ((hx[j] * c[0] + hy[j] * c[1]) + hz[j] * c[2]);
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
        if (has_init && !(vv_abs1(ini) <= DBL_MAX)) flags |= MMW_VEHICLE_FLAG_NONFINITE;

        // H = p / |p| (the norm: sqrt of the left-to-right sum of squares, as np.linalg.norm(axis=1)), y = v
        double st[2] = {0.0, 0.0};                                // max |y|, non-finite entries
        const double4 *p = reinterpret_cast<const double4 *>(a.points) + f * (long)cap;
        for (int i = tid; i < N0; i += NW * 64) {
            const double4 q = p[i];
            double ss = q.x * q.x + q.y * q.y;
            if (dim == 3) ss = ss + q.z * q.z;
            const double nrm = __dsqrt_rn(ss);
            const double x = q.x / nrm, y = q.y / nrm, z = dim == 3 ? q.z / nrm : 0.0;
            hx[i] = x;
            hy[i] = y;
            hz[i] = z;
            ys[i] = q.w;
            const double s = fabs(x) + fabs(y) + fabs(z) + fabs(q.w);
            if (!(s <= DBL_MAX)) st[1] = 1.0;
            else if (fabs(q.w) > st[0]) st[0] = fabs(q.w);
        }
        vv_block_reduce<2, VvMax, NW>(st, red);
        const double ymax = st[0];
        if (st[1] != 0.0) flags |= MMW_VEHICLE_FLAG_NONFINITE;

        // the static filter: points whose speed the initial estimate explains, kept in order (one wavefront compacts in place);
        // a frame below num_close_pts points is empty before the filter is asked
        int N = N0;
        if (has_init && flags == 0 && N0 >= a.ncp) {
            if (wave == 0) {
                const double band_r = 8.0 * VV_U * (ymax + vv_abs1(ini)) + ini_band;
                int cnt = 0;
                bool near = false;
                for (int base = 0; base < N0; base += 64) {
                    const int j = base + lane;
                    double x = 0.0, y = 0.0, z = 0.0, v = 0.0;
                    bool keep = false, nr = false;
                    if (j < N0) {
                        x = hx[j], y = hy[j], z = hz[j], v = ys[j];
                        const double r = v - ((x * -ini[0] + y * -ini[1]) + z * -ini[2]);
                        const double e = r * r;
                        nr = fabs(e - a.static_thr) <= vv_band_sq(r, band_r);
                        keep = e < a.static_thr;
                    }
                    const unsigned long long kept = __ballot(keep);
                    const unsigned long long close = __ballot(nr);
                    near = near || close != 0ull;
                    // every lane holds its point in registers before any lane stores (a store's slot is at or below its own)
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    if (keep) {
                        const int pos = cnt + __popcll(kept & ((1ull << lane) - 1ull));
                        hx[pos] = x, hy[pos] = y, hz[pos] = z, ys[pos] = v;
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    cnt += __popcll(kept);
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
                for (int k = 0; k < ppf; ++k) {
                    const int i = dr[k];
                    const double x = hx[i], y = hy[i], z = hz[i], v = ys[i];
                    g[0] += x * x, g[1] += x * y, g[2] += y * y, g[3] += x * z, g[4] += y * z, g[5] += z * z;
                    b[0] += x * v, b[1] += y * v, b[2] += z * v;
                }
                vv_solve(dim, g, b, c, &cond);
                if (!(cond <= VV_COND_CAP)) {
                    wf |= MMW_VEHICLE_FLAG_COND;
                    break;
                }
                const double scale = ymax + vv_abs1(c);
                const double band_r = vv_band_coef(ppf, cond, scale) + 8.0 * VV_U * scale;
                // the refit's members: count, residuals inside the band of the threshold, their Gram sums
                double s[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
                for (int j = lane; j < N; j += 64) {
                    const double x = hx[j], y = hy[j], z = hz[j], v = ys[j];
                    bool in = vv_drawn(dr, ppf, j);
                    if (!in) {
                        const double r = v - ((x * c[0] + y * c[1]) + z * c[2]);
                        const double e = r * r;
                        if (fabs(e - a.fit_thr) <= vv_band_sq(r, band_r)) s[1] += 1.0;
                        in = e < a.fit_thr;
                    }
                    if (in) {
                        s[0] += 1.0;
                        s[2] += x * x, s[3] += x * y, s[4] += y * y, s[5] += x * z, s[6] += y * z, s[7] += z * z;
                        s[8] += x * v, s[9] += y * v, s[10] += z * v;
                    }
                }
                vv_wave_sum<11>(s);
                if (s[1] != 0.0) {
                    wf |= MMW_VEHICLE_FLAG_RESIDUAL;
                    break;
                }
                const int m = (int)s[0];
                double mse = __builtin_huge_val(), band = 0.0, band_c2 = 0.0, c2[3] = {0.0, 0.0, 0.0};
                if (m > a.ncp) {                                    // consensus: refit on every member, their mean squared error
                    double cond2;
                    vv_solve(dim, s + 2, s + 8, c2, &cond2);
                    if (!(cond2 <= VV_COND_CAP)) {
                        wf |= MMW_VEHICLE_FLAG_COND;
                        break;
                    }
                    const double scale2 = ymax + vv_abs1(c2);
                    band_c2 = vv_band_coef(m, cond2, scale2);
                    const double band_r2 = band_c2 + 8.0 * VV_U * scale2;
                    double q[2] = {0.0, 0.0};                       // sum r^2, sum |r|
                    for (int j = lane; j < N; j += 64)
                        if (fr.member(dr, c, j)) {
                            const double r = ys[j] - ((hx[j] * c2[0] + hy[j] * c2[1]) + hz[j] * c2[2]);
                            q[0] += r * r;
                            q[1] += fabs(r);
                        }
                    vv_wave_sum<2>(q);
                    mse = q[0] / m;
                    band = (2.0 * band_r2 * q[1] + m * band_r2 * band_r2 + (m + 4) * VV_U * q[0]) / m + 2.0 * VV_U * mse;
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
                    vv_block_reduce<1, VvSum, NW>(df, red);
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
