// The per-detection angle FFT + argmax of the point cloud: the float32 form with its rounding-error bound and the float64
// refinement of what the bound cannot decide.  (mmw_tu_points.hip; mmw_detect.h and mmw_cells64.h build on it)
#pragma once
#include "mmw_ctx.h"

namespace mmw {

// np.argmax order on magnitudes: a NaN beats everything that is not a NaN, the FIRST maximum wins
template <typename T> __device__ __forceinline__ bool mag_gt(T a, T b) {
    if (a != a) return !(b != b);
    if (b != b) return false;
    return a > b;
}
template <typename T> __device__ __forceinline__ bool mag_better(T a, int ia, T b, int ib) {   // (a, ia) ahead of (b, ib)
    return mag_gt(a, b) || (!mag_gt(b, a) && ia < ib);
}

// Detections whose float32 argmax is not provably the float64 one are appended here and re-evaluated in float64.
struct ArgmaxRefine {
    const float *l1;        // [F][V] from k_plane_l1; nullptr: no refinement (plain float32 argmax)
    int *n_flag;            // number of flagged detections (may exceed list_cap)
    int *list;              // f * cap + det of the flagged detections
    int list_cap;
    float k_fft, k_ang;     // error-bound constants (see below)
    int *flagpos;           // optional [F][cap]: 1 + list position of a flagged detection (the dense refinement finds a frame's
    int dense_cap;          // flagged detections through it: mmw_cells64.h); positions from dense_cap on are not recorded
    int tag;                // ORed into the list entries (REFINE_SECOND: the second list of a call that refines two at once)
    int *n_tagged;          // optional: counts the flagged evaluations of a tagged list
};

// One wave per detection: gather rd[f][ant[i]][r][v], lane k evaluates angle bins k, k+64, ... of the
// zero-padded A-point DFT, first-max argmax over the (optionally fftshifted) response.
// (processors/point_cloud_generator.py:168-214; np.argmax returns the FIRST maximum.)
// The reference does this in complex128 on a complex128 range-Doppler cube.  Here the cube is float32, so the kernel also
// bounds how far its magnitudes can be from the float64 ones:
//   |rd32 - rd64| <= k_fft * l1(plane)   (each RD cell is a sum of S*C products w x W with <= log2(S) + log2(C) + 2
//                                          roundings on the way: (log2 S + log2 C + 2) eps sum|w x| <= 17 eps l1 for
//                                          256 x 128; k_fft = 32 eps leaves a factor ~2)
//   |m32[k] - m64[k]| <= B = sum_i k_fft l1_i + k_ang sum_i |x_i|   (n_ant-term float32 sum + hypotf)
// and flags the detection unless best - second > 2 B: the float64 argmax of an unflagged detection is the one found.
// NA: antennas held in registers (the list is padded to it): 4 / 8 / 16 / 32 -- the gathers are cold, strided 8-byte
// loads, so the kernel lives on the number of waves in flight, i.e. on a small register footprint.
// gather of one detection's cells: x[i] = rd[f][ants.idx[i]][r][v] (zero beyond the list), sum_abs = sum |re| + |im|
template <int NA>
__device__ __forceinline__ void argmax_gather(const float2 *rd, long f, int V, int S, int C, int r, int v, const AntList &ants,
                                              float2 (&x)[NA], float &sum_abs) {
    sum_abs = 0.f;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        // unconditional (entries of the list past n are antenna 0): a guarded load would be followed by its own wait
        x[i] = rd[((f * V + ants.idx[i]) * S + r) * C + v];
        if (i >= ants.n) x[i] = make_float2(0.f, 0.f);
        if (i < ants.n) sum_abs += fabsf(x[i].x) + fabsf(x[i].y);
    }
}

// one wave: zero-padded A-point DFT of the n cells, |.|, wave-wide FIRST maximum (wb at bin wi) and the largest
// magnitude among all other bins (ws2)
template <int NA>
__device__ __forceinline__ void argmax_eval(const float2 (&x)[NA], int n, int A, int shift, const float2 *twA, int lane,
                                            float &wb, int &wi, float &ws2, float &lane_re, float &lane_im, int &lane_idx) {
    const float NEG = -__builtin_huge_valf();
    float best = NEG, second = NEG;
    int best_idx = 0x7fffffff;
    lane_re = lane_im = 0.f;
    for (int k = lane; k < A; k += 64) {
        float re = 0.f, im = 0.f;
        int t = 0;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            if (i < n) {
                const float2 w = twA[t];
                re += x[i].x * w.x - x[i].y * w.y;
                im += x[i].x * w.y + x[i].y * w.x;
                t += k;
                if (t >= A) t -= A;
            }
        }
        const float m = hypotf(re, im);
        const int kk = shift ? (k + A / 2) % A : k;
        if (best_idx == 0x7fffffff || mag_better(m, kk, best, best_idx)) {
            if (best_idx != 0x7fffffff) second = best;
            best = m;
            best_idx = kk;
            lane_re = re;
            lane_im = im;
        } else if (mag_gt(m, second)) second = m;
    }
    lane_idx = best_idx;
    // wave-wide first maximum, then the largest magnitude among everything else
    wb = best;
    wi = best_idx;
    for (int d = 32; d >= 1; d >>= 1) {
        const float ob = __shfl_xor(wb, d, 64);
        const int oi = __shfl_xor(wi, d, 64);
        if (oi != 0x7fffffff && (wi == 0x7fffffff || mag_better(ob, oi, wb, wi))) {
            wb = ob;
            wi = oi;
        }
    }
    ws2 = (best_idx == wi) ? second : best;
    for (int d = 32; d >= 1; d >>= 1) {
        const float o = __shfl_xor(ws2, d, 64);
        if (mag_gt(o, ws2)) ws2 = o;
    }
}

// Second pass of the certainty test (lists of at most 8 antennas; same form as detect_argmax_list in mmw_detect.h): the
// errors of two bins of one detection are the SAME per-antenna cell errors e_i seen through two steering vectors, so
//   |(m1 - mk)_32 - (m1 - mk)_64| <= sum_i e_i |conj(u1) W^(i k1) - conj(uk) W^(i k)| + Be^2 / (2 min(m1, mk)) + 2 c_ang,
// far below the independent-errors 2 (Be + c_ang) for neighbouring bins.  Every bin other than the winner is tested;
// returns true when some bin is not provably below the winner.
template <int NA>
__device__ __forceinline__ bool argmax_pairwise(const float2 (&x)[NA], const float (&e)[NA], int A, int shift, const float2 *twA,
                                                int lane, int wi, float m1, float re1, float im1, float be, float c_ang) {
    const float inv1 = 1.f / m1, u1x = re1 * inv1, u1y = im1 * inv1, two_b = 2.f * (be + c_ang);
    const int k1 = shift ? (wi + A - A / 2) % A : wi;
    float2 t1[NA];                      // conj(u_1) W^(i k_1)
    {
        int t = 0;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const float2 w = twA[t];
            t1[i] = make_float2(u1x * w.x + u1y * w.y, u1x * w.y - u1y * w.x);
            t += k1;
            if (t >= A) t -= A;
        }
    }
    bool bad = false;
    for (int k = lane; k < A; k += 64) {
        const int kk = shift ? (k + A / 2) % A : k;
        if (kk == wi) continue;
        float2 w[NA];
        int t = 0;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            w[i] = twA[t];
            t += k;
            if (t >= A) t -= A;
        }
        float re = 0.f, im = 0.f;
#pragma unroll
        for (int i = 0; i < NA; ++i) {      // (cells past the list are zero: same sums as the first pass)
            re += x[i].x * w[i].x - x[i].y * w[i].y;
            im += x[i].x * w[i].y + x[i].y * w[i].x;
        }
        const float m = hypotf(re, im), margin = m1 - m;
        bool ok = margin > two_b;
        if (!ok && m > 0.f) {
            const float inv = 1.f / m, ux = re * inv, uy = im * inv;
            float lin = 0.f;
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const float dx = t1[i].x - (ux * w[i].x + uy * w[i].y), dy = t1[i].y - (ux * w[i].y - uy * w[i].x);
                lin += e[i] * __fsqrt_rn(fmaf(dx, dx, dy * dy));
            }
            ok = margin > 1.001f * (lin + be * be / (2.f * fminf(m1, m))) + 2.f * c_ang;
        }
        bad |= !ok;
    }
    return __ballot(bad) != 0ull;
}

template <int NA>
__global__ __launch_bounds__(256) void k_angle_argmax(const float2 *rd, const int32_t *dets, const int32_t *counts,
                                                       int32_t *out_idx, int V, int S, int C, int cap,
                                                       AntList ants, int A, int shift, const float2 *twA, ArgmaxRefine rf) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int f = blockIdx.y;
    int n_det = counts[f];
    if (n_det > cap) n_det = cap;
    constexpr bool PAIR = NA <= 8;      // longer lists keep the independent-errors test (more of them are refined)
    float sum_l1 = 0.f, e[PAIR ? NA : 1];
    if (rf.l1) {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const float l = i < ants.n ? rf.l1[(long)f * V + ants.idx[i]] : 0.f;
            sum_l1 += l;
            if constexpr (PAIR) e[i] = rf.k_fft * l;
        }
    }
    // grid.x covers the usual detection counts in one pass; a wave walks on for frames with more
    for (int det = blockIdx.x * 4 + wave; det < n_det; det += gridDim.x * 4) {
        const int r = dets[((long)f * cap + det) * 2], v = dets[((long)f * cap + det) * 2 + 1];
        float2 x[NA];
        float sum_abs, wb, ws2, lre, lim;
        int wi, lidx;
        argmax_gather<NA>(rd, f, V, S, C, r, v, ants, x, sum_abs);
        argmax_eval<NA>(x, ants.n, A, shift, twA, lane, wb, wi, ws2, lre, lim, lidx);
        bool flag = false;
        if (rf.l1) {
            const float be = rf.k_fft * sum_l1, c_ang = rf.k_ang * sum_abs;
            flag = !(wb - ws2 > 2.f * (be + c_ang));             // (also for NaN / inf magnitudes)
            if constexpr (PAIR) {
                if (flag && wb == wb && wb > 0.f && wb < __builtin_huge_valf()) {
                    const int l1 = __ffsll((long long)__ballot(lidx == wi)) - 1;
                    const float re1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, lre), l1));
                    const float im1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, lim), l1));
                    flag = argmax_pairwise<NA>(x, e, A, shift, twA, lane, wi, wb, re1, im1, be, c_ang);
                }
            }
        }
        if (lane == 0) {
            out_idx[(long)f * cap + det] = wi;
            if (flag) {
                const int pos = atomicAdd(rf.n_flag, 1);
                if (pos < rf.list_cap) rf.list[pos] = f * cap + det;
                if (rf.flagpos && pos < rf.dense_cap) rf.flagpos[(long)f * cap + det] = pos + 1;
            }
        }
    }
}

// float64 first-max argmax of the zero-padded A-point DFT of n_ant complex128 cells per row (np.fft.fft + np.abs +
// np.argmax of the reference, point_cloud_generator.py:187-206).  One wave per row.
__device__ __forceinline__ int argmax64_wave(const cplx<double> *X, int n_ant, int A, int shift, const cplx<double> *twA,
                                             int lane) {
    double best = 0.0;
    int best_idx = 0x7fffffff;
    for (int k = lane; k < A; k += 64) {
        double re = 0.0, im = 0.0;
        int t = 0;
        for (int i = 0; i < n_ant; ++i) {
            const cplx<double> w = twA[t], xi = X[i];
            re += xi.x * w.x - xi.y * w.y;
            im += xi.x * w.y + xi.y * w.x;
            t += k;
            if (t >= A) t -= A;
        }
        const double m = hypot(re, im);
        const int kk = shift ? (k + A / 2) % A : k;
        if (best_idx == 0x7fffffff || mag_better(m, kk, best, best_idx)) {
            best = m;
            best_idx = kk;
        }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const double ob = __shfl_xor(best, d, 64);
        const int oi = __shfl_xor(best_idx, d, 64);
        if (oi != 0x7fffffff && (best_idx == 0x7fffffff || mag_better(ob, oi, best, best_idx))) {
            best = ob;
            best_idx = oi;
        }
    }
    return best_idx;
}

__global__ __launch_bounds__(256) void k_argmax64_cells(const cplx<double> *cells, int32_t *out_idx, int n_rows, int n_ant,
                                                         int A, int shift, const cplx<double> *twA) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n_rows) return;
    const int idx = argmax64_wave(cells + (long)row * n_ant, n_ant, A, shift, twA, lane);
    if (lane == 0) out_idx[row] = idx;
}

// Flagged detections: the range-Doppler cell of every listed antenna as the float64 2-D DFT coefficient of the windowed
// cube (direct S*C-term sum, table twiddles), then the float64 argmax.  The sum over a plane is cut into REFINE_PARTS
// slices, one workgroup each (a single workgroup per detection is latency-bound on its 32 trips to cold HBM lines):
//   k_argmax_refine_part   partial[e][part][i] for the first `n_split` flagged detections; a thread walks cells
//                          base + tid, + 256, ... keeping (s, c) and the two twiddle indices up to date incrementally and
//                          uses each cell's window * phase factor for all antennas of the list (phase tables: see
//                          refine_phases);
//   k_argmax_refine_finish adds the slices in a fixed order and runs the float64 argmax (one wave per detection);
//   k_argmax_refine_whole  whole planes in one workgroup: the (never yet seen) overflow beyond n_split detections.
// One flagged list may serve TWO antenna lists (mmw_detect_points: azimuth and elevation): an entry with bit 31 set
// belongs to the second (ants2 / shift2 / out_idx2).
#ifndef MMW_REFINE_PARTS
#define MMW_REFINE_PARTS 16
#endif
constexpr int REFINE_PARTS = MMW_REFINE_PARTS, REFINE_NA = 4;      // NA = 8 took 228 VGPRs: two workgroups per CU
constexpr int REFINE_SECOND = (int)0x80000000;

struct RefineArgs {
    const float2 *cubes;
    const int32_t *dets;
    const int *n_flag, *list;
    int list_cap;
    int32_t *out_idx, *out_idx2;
    int V, S, C, cap;
    AntList ants, ants2;
    int A, shift, shift2;
    const double *ws, *wc;
    const cplx<double> *twS, *twC, *twA;
    cplx<double> *partial;      // [n_split][parts][max(ants.n, ants2.n)]
    int n_split;
    int parts;                  // slices a plane sum is cut into (<= REFINE_PARTS): few when many detections are expected
    int dense_min, dense_cap;   // dense_min > 0: with *n_flag >= dense_min the first dense_cap entries belong to k_cells64
                                // (mmw_cells64.h) and these kernels take only what lies beyond them
};
// the entries [lo, n) of the flagged list the direct kernels own
__device__ __forceinline__ int refine_first(const RefineArgs &a, int n) {
    return a.dense_min > 0 && n >= a.dense_min ? (a.dense_cap < n ? a.dense_cap : n) : 0;
}

// Per flagged detection the factor of cell (s, c) splits into a range part and a Doppler part,
//   w_s(s) W_S^(r s)  *  w_c(c) W_C^(kd c),
// built once per task into two LDS tables (phS[S], phC[C]); the plane loop then reads phS[s] (one address per wave
// row: broadcast) and phC[c] (consecutive lanes, consecutive entries).  Gathering W_C^(kd c mod C) per cell instead put
// up to 64 lanes on one LDS bank (kd a multiple of 32) and the slowest task set the kernel's time.
inline size_t refine_tabs_lds(int S, int C) { return ((size_t)S + C) * 16 + 2 * MAX_ANT * sizeof(int); }

struct RefineTabs {
    cplx<double> *phS, *phC;
    int *ant;                   // ant[0..32) first list, ant[32..64) second
};
__device__ __forceinline__ RefineTabs refine_tabs(const RefineArgs &a, char *smem, int tid) {
    RefineTabs t;
    t.phS = reinterpret_cast<cplx<double> *>(smem);
    t.phC = t.phS + a.S;
    t.ant = reinterpret_cast<int *>(t.phC + a.C);
    if (tid == 0) {
        static_for<MAX_ANT>([&](auto I) {
            constexpr int i = decltype(I)::value;
            t.ant[i] = a.ants.idx[i];
            t.ant[MAX_ANT + i] = a.ants2.idx[i];
        });
    }
    return t;
}
// (every thread of the workgroup; ends with a barrier)
__device__ __forceinline__ void refine_phases(const RefineArgs &a, const RefineTabs &t, int r, int kd, int tid, int nt) {
    __syncthreads();            // the previous task's readers are done
    for (int s = tid; s < a.S; s += nt) t.phS[s] = a.twS[(int)(((long)r * s) % a.S)] * a.ws[s];
    for (int c = tid; c < a.C; c += nt) t.phC[c] = a.twC[(int)(((long)kd * c) % a.C)] * a.wc[c];
    __syncthreads();
}

// sum over cells [cell_lo, cell_hi) of plane (f, ant[a0 + i]) * window * phase, i < NA (antennas beyond n_ant: zero)
template <int NA>
__device__ __forceinline__ void refine_accumulate(const RefineArgs &a, const RefineTabs &t, const int *ant, int n_ant, int f, int a0,
                                                  long cell_lo, long cell_hi, int tid, cplx<double> (&acc)[NA]) {
    const int S = a.S, C = a.C;
    const long plane_cells = (long)S * C;
    const int ds = 256 / C, dc = 256 - ds * C;         // advancing a cell index by 256: c += dc (carry into s), s += ds
    const float2 *plane[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        acc[i] = cplx<double>{0.0, 0.0};
        plane[i] = a.cubes + ((long)f * a.V + (a0 + i < n_ant ? ant[a0 + i] : 0)) * plane_cells;
    }
    const long first = cell_lo + tid;
    int s = (int)(first / C), c = (int)(first - (long)s * C);
    if (s >= S) s = 0;
    constexpr int U = 4;        // four cells per trip: all of their (cold) samples are requested before any is used
    for (long cell0 = first; cell0 < cell_hi; cell0 += 256 * U) {
        float2 xv[U][NA];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                // unconditional, clamped (a guarded load is followed by its own wait: every one of these 16 loads cost a
                // full trip to HBM); cells past the end are not used, antennas past the list read plane 0 and are dropped
                const long cell = cell0 + 256 * u;
                xv[u][i] = plane[i][cell < cell_hi ? cell : cell_hi - 1];
            }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (cell0 + 256 * u < cell_hi) {
                const cplx<double> ph = cmul(t.phS[s], t.phC[c]);
#pragma unroll
                for (int i = 0; i < NA; ++i) acc[i] = acc[i] + cmul(cplx<double>{(double)xv[u][i].x, (double)xv[u][i].y}, ph);
            }
            c += dc;
            if (c >= C) {
                c -= C;
                ++s;
            }
            s += ds;
            if (s >= S) s = 0;          // past the plane (guarded above): keep the table index in range
        }
    }
}

// block-wide sum of acc[i] in a fixed order -> out[i] (thread i writes), `red` = [4][NA] LDS words
template <int NA>
__device__ __forceinline__ void refine_reduce(cplx<double> (&acc)[NA], cplx<double> (*red)[NA], int tid, cplx<double> *out, int n_out) {
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        for (int d = 32; d >= 1; d >>= 1) {
            acc[i].x += __shfl_xor(acc[i].x, d, 64);
            acc[i].y += __shfl_xor(acc[i].y, d, 64);
        }
        if (lane == 0) red[wave][i] = acc[i];
    }
    __syncthreads();
    if (tid < NA && tid < n_out) out[tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
    __syncthreads();
}

struct RefineEntry {
    int f, det, r, kd, which, n_ant;
};
__device__ __forceinline__ RefineEntry refine_entry(const RefineArgs &a, int e) {
    RefineEntry q;
    int id = a.list[e];
    q.which = id < 0 ? 1 : 0;
    id &= 0x7fffffff;
    q.n_ant = q.which ? a.ants2.n : a.ants.n;
    q.f = id / a.cap;
    q.det = id - q.f * a.cap;
    q.r = a.dets[((long)q.f * a.cap + q.det) * 2];
    int k = a.dets[((long)q.f * a.cap + q.det) * 2 + 1] - a.C / 2;     // FFT bin behind the fftshifted Doppler index
    if (k < 0) k += a.C;
    q.kd = k;
    return q;
}
__device__ __forceinline__ int refine_stride(const RefineArgs &a) { return a.ants.n > a.ants2.n ? a.ants.n : a.ants2.n; }

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void k_argmax_refine_part(RefineArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ cplx<double> red[4][REFINE_NA];
    int n = *a.n_flag;
    if (n > a.list_cap) n = a.list_cap;
    const int first = refine_first(a, n);
    if (n > a.n_split) n = a.n_split;
    if (first + (int)blockIdx.y >= n) return;
    const int part = blockIdx.x, tid = threadIdx.x;
    const RefineTabs t = refine_tabs(a, smem, tid);
    const long plane_cells = (long)a.S * a.C;
    const long per = ((plane_cells + a.parts - 1) / a.parts + 255) / 256 * 256;
    const long lo = (long)part * per, hi = lo + per < plane_cells ? lo + per : plane_cells;
    const int stride = refine_stride(a);
    for (int e = first + blockIdx.y; e < n; e += gridDim.y) {
        const RefineEntry q = refine_entry(a, e);
        refine_phases(a, t, q.r, q.kd, tid, 256);
        const int *al = t.ant + (q.which ? MAX_ANT : 0);
        for (int a0 = 0; a0 < q.n_ant; a0 += REFINE_NA) {
            cplx<double> acc[REFINE_NA];
            refine_accumulate<REFINE_NA>(a, t, al, q.n_ant, q.f, a0, lo < hi ? lo : hi, hi, tid, acc);
            refine_reduce<REFINE_NA>(acc, red, tid, a.partial + ((long)e * a.parts + part) * stride + a0, q.n_ant - a0);
        }
    }
}

__global__ __launch_bounds__(256) void k_argmax_refine_finish(RefineArgs a) {
    __shared__ cplx<double> X[4][MAX_ANT];
    int n = *a.n_flag;
    if (n > a.list_cap) n = a.list_cap;
    const int first = refine_first(a, n);
    if (n > a.n_split) n = a.n_split;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int stride = refine_stride(a);
    for (int e0 = first + blockIdx.x * 4; e0 < n; e0 += gridDim.x * 4) {
        const int e = e0 + wave;
        RefineEntry q{};
        if (e < n) {
            q = refine_entry(a, e);
            for (int i = lane; i < q.n_ant; i += 64) {
                cplx<double> s = cplx<double>{0.0, 0.0};
                for (int p = 0; p < a.parts; ++p) s = s + a.partial[((long)e * a.parts + p) * stride + i];
                X[wave][i] = s;
            }
        }
        __syncthreads();
        if (e < n) {
            const int idx = argmax64_wave(X[wave], q.n_ant, a.A, q.which ? a.shift2 : a.shift, a.twA, lane);
            if (lane == 0) (q.which ? a.out_idx2 : a.out_idx)[(long)q.f * a.cap + q.det] = idx;
        }
        __syncthreads();
    }
}

// Read-out of the cells themselves (mmw_rd_cells64_at): the slices k_argmax_refine_part left, added in the order
// k_argmax_refine_finish adds them, to cells[list[e]][i] instead of into an argmax.  One thread per (entry, antenna).
__global__ __launch_bounds__(256) void k_refine_cells_sum(RefineArgs a, cplx<double> *cells, int n) {
    const int stride = refine_stride(a);
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const int e = (int)(t / a.ants.n), i = (int)(t - (long)e * a.ants.n);
    if (e >= n) return;
    cplx<double> s = cplx<double>{0.0, 0.0};
    for (int p = 0; p < a.parts; ++p) s = s + a.partial[((long)e * a.parts + p) * stride + i];
    cells[(long)(a.list[e] & 0x7fffffff) * a.ants.n + i] = s;
}

__global__ __launch_bounds__(256) void k_argmax_refine_whole(RefineArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ cplx<double> red[4][REFINE_NA];
    __shared__ cplx<double> X[MAX_ANT];
    int n = *a.n_flag;
    if (n > a.list_cap) n = a.list_cap;
    const int tid = threadIdx.x;
    const int begin = a.n_split > refine_first(a, n) ? a.n_split : refine_first(a, n);
    if (begin + (int)blockIdx.x >= n) return;
    const RefineTabs t = refine_tabs(a, smem, tid);
    for (int e = begin + blockIdx.x; e < n; e += gridDim.x) {
        const RefineEntry q = refine_entry(a, e);
        refine_phases(a, t, q.r, q.kd, tid, 256);
        const int *al = t.ant + (q.which ? MAX_ANT : 0);
        for (int a0 = 0; a0 < q.n_ant; a0 += REFINE_NA) {
            cplx<double> acc[REFINE_NA];
            refine_accumulate<REFINE_NA>(a, t, al, q.n_ant, q.f, a0, 0, (long)a.S * a.C, tid, acc);
            refine_reduce<REFINE_NA>(acc, red, tid, X + a0, q.n_ant - a0);
        }
        if (tid < 64) {
            const int idx = argmax64_wave(X, q.n_ant, a.A, q.which ? a.shift2 : a.shift, a.twA, tid);
            if (tid == 0) (q.which ? a.out_idx2 : a.out_idx)[(long)q.f * a.cap + q.det] = idx;
        }
        __syncthreads();
    }
}

}  // namespace mmw
