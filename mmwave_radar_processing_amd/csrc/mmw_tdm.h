// TDM-MIMO Doppler phase compensation in front of the per-detection angle FFT + argmax (no upstream
// implementation).  The transmitters of a TDM-MIMO radar fire one chirp apart, so a target in fftshifted Doppler column c
// carries the extra phase 2 pi slot (c - C/2) / (n_slots C) on the virtual antennas of transmit slot `slot`.  The caller
// hands in the conjugate factors p[i][c] (complex128, made once on the host); every cell is multiplied by its factor
// before the zero-padded A-point DFT:
//   k_argmax_tdm<NA>        float32 pass over the resident complex64 cube, one lane per detection, with the worst-case
//                           certainty rule of mmw_argmax.h (independent errors; no pairwise form) widened by the error of
//                           the rounded phasor and of the float32 complex product;
//   k_tdm_gather_dets       the detections the float32 pass left undecided, as per-frame lists for the float64 cells;
//   k_argmax64_cells_tdm    float64 stage: cells x float64 table, then the angle DFT of k_argmax64_cells in its order.
// tdm_compensate / tdm_argmax64_bins are that float64 stage in plain C++: the kernel and mmw_diag_angle_argmax_tdm_host both
// call them (mmw_tu_tdm.hip is built with -ffp-contract=off, so neither side fuses what the other does not).
#pragma once
#include "mmw_argmax.h"

namespace mmw {

// rounded phasor + float32 complex product, in units of 2^-24 (|re| + |im|) of the float32 cell: DESIGN.md 4.30 derives
// sqrt(5) + 1 = 3.24
constexpr float TDM_PRODUCT_ULPS = 3.5f;

// which row of the de-duplicated float32 phasor table serves antenna i of the list
struct TdmRows {
    int n_rows;
    unsigned char row[MAX_ANT];
};

inline size_t tdm_lds(int A, int n_rows, int C) { return ((size_t)A + (size_t)n_rows * C) * sizeof(float2); }

// One lane per detection: 256 detections of a frame per workgroup (grid.x covers cap: no loop).  LDS: W_A^m and the
// float32 phasor rows, one per DISTINCT row of the table (a transmit slot) -- the DFT reads W_A^(ik) at an address the
// whole wave shares (broadcast), the phasor at the lane's own Doppler column.
template <int NA>
__global__ __launch_bounds__(256) void k_argmax_tdm(const float2 *__restrict__ rd, const int32_t *__restrict__ dets,
                                                     const int32_t *__restrict__ counts, int32_t *__restrict__ out_idx, int V, int S,
                                                     int C, int cap, AntList ants, int A, int shift, const float2 *__restrict__ twA,
                                                     const float2 *__restrict__ ph32, TdmRows rows, ArgmaxRefine rf, float k_tdm) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2 *tw = reinterpret_cast<float2 *>(smem);          // [A]
    float2 *ph = tw + A;                                    // [n_rows][C]
    const int tid = threadIdx.x;
    const long f = blockIdx.y;
    int n_det = counts[f];
    if (n_det > cap) n_det = cap;
    if ((int)blockIdx.x * 256 >= n_det) return;             // (the whole workgroup)
    for (int i = tid; i < A; i += 256) tw[i] = twA[i];
    for (int i = tid; i < rows.n_rows * C; i += 256) ph[i] = ph32[i];
    __syncthreads();
    const int det = blockIdx.x * 256 + tid;
    if (det >= n_det) return;
    const int n = ants.n;
    const long slot = f * cap + det;
    int r = dets[slot * 2], c = dets[slot * 2 + 1];
    // a detection outside the plane (never written by the detectors) must not turn into a wild read
    r = r < 0 ? 0 : (r >= S ? S - 1 : r);
    c = c < 0 ? 0 : (c >= C ? C - 1 : c);
    const long cell = (long)r * C + c;
    float2 y[NA];
    float sum_l1 = 0.f, sum_abs = 0.f, sum_in = 0.f;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int ant = ants.idx[i < n ? i : 0];
        const float2 x = rd[(f * V + ant) * (long)S * C + cell];        // unconditional; unused antennas read as zeros
        const float2 p = ph[(int)rows.row[i < n ? i : 0] * C + c];
        y[i] = i < n ? make_float2(x.x * p.x - x.y * p.y, x.x * p.y + x.y * p.x) : make_float2(0.f, 0.f);
        if (i < n) {
            sum_l1 += rf.l1[f * V + ant];
            sum_in += fabsf(x.x) + fabsf(x.y);
            sum_abs += fabsf(y[i].x) + fabsf(y[i].y);
        }
    }
    // first maximum in output order and the largest other magnitude
    float best = 0.f, second = -__builtin_huge_valf();
    int wi = 0;
    const int k0 = shift ? A - A / 2 : 0;                   // output bin kk is DFT bin (kk + k0) mod A
    int k = k0 >= A ? k0 - A : k0;
    for (int kk = 0; kk < A; ++kk) {
        float re = 0.f, im = 0.f;
        int t = 0;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const float2 w = tw[t];
            re += y[i].x * w.x - y[i].y * w.y;
            im += y[i].x * w.y + y[i].y * w.x;
            t += k;
            if (t >= A) t -= A;
        }
        const float m = hypotf(re, im);
        if (kk == 0) {
            best = m;
        } else if (mag_gt(m, best)) {
            second = best;
            best = m;
            wi = kk;
        } else if (mag_gt(m, second)) {
            second = m;
        }
        if (++k >= A) k -= A;
    }
    out_idx[slot] = wi;
    // worst case, independent errors: range-Doppler cells + the phasor product + the n-term sum and the magnitude
    const float bound = rf.k_fft * sum_l1 + k_tdm * sum_in + rf.k_ang * sum_abs;
    if (!(best - second > 2.f * bound)) {                   // (also for NaN / inf magnitudes, and for A == 1)
        const int pos = atomicAdd(rf.n_flag, 1);
        if (pos < rf.list_cap) rf.list[pos] = (int)slot;
    }
}

// dets2[j] = dets[slot2[j]] for the n listed slots (the per-frame lists of undecided detections mmw_rd_cells64_at reads)
__global__ __launch_bounds__(256) void k_tdm_gather_dets(const int32_t *dets, const int32_t *slot2, int32_t *dets2, int n) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const int s = slot2[j];
    if (s < 0) return;                                      // (past the frame's count)
    dets2[2 * (long)j] = dets[2 * (long)s];
    dets2[2 * (long)j + 1] = dets[2 * (long)s + 1];
}

// np.argmax order without device intrinsics (the host calls it too)
__host__ __device__ inline bool tdm_mag_gt(double a, double b) {
    if (a != a) return !(b != b);
    if (b != b) return false;
    return a > b;
}

// The float64 stage of one row.  tdm_compensate: y_i = z_i p_i (four products, one rounding each).  tdm_argmax64_bins: bins
// lane, lane + stride, ... with the sums of argmax64_wave in its order.  The order of two bins is decided on re^2 + im^2
// (every operation rounded once): the square root is monotone, so this is the order of |.| short of overflow, and the host
// and the device agree on it bit for bit, which their hypot() implementations do not promise.  Returns the lane's best
// (index 0x7fffffff: none).
__host__ __device__ inline void tdm_compensate(const double *z, const double *p, double *y) {
    const double zr = z[0], zi = z[1], pr = p[0], pi = p[1];
    y[0] = zr * pr - zi * pi;
    y[1] = zr * pi + zi * pr;
}
__host__ __device__ inline bool tdm_better(double a, int ia, double b, int ib) {
    return tdm_mag_gt(a, b) || (!tdm_mag_gt(b, a) && ia < ib);
}
__host__ __device__ inline void tdm_argmax64_bins(const double *y, int n_ant, int A, int shift, const double *twA, int lane,
                                                  int stride, double *best_out, int *idx_out) {
    double best = 0.0;
    int best_idx = 0x7fffffff;
    for (int k = lane; k < A; k += stride) {
        double re = 0.0, im = 0.0;
        int t = 0;
        for (int i = 0; i < n_ant; ++i) {
            const double wr = twA[2 * t], wi = twA[2 * t + 1];
            re += y[2 * i] * wr - y[2 * i + 1] * wi;
            im += y[2 * i] * wi + y[2 * i + 1] * wr;
            t += k;
            if (t >= A) t -= A;
        }
        const double m = re * re + im * im;
        const int kk = shift ? (k + A / 2) % A : k;
        if (best_idx == 0x7fffffff || tdm_better(m, kk, best, best_idx)) {
            best = m;
            best_idx = kk;
        }
    }
    *best_out = best;
    *idx_out = best_idx;
}

// One wave per row: cells[row][n_ant] x phase[i][col[row]] (both complex128), argmax to out_idx[dst ? dst[row] : row].
// cols: the row's Doppler column at cols[row * col_stride].  count / cap2 (optional): row (f, j) of an [F][cap2] layout
// is live while j < count[f].
__global__ __launch_bounds__(256) void k_argmax64_cells_tdm(const double *cells, const int32_t *cols, int col_stride,
                                                             const double *phase, const int32_t *dst, const int32_t *count, int cap2,
                                                             int32_t *out_idx, long n_rows, int n_ant, int C, int A, int shift,
                                                             const double *twA) {
    __shared__ double y[4][2 * MAX_ANT];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + wave;
    bool live = row < n_rows;
    if (live && count) live = (int)(row % cap2) < count[row / cap2];
    if (live && lane < n_ant) {
        int c = cols[row * col_stride];
        c = c < 0 ? 0 : (c >= C ? C - 1 : c);
        tdm_compensate(cells + 2 * (row * n_ant + lane), phase + 2 * ((long)lane * C + c), y[wave] + 2 * lane);
    }
    __syncthreads();
    if (!live) return;
    double best;
    int best_idx;
    tdm_argmax64_bins(y[wave], n_ant, A, shift, twA, lane, 64, &best, &best_idx);
    for (int d = 32; d >= 1; d >>= 1) {
        const double ob = __shfl_xor(best, d, 64);
        const int oi = __shfl_xor(best_idx, d, 64);
        if (oi != 0x7fffffff && (best_idx == 0x7fffffff || tdm_better(ob, oi, best, best_idx))) {
            best = ob;
            best_idx = oi;
        }
    }
    if (lane == 0) out_idx[dst ? dst[row] : row] = best_idx;
}

}  // namespace mmw
