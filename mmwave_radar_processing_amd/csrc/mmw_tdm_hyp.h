// TDM-MIMO velocity unwrapping: Doppler hypotheses per detection (no upstream implementation).  TDM with n_slots
// transmitters samples each virtual antenna every n_slots-th chirp, so a target's Doppler bin is known modulo C only: its true
// bin is k + h C for one h in [0, n_slots), and the compensation of mmw_tdm.h needs the factor of THAT bin.  The wrong h leaves a
// phase step of 2 pi slot h / n_slots between the sub-apertures of different slots and lowers the angle peak; the caller hands in
// one phase table per hypothesis (batch.tdm_hypothesis_table), and the hypothesis with the highest peak is the answer:
//   k_argmax_tdm_hyp<NA>          float32 pass, one lane per detection, cells loaded once, every distinct hypothesis compensated
//                                 and transformed in turn; the certainty rule of mmw_tdm.h applied across all (h, bin) pairs;
//   k_argmax64_cells_tdm_hyp      float64 stage: one wave per row, tdm_compensate / tdm_argmax64_bins per distinct hypothesis,
//                                 tdm_better between hypotheses;
//   k_tdm_hyp_fill                live slots of d_hyp <- 0 (calls with one distinct hypothesis);
//   k_tdm_unwrap_velocity         column 3 of the point cloud <- vel_bins[c] + m span where the chosen hypothesis folds (m != 0).
// Hypotheses whose [n_ant][C] blocks are equal bit for bit, or are both a phase common to the whole list (all rows equal), cannot
// be told apart: the later one is a duplicate and is never evaluated (tdm_hyp_plan).  tdm_hyp_row64_host is the float64 stage of
// one row in plain C++, built from the functions the kernel calls (tdm_compensate, tdm_argmax64_bins, tdm_better; this unit is
// built with -ffp-contract=off, so neither side fuses what the other does not).
#pragma once
#include "mmw_tdm.h"

#include <cstring>
#include <vector>

namespace mmw {

constexpr int TDM_MAX_HYP = 8;

// what the kernels need to know about the hypotheses of one call
struct TdmHypRows {
    int n_hyp;                                  // distinct hypotheses, evaluated in ascending order of their original number
    int H;                                      // hypotheses the caller listed
    int n_rows;                                 // distinct float32 phasor rows over (distinct hypothesis, antenna)
    int orig[TDM_MAX_HYP];                      // original number of distinct hypothesis d
    int map[TDM_MAX_HYP];                       // distinct index of original hypothesis h (a duplicate: of the one it duplicates)
    unsigned char row[TDM_MAX_HYP][MAX_ANT];    // float32 row of (distinct hypothesis d, antenna i)
};

// Host: the distinct hypotheses of h_phase [H][n_ant][C][2] and the de-duplicated float32 rows (ph32, may be null).
inline TdmHypRows tdm_hyp_plan(const double *h_phase, int H, int n_ant, int C, std::vector<float> *ph32) {
    TdmHypRows p{};
    p.H = H;
    const size_t row_bytes = (size_t)C * 2 * sizeof(double), block = (size_t)n_ant * C * 2;
    bool common[TDM_MAX_HYP];
    for (int h = 0; h < H; ++h) {
        const double *b = h_phase + (size_t)h * block;
        common[h] = true;
        for (int i = 1; i < n_ant && common[h]; ++i) common[h] = std::memcmp(b, b + (size_t)i * C * 2, row_bytes) == 0;
        int d = -1;
        for (int j = 0; j < p.n_hyp && d < 0; ++j) {
            const int g = p.orig[j];
            if ((common[h] && common[g]) || std::memcmp(b, h_phase + (size_t)g * block, block * sizeof(double)) == 0) d = j;
        }
        if (d < 0) {
            d = p.n_hyp++;
            p.orig[d] = h;
        }
        p.map[h] = d;
    }
    // float32 rows: (d, i) pairs whose float64 rows are equal bit for bit share one (slot 0 is one row of ones)
    std::vector<const double *> first;
    for (int d = 0; d < p.n_hyp; ++d)
        for (int i = 0; i < n_ant; ++i) {
            const double *src = h_phase + (size_t)p.orig[d] * block + (size_t)i * C * 2;
            int r = -1;
            for (size_t j = 0; j < first.size() && r < 0; ++j)
                if (std::memcmp(src, first[j], row_bytes) == 0) r = (int)j;
            if (r < 0) {
                r = (int)first.size();
                first.push_back(src);
                if (ph32)
                    for (int c = 0; c < 2 * C; ++c) ph32->push_back((float)src[c]);
            }
            p.row[d][i] = (unsigned char)r;       // (at most TDM_MAX_HYP * MAX_ANT = 256 rows)
        }
    p.n_rows = (int)first.size();
    return p;
}

// One lane per detection, as k_argmax_tdm: 256 detections of a frame per workgroup, W_A^m and the de-duplicated float32 phasor
// rows in the LDS, the cells of the detection loaded ONCE into registers; every distinct hypothesis is compensated into a second
// register array and transformed.  hyp_given: only hypothesis hyp[slot] (clamped, a duplicate mapped) is evaluated and hyp is left
// alone; else hyp[slot] <- the original number of the winner.
template <int NA>
__global__ __launch_bounds__(256) void k_argmax_tdm_hyp(const float2 *__restrict__ rd, const int32_t *__restrict__ dets,
                                                         const int32_t *__restrict__ counts, int32_t *__restrict__ out_idx,
                                                         int32_t *__restrict__ hyp, int hyp_given, int V, int S, int C, int cap,
                                                         AntList ants, int A, int shift, const float2 *__restrict__ twA,
                                                         const float2 *__restrict__ ph32, TdmHypRows rows, ArgmaxRefine rf, float k_tdm) {
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
    r = r < 0 ? 0 : (r >= S ? S - 1 : r);                   // (as k_argmax_tdm: never a wild read)
    c = c < 0 ? 0 : (c >= C ? C - 1 : c);
    const long cell = (long)r * C + c;
    float2 x[NA], y[NA];
    float sum_l1 = 0.f, sum_in = 0.f;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int ant = ants.idx[i < n ? i : 0];
        x[i] = rd[(f * V + ant) * (long)S * C + cell];
        if (i < n) {
            sum_l1 += rf.l1[f * V + ant];
            sum_in += fabsf(x[i].x) + fabsf(x[i].y);
        }
    }
    // the hypothesis loop runs on a wave-uniform d (the tables of `rows` are read with scalar loads); a lane with a given
    // hypothesis skips the others
    int mine = -1;
    if (hyp_given) {
        int h = hyp[slot];
        h = h < 0 ? 0 : (h >= rows.H ? rows.H - 1 : h);
        for (int g = 0; g < rows.H; ++g)
            if (g == h) mine = rows.map[g];
    }
    // first maximum over (hypothesis, bin) in that order and the largest other magnitude of all pairs
    float best = 0.f, second = -__builtin_huge_valf(), max_abs = 0.f;
    int wi = 0, wh = 0;
    bool first = true;
    const int k0 = shift ? A - A / 2 : 0;                   // output bin kk is DFT bin (kk + k0) mod A
    for (int d = 0; d < rows.n_hyp; ++d) {
        if (mine >= 0 && d != mine) continue;
        float sum_abs = 0.f;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const float2 p = ph[(int)rows.row[d][i < n ? i : 0] * C + c];
            y[i] = i < n ? make_float2(x[i].x * p.x - x[i].y * p.y, x[i].x * p.y + x[i].y * p.x) : make_float2(0.f, 0.f);
            if (i < n) sum_abs += fabsf(y[i].x) + fabsf(y[i].y);
        }
        max_abs = fmaxf(max_abs, sum_abs);
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
            if (first) {
                best = m;
                wh = rows.orig[d];
                first = false;
            } else if (mag_gt(m, best)) {
                second = best;
                best = m;
                wi = kk;
                wh = rows.orig[d];
            } else if (mag_gt(m, second)) {
                second = m;
            }
            if (++k >= A) k -= A;
        }
    }
    out_idx[slot] = wi;
    if (!hyp_given) hyp[slot] = wh;
    // the rule of k_argmax_tdm across the hypotheses: every p_h is a unit phasor rounded the same way, so the derived terms hold
    // per hypothesis, and the largest of the DFT-input norms covers them all
    const float bound = rf.k_fft * sum_l1 + k_tdm * sum_in + rf.k_ang * max_abs;
    if (A == 1 || !(best - second > 2.f * bound)) {         // (also NaN / inf magnitudes and exact ties between hypotheses)
        const int pos = atomicAdd(rf.n_flag, 1);
        if (pos < rf.list_cap) rf.list[pos] = (int)slot;
    }
}

// One wave per row: cells[row][n_ant] (complex128), the row's Doppler column at cols[row * col_stride], results to
// out_idx / hyp [dst ? dst[row] : row].  count / cap2 (optional): row (f, j) of an [F][cap2] layout is live while j < count[f].
// Every wave of the workgroup walks all n_hyp hypotheses (the barriers are workgroup-wide); a row skips the ones it does not need.
__global__ __launch_bounds__(256) void k_argmax64_cells_tdm_hyp(const double *cells, const int32_t *cols, int col_stride,
                                                                 const double *phase, TdmHypRows rows, const int32_t *dst,
                                                                 const int32_t *count, int cap2, int32_t *out_idx, int32_t *hyp,
                                                                 int hyp_given, long n_rows, int n_ant, int C, int A, int shift,
                                                                 const double *twA) {
    __shared__ double y[4][2 * MAX_ANT];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + wave;
    bool live = row < n_rows;
    if (live && count) live = (int)(row % cap2) < count[row / cap2];
    const long out = live ? (dst ? dst[row] : row) : 0;
    int c = 0, mine = -1;
    if (live) {
        c = cols[row * col_stride];
        c = c < 0 ? 0 : (c >= C ? C - 1 : c);
        if (hyp_given) {
            int h = hyp[out];
            h = h < 0 ? 0 : (h >= rows.H ? rows.H - 1 : h);
            for (int g = 0; g < rows.H; ++g)
                if (g == h) mine = rows.map[g];
        }
    }
    double best_p = 0.0;
    int best_idx = 0, best_d = -1, best_h = 0;
    for (int d = 0; d < rows.n_hyp; ++d) {
        const bool on = live && (mine < 0 || mine == d);
        if (on && lane < n_ant)
            tdm_compensate(cells + 2 * (row * n_ant + lane), phase + 2 * (((size_t)rows.orig[d] * n_ant + lane) * C + c), y[wave] + 2 * lane);
        __syncthreads();
        if (on) {
            double pd;
            int id;
            tdm_argmax64_bins(y[wave], n_ant, A, shift, twA, lane, 64, &pd, &id);
            for (int s = 32; s >= 1; s >>= 1) {
                const double ob = __shfl_xor(pd, s, 64);
                const int oi = __shfl_xor(id, s, 64);
                if (oi != 0x7fffffff && (id == 0x7fffffff || tdm_better(ob, oi, pd, id))) {
                    pd = ob;
                    id = oi;
                }
            }
            if (best_d < 0 || tdm_better(pd, d, best_p, best_d)) {
                best_p = pd;
                best_idx = id;
                best_d = d;
                best_h = rows.orig[d];
            }
        }
        __syncthreads();                                    // (y is rewritten by the next hypothesis)
    }
    if (live && lane == 0) {
        out_idx[out] = best_idx;
        if (!hyp_given) hyp[out] = best_h;
    }
}

// The same row on the host: the distinct hypotheses d_lo .. d_hi - 1 in turn, the functions the kernel calls (one lane, stride 1).
// Returns the angle index and the distinct hypothesis of the first maximum.
inline void tdm_hyp_row64_host(const double *z, const double *phase, const TdmHypRows &rows, int d_lo, int d_hi, int c, int n_ant, int C,
                               int A, int shift, const double *twA, int *idx_out, int *d_out) {
    double y[2 * MAX_ANT], best_p = 0.0;
    int best_idx = 0, best_d = -1;
    for (int d = d_lo; d < d_hi; ++d) {
        for (int i = 0; i < n_ant; ++i)
            tdm_compensate(z + 2 * i, phase + 2 * (((size_t)rows.orig[d] * n_ant + i) * C + c), y + 2 * i);
        double pd;
        int id;
        tdm_argmax64_bins(y, n_ant, A, shift, twA, 0, 1, &pd, &id);
        if (best_d < 0 || tdm_better(pd, d, best_p, best_d)) {
            best_p = pd;
            best_idx = id;
            best_d = d;
        }
    }
    *idx_out = best_idx;
    *d_out = best_d;
}

// live slots of hyp[F][cap] <- 0
__global__ __launch_bounds__(256) void k_tdm_hyp_fill(const int32_t *counts, int32_t *hyp, int cap) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const long f = blockIdx.y;
    int n = counts[f];
    n = n > cap ? cap : n;
    if (j < n) hyp[f * cap + j] = 0;
}

// sym(q) = ((q + M // 2) mod M) - M // 2 with a floor mod; k' = sym(k + h C), m = (k' - k) / C (exact)
__host__ __device__ inline int tdm_unwrap_m(int c, int h, int n_slots, int C) {
    const long M = (long)n_slots * C, k = c - C / 2;
    long q = (k + (long)h * C + M / 2) % M;
    if (q < 0) q += M;
    return (int)((q - M / 2 - k) / C);
}

// One lane per live slot: v = vel_bins[c] + float64(m) span where m != 0 (one multiply, one add; this unit does not contract);
// a slot with m == 0 is not written.  The Doppler column is read as k_point_cloud reads it (outside the plane: column 0).
__global__ __launch_bounds__(256) void k_tdm_unwrap_velocity(double *points, const int32_t *dets, const int32_t *counts,
                                                              const int32_t *hyp, int cap, int C, int n_slots, double span) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const long f = blockIdx.y;
    int n = counts[f];
    n = n > cap ? cap : n;
    if (j >= n) return;
    const long s = f * cap + j;
    int c = dets[2 * s + 1];
    c = (unsigned)c < (unsigned)C ? c : 0;
    int h = hyp[s];
    h = h < 0 ? 0 : (h >= n_slots ? n_slots - 1 : h);
    const int m = tdm_unwrap_m(c, h, n_slots, C);
    if (m != 0) points[4 * s + 3] = points[4 * s + 3] + (double)m * span;
}

}  // namespace mmw
