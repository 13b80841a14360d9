// Batched sequential detector (FramePipeline(sequential=...)): RangeDopplerDetectorSequential.process for
// F frames at once.
//
//   k_seq_rows      one workgroup per frame: the range CFAR (cfar1d_threshold, the code of k_cfar1d) on the float64 chirp-0
//                   range profile -> the ascending list of selected range rows and its length
//   k_seq_detect    one workgroup per frame: for the selected rows only, the float64 Doppler row of antenna 0
//                   |fftshift FFT_C(hann(C) * X[r, :])|, the velocity CFAR on it and the ordered list of hits.  The row
//                   never leaves the CU: range bins are direct sums from a float64 twiddle table in LDS, the Doppler
//                   transform is a direct float64 DFT of the row in LDS (any C, no power-of-two requirement), the
//                   magnitudes are tested by cfar1d_threshold where they lie.
//   The full-plane route (MMW_SEQ_FULL_PLANE = 1, the default) is mmw_ground.h's k_cfar1d_gated given the row list;
//   k_seq_detect runs with MMW_SEQ_FULL_PLANE = 0.
//
// Work per thread in k_seq_detect: SEQ_RPT rows of one column.  The 256 threads of a workgroup cover min(C, 256) columns
// times 256 / min(C, 256) row groups, so one pass takes SEQ_RPT * (256 / min(C, 256)) selected rows (8 for C = 128) and
// reads antenna 0's plane once, from L2; a frame with n selected rows takes ceil(n / that) passes.  Within a wave the
// twiddle index r * s mod S is the same for every lane (an LDS broadcast) and the sample loads are consecutive.
#pragma once
#include "mmw_cfar.h"

namespace mmw {

constexpr int SEQ_RPT = 4;                   // selected rows one thread accumulates at a time
constexpr size_t SEQ_LDS_MAX = 160 * 1024;   // LDS of one CU
constexpr int SEQ_FULL_PLANE_DEFAULT = 1;    // MMW_SEQ_FULL_PLANE when nobody sets it: the full plane measured faster

// wave 0 appends the set flags of one row in ascending order; returns the number of flags (all lanes)
template <typename Emit>
__device__ __forceinline__ int wave_append_row(const uint8_t *flags, int n, int base, Emit emit) {
    const int lane = threadIdx.x & 63;
    int total = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const bool on = i < n && flags[i];
        const unsigned long long m = __ballot(on);
        if (on) emit(base + total + __popcll(m & ((1ull << lane) - 1ull)), i);
        total += __popcll(m);
    }
    return total;
}

// prof[F][S] float64 -> rows[F][S] (the first nrows[f] entries: indices with prof > threshold, ascending), nrows[F]
__global__ __launch_bounds__(256) void k_seq_rows(Cfar1dArgs p, int32_t *rows, int32_t *nrows) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int S = p.L;
    double *x = reinterpret_cast<double *>(smem);                    // [S]
    uint8_t *hit = reinterpret_cast<uint8_t *>(x + S);               // [S]
    const long f = blockIdx.x;
    for (int i = threadIdx.x; i < S; i += 256) x[i] = p.x[f * S + i];
    __syncthreads();
    for (int i = threadIdx.x; i < S; i += 256) {
        double est;
        hit[i] = x[i] > cfar1d_threshold(p, x, i, &est) ? 1 : 0;
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        int32_t *out = rows + f * S;
        const int n = wave_append_row(hit, S, 0, [&](int pos, int i) { out[pos] = i; });
        if (threadIdx.x == 0) nrows[f] = n;
    }
}

struct SeqArgs {
    const float2 *cubes;                 // [F][V][S][C] complex64; antenna 0 is read
    const double *hann_s, *hann_c;       // np.hanning(S), np.hanning(C) (TAB_HANN)
    const double2 *tw_s, *tw_c;          // exp(-2 pi i m / S), exp(-2 pi i m / C) (TAB_TWIDDLE)
    const int32_t *rows, *nrows;         // [F][S], [F] from k_seq_rows
    int32_t *dets, *counts;              // [F][cap][2], [F]
    double *rowmag;                      // nullptr, or [F][S][C]: Doppler row of rows[f][j] at [f][j] (error measurement)
    int V, S, C, cap;
    Cfar1dArgs cfar;                     // the velocity CFAR; x unused, L = C
};

__host__ __device__ inline int seq_cols(int C) { return C < 256 ? C : 256; }
__host__ __device__ inline int seq_pass_rows(int C) { return SEQ_RPT * (256 / seq_cols(C)); }
// twiddles of S and C, then per pass: windowed range bins (double2), magnitudes (double), hit flags
inline size_t seq_lds_bytes(int S, int C) {
    return ((size_t)S + C) * sizeof(double2) + (size_t)seq_pass_rows(C) * C * (sizeof(double2) + sizeof(double) + 1);
}

__global__ __launch_bounds__(256) void k_seq_detect(SeqArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int S = a.S, C = a.C;
    const int ncol = seq_cols(C), parts = 256 / ncol, RB = SEQ_RPT * parts;
    double2 *twS = reinterpret_cast<double2 *>(smem);                // [S]
    double2 *twC = twS + S;                                          // [C]
    double2 *y = twC + C;                                            // [RB][C] hann(C)[c] * X[r, c]
    double *mag = reinterpret_cast<double *>(y + (size_t)RB * C);    // [RB][C] the Doppler rows
    uint8_t *hit = reinterpret_cast<uint8_t *>(mag + (size_t)RB * C);
    const long f = blockIdx.x;
    const int tid = threadIdx.x;
    for (int i = tid; i < S; i += 256) twS[i] = a.tw_s[i];
    for (int i = tid; i < C; i += 256) twC[i] = a.tw_c[i];
    int n = a.nrows[f];
    n = n < 0 ? 0 : (n > S ? S : n);
    const int32_t *rows = a.rows + f * S;
    const float2 *x0 = a.cubes + f * a.V * (long)S * C;              // antenna 0
    int32_t *out = a.dets + f * (long)a.cap * 2;
    const int col = tid % ncol, q = tid / ncol;                      // q >= parts: no work (C does not divide 256)
    Cfar1dArgs cf = a.cfar;
    cf.L = C;
    int total = 0;                                                   // hits so far (wave 0)
    __syncthreads();
    for (int j0 = 0; j0 < n; j0 += RB) {
        const int nr = n - j0 < RB ? n - j0 : RB;
        int slot[SEQ_RPT], r[SEQ_RPT];
#pragma unroll
        for (int k = 0; k < SEQ_RPT; ++k) {
            slot[k] = q + k * parts;
            const int v = slot[k] < nr ? rows[j0 + slot[k]] : 0;     // idle slots and entries outside [0, S) run row 0 and are dropped
            r[k] = (unsigned)v < (unsigned)S ? v : 0;
        }
        // range bins X[r, c] = sum_s hann(S)[s] x[0, s, c] W_S^(r s), in the order s = 0 .. S - 1
        if (q < parts && slot[0] < nr) {
            for (int c = col; c < C; c += ncol) {
                double2 acc[SEQ_RPT];
                int idx[SEQ_RPT];
#pragma unroll
                for (int k = 0; k < SEQ_RPT; ++k) {
                    acc[k] = make_double2(0.0, 0.0);
                    idx[k] = 0;
                }
#pragma unroll 4
                for (int s = 0; s < S; ++s) {
                    const float2 v = x0[(long)s * C + c];
                    const double hs = a.hann_s[s];
                    const double xr = (double)v.x * hs, xi = (double)v.y * hs;
#pragma unroll
                    for (int k = 0; k < SEQ_RPT; ++k) {
                        const double2 w = twS[idx[k]];
                        acc[k].x += xr * w.x - xi * w.y;
                        acc[k].y += xr * w.y + xi * w.x;
                        idx[k] += r[k];
                        if (idx[k] >= S) idx[k] -= S;
                    }
                }
                const double hc = a.hann_c[c];
#pragma unroll
                for (int k = 0; k < SEQ_RPT; ++k)
                    if (slot[k] < nr) y[(size_t)slot[k] * C + c] = make_double2(acc[k].x * hc, acc[k].y * hc);
            }
        }
        __syncthreads();
        // Doppler rows: bin d of the shifted spectrum is frequency (d - C / 2) mod C (np.fft.fftshift)
        if (q < parts) {
            for (int d = col; d < C; d += ncol) {
                const int kf = (d + C - C / 2) % C;
                double2 acc[SEQ_RPT];
#pragma unroll
                for (int k = 0; k < SEQ_RPT; ++k) acc[k] = make_double2(0.0, 0.0);
                int idx = 0;
                for (int c = 0; c < C; ++c) {
                    const double2 w = twC[idx];
                    idx += kf;
                    if (idx >= C) idx -= C;
#pragma unroll
                    for (int k = 0; k < SEQ_RPT; ++k) {
                        if (slot[k] < nr) {
                            const double2 v = y[(size_t)slot[k] * C + c];
                            acc[k].x += v.x * w.x - v.y * w.y;
                            acc[k].y += v.x * w.y + v.y * w.x;
                        }
                    }
                }
#pragma unroll
                for (int k = 0; k < SEQ_RPT; ++k)
                    if (slot[k] < nr) {
                        const double m = hypot(acc[k].x, acc[k].y);
                        mag[(size_t)slot[k] * C + d] = m;
                        if (a.rowmag) a.rowmag[((size_t)f * S + j0 + slot[k]) * C + d] = m;
                    }
            }
        }
        __syncthreads();
        if (q < parts) {
            for (int d = col; d < C; d += ncol) {
#pragma unroll
                for (int k = 0; k < SEQ_RPT; ++k) {
                    if (slot[k] < nr) {
                        const double *row = mag + (size_t)slot[k] * C;
                        double est;
                        hit[(size_t)slot[k] * C + d] = row[d] > cfar1d_threshold(cf, row, d, &est) ? 1 : 0;
                    }
                }
            }
        }
        __syncthreads();
        if (tid < 64) {
            for (int j = 0; j < nr; ++j) {
                const int rj = rows[j0 + j];
                if ((unsigned)rj >= (unsigned)S) continue;           // no such row: no hits (its slot ran row 0), as k_cfar1d_gated
                total += wave_append_row(hit + (size_t)j * C, C, total, [&](int pos, int d) {
                    if (pos < a.cap) {
                        out[2 * pos] = rj;
                        out[2 * pos + 1] = d;
                    }
                });
            }
        }
    }
    if (tid == 0) a.counts[f] = total;
}

}  // namespace mmw
