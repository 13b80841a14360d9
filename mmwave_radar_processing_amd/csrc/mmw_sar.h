// Strip-map SAR slices (mmw_sar_slices): per frame one window of the un-windowed range-Doppler plane of one antenna, complex,
//   out_f[r - row_lo][c - col_lo] = X_f[r][(c + C - C/2) mod C],   X_f = FFT_S FFT_C( x[f][rx] ),
//   row_lo <= r < row_hi, col_lo <= c < col_hi, every frame with a window of its own and its block at an offset of its own.
//
// StripMapSARProcessor.process (processors/strip_map_SAR_processor.py:160-194) takes fftshift_C(fft2(x[rx])) and keeps
// [valid_ranges_slice, valid_angles_slice] of it: the rows between the sensor height and the maximum distance, the Doppler columns
// between two azimuth angles at that frame's platform speed.  As in mmw_micro_doppler.h only the K rows of the window are made
// (a K-row partial DFT over fast time: the same stage 1, lane = column, wave = every fourth sample), and of the slow-time
// transform only the N columns of the window: K N direct sums of length C, one (row, column) pair per thread.  Everything is
// float32 and a direct sum, so every S and C runs the same code.  Nothing but the blocks is written.
//
// Shapes: any S >= 1, and the C that mmw_micro_doppler serves (md_pick_kt: C <= 3444, the rows in flight live in the LDS).
// The launch asks for md_lds_bytes(KT, C), which counts k_micro_doppler's C running maxima too; this kernel has no use for
// them.  The 4 C bytes are asked for all the same so that both entries refuse at the same C, by one formula.  The shape is judged
// before the windows: a C beyond the limit is MMW_ERR_UNSUPPORTED even when every window of the call is empty.
// Grid: one workgroup per frame up to SAR_GRID_MAX workgroups; past that a workgroup walks frames f, f + grid, ...
#pragma once
#include "mmw_md_core.h"

namespace mmw {

constexpr int SAR_GRID_MAX = 4096;      // workgroups of one launch: 16 per CU of an MI355X

struct SarArgs {
    const float2 *cubes;                // [F][V][S][C]
    const float2 *tw1;                  // [S][KP]: W_S^((row0 + kp) s), k_sar_twiddle's table over the union of the row windows
    const float2 *twc;                  // [C]: W_C^m
    const int4 *win;                    // [F]: row_lo, row_hi, col_lo, col_hi (half open)
    const long long *off;               // [F]: first element of the frame's block
    float2 *out;
    int n_frames, V, S, C, rx, row0, KP;
};

// tw[s][kp] = W_S^((row0 + kp) s), kp < KP: rows row0 ... of the union of the frames' row windows plus the padding of a last
// chunk (valid twiddles of rows that no frame stores), every entry copied from the exactly rounded table W_S^m.
__global__ __launch_bounds__(256) void k_sar_twiddle(const float2 *__restrict__ base, float2 *__restrict__ tw, int S, int row0, int KP) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= (long)S * KP) return;
    const long s = i / KP, r = (row0 + i % KP) % S;
    tw[i] = base[(r * s) % S];
}

// One workgroup (4 waves) per frame, the window's rows in chunks of KT.
//   stage 1  Z[c][kt] = sum_s W_S^((row_lo + k0 + kt) s) x[s][c] for every column c: k_micro_doppler's stage 1 (same loads, same
//            order of every sum), with the twiddle row of the frame's window picked out of the table of the union.
//   stage 2  thread i of the chunk's KT x N outputs (column fastest, so a wave stores consecutive elements of a block row):
//            Y = sum_j Z[j][kt] W_C^(j k), k = (col + C - C/2) mod C the FFT bin behind column col of np.fft.fftshift; the
//            twiddle index steps by k (mod C, exact).  Rows past the window's end (the padding of the last chunk) are skipped.
// The order of every sum depends on (S, C) alone: a frame's block does not depend on KT, the batch or the other windows.
template <int KT>
__global__ __launch_bounds__(256) void k_sar_slices(SarArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2 *part = reinterpret_cast<float2 *>(smem);                    // [3][KT][MD_COLS]
    float2 *Z = part + 3 * KT * MD_COLS;                                // [C][KT]
    float2 *twl = Z + (size_t)p.C * KT;                                 // [C]
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int S = p.S, C = p.C;
    for (int c = threadIdx.x; c < C; c += 256) twl[c] = p.twc[c];
    for (long f = blockIdx.x; f < p.n_frames; f += gridDim.x) {
        const int4 wn = p.win[f];
        const int K = wn.y - wn.x, N = wn.w - wn.z;
        if (K <= 0 || N <= 0) continue;                                 // an empty window: nothing to write (the whole workgroup agrees)
        const float2 *src = p.cubes + ((f * p.V + p.rx) * (long)S) * C;
        float2 *dst = p.out + p.off[f];
        const int kbase = wn.x - p.row0;                                // the window's first row in the twiddle table
        for (int k0 = 0; k0 < K; k0 += KT) {
            __syncthreads();        // Z and part are free: stage 2 of the chunk (or frame) before has read them; twl is in place
            for (int cb = 0; cb < C; cb += MD_COLS) {
                const int c0 = cb + lane, c1 = c0 + 64;
                const bool v0 = c0 < C, v1 = c1 < C;
                float2 acc[KT][2];
#pragma unroll
                for (int kt = 0; kt < KT; ++kt) acc[kt][0] = acc[kt][1] = make_float2(0.f, 0.f);
#pragma unroll 2
                for (int s = w; s < S; s += 4) {
                    const float2 *row = src + (long)s * C;
                    const float2 x0 = v0 ? row[c0] : make_float2(0.f, 0.f);
                    const float2 x1 = v1 ? row[c1] : make_float2(0.f, 0.f);
                    const float2 *t = p.tw1 + (long)s * p.KP + kbase + k0;
#pragma unroll
                    for (int kt = 0; kt < KT; ++kt) {
                        const float2 tw = t[kt];
                        md_cmac(acc[kt][0], tw, x0);
                        md_cmac(acc[kt][1], tw, x1);
                    }
                }
                if (w) {
#pragma unroll
                    for (int kt = 0; kt < KT; ++kt) {
                        part[((w - 1) * KT + kt) * MD_COLS + lane] = acc[kt][0];
                        part[((w - 1) * KT + kt) * MD_COLS + lane + 64] = acc[kt][1];
                    }
                }
                __syncthreads();
                if (w == 0) {
#pragma unroll
                    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            float2 z = acc[kt][j];
#pragma unroll
                            for (int q = 0; q < 3; ++q) {
                                const float2 pq = part[(q * KT + kt) * MD_COLS + lane + 64 * j];
                                z.x += pq.x;
                                z.y += pq.y;
                            }
                            if (j ? v1 : v0) Z[(size_t)(j ? c1 : c0) * KT + kt] = z;
                        }
                }
                __syncthreads();        // Z of this column block is in place; part is free for the next block
            }
            const int rows = K - k0 < KT ? K - k0 : KT;
            for (int i = threadIdx.x; i < rows * N; i += 256) {
                const int kt = i / N, ci = i - kt * N;
                const int col = wn.z + ci;
                const int k = col >= C / 2 ? col - C / 2 : col + C - C / 2;      // (col + C - C/2) mod C
                int m = 0;
                float2 y = make_float2(0.f, 0.f);
                for (int j = 0; j < C; ++j) {
                    md_cmac(y, Z[(size_t)j * KT + kt], twl[m]);
                    m += k;
                    if (m >= C) m -= C;
                }
                dst[(long)(k0 + kt) * N + ci] = y;
            }
        }
    }
}

}  // namespace mmw
