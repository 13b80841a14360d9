// Batched Doppler-azimuth maps (mmw_doppler_azimuth_batch / mmw_doppler_azimuth_zoom_batch): per frame its own range window,
// per call several antenna subsets, all from ONE range(-Doppler) pass over the resident cubes.
//
//   k_dopaz_rmean   angle FFT + |.| + mean over the frame's range rows for one (frame, set): the pruned 8 x 8 DFT of
//                   k_angle64_rmean (mmw_fft_fused.h), its n <= 16 inputs gathered through the set's antenna list from a cube of
//                   all antennas, its rows read from a per-frame table.
//   k_dopaz_finish  adds the partitions of a (frame, set) in a fixed order, scales by 1 / rows of THAT frame, transposes to
//                   out[set][frame][col][angle]; NaN for a frame without rows (np.mean over an empty axis).
//   k_dopaz_zoom    the zoom transform as a direct sum, only on the rows of each frame's window and the antennas some set uses,
//                   each frame with a frequency list of its own; twiddles from the float64 phase, as k_zoom_table makes them.
#pragma once
#include "mmw_ctx.h"

namespace mmw {

constexpr int DOPAZ_MAX_N = 16;                 // antennas of a set
constexpr int DOPAZ_SET_WORDS = DOPAZ_MAX_N + 1; // device table of a set: its antenna indices, then the fftshift offset (32 / 0)
constexpr int DOPAZ_RL = 4;                     // row lanes of a workgroup (256 threads = 64 columns x 4)
constexpr int DOPAZ_PART_ROWS = 32;             // rows a partition takes before a frame gets another one ...
constexpr int DOPAZ_PMAX = 8;                   // ... up to this many

// Partitions of a frame with `rows` rows.  A function of the frame's own row count and of nothing else: the order of its sums
// -- and with it every bit of its result -- does not depend on the batch, the chunk or the other frames' windows.
__host__ __device__ inline int dopaz_parts(int rows) {
    const int p = (rows + DOPAZ_PART_ROWS - 1) / DOPAZ_PART_ROWS;
    return p < 1 ? 1 : (p > DOPAZ_PMAX ? DOPAZ_PMAX : p);
}

struct DopazArgs {
    const cplx<float> *src;     // [nf][planes][rows_alloc][ncols]
    long frame_stride, plane_stride;
    int ncols;                  // columns of a row (C, or M behind the zoom transform)
    const int2 *rows;           // [nf]: the rows [x, y) of the frame inside a plane
    const int *sets;            // [n_sets][DOPAZ_SET_WORDS]
    float *part;                // [nf * n_sets][pmax][64][ncols]
    float *out;                 // [n_sets][F_total][ncols][64], already at the chunk's first frame
    long out_set_stride;        // F_total * ncols * 64
    int n_sets, n, pmax, nf;
    float h[DOPAZ_MAX_N];       // antenna window over the n antennas of a set (ones without)
};

// grid (ceil(ncols / 64), pmax, nf * n_sets).  Slot q = p * DOPAZ_RL + rl of a frame's P * DOPAZ_RL slots takes the rows
// lo + q, lo + q + P * DOPAZ_RL, ...: a window of a few rows is spread over the row lanes of partition 0 instead of queueing on
// one of them.  Partitions p >= P of a frame leave at once and own no partial sums (k_dopaz_finish reads P of them).
// The four row lanes are added through the LDS in the order 0, 1, 2, 3 by lane 0, which stores part[a][c].
template <int VIN>
__global__ __launch_bounds__(256) void k_dopaz_rmean(DopazArgs a) {
    typedef cplx<float> Cx;
    __shared__ float red[DOPAZ_RL - 1][64][64];
    const int col = threadIdx.x & 63, rl = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int c = blockIdx.x * 64 + col;
    const int z = blockIdx.z, f = z / a.n_sets, k = z - f * a.n_sets;
    const int2 rw = a.rows[f];
    const int P = dopaz_parts(rw.y - rw.x), p = blockIdx.y;
    if (p >= P) return;                                     // the whole workgroup
    const bool live = c < a.ncols;
    const int *set = a.sets + k * DOPAZ_SET_WORDS;
    const Cx *src = a.src + (long)f * a.frame_stride + (live ? c : 0);
    float acc[64];
#pragma unroll
    for (int i = 0; i < 64; ++i) acc[i] = 0.f;
    for (int s = rw.x + p * DOPAZ_RL + rl; s < rw.y; s += P * DOPAZ_RL) {
        Cx x[VIN];
#pragma unroll
        for (int v = 0; v < VIN; ++v) {
            x[v] = Cx{0.f, 0.f};
            // the zero ends of a Hann window and the padding beyond n are never loaded
            if (v < a.n && a.h[v] != 0.f && live) x[v] = src[(long)set[v] * a.plane_stride + (long)s * a.ncols] * a.h[v];
        }
        static_for<8>([&](auto K1) {
            constexpr int k1 = decltype(K1)::value;
            Cx zz[8];
            static_for<8>([&](auto N2) {
                constexpr int n2 = decltype(N2)::value;
                Cx y = Cx{0.f, 0.f};
                if constexpr (n2 < VIN) y = x[n2];
                if constexpr (n2 + 8 < VIN) y = y + mul_w<8, k1, float, Cx>(x[n2 + 8]);
                zz[n2] = mul_w<64, n2 * k1, float, Cx>(y);
            });
            RegFFT<8, float, 8, 0, Cx>::run(zz);
            static_for<8>([&](auto K2) {
                constexpr int k2 = decltype(K2)::value;
                const Cx v = zz[bitrev<8>(k2)];
                acc[k1 + 8 * k2] += __builtin_amdgcn_sqrtf(v.x * v.x + v.y * v.y);
            });
        });
    }
    if (rl > 0) {
#pragma unroll
        for (int i = 0; i < 64; ++i) red[rl - 1][i][col] = acc[i];
    }
    __syncthreads();
    if (rl == 0 && live) {
        const int shift_off = set[DOPAZ_MAX_N];
        float *dst = a.part + (((long)z * a.pmax + p) * 64) * a.ncols + c;
#pragma unroll
        for (int i = 0; i < 64; ++i) {
            float t = acc[i];
#pragma unroll
            for (int q = 0; q < DOPAZ_RL - 1; ++q) t += red[q][i][col];
            dst[(long)((i + shift_off) & 63) * a.ncols] = t;
        }
    }
}

__global__ __launch_bounds__(256) void k_dopaz_finish(DopazArgs a) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    const long per_z = 64L * a.ncols;
    if (gid >= per_z * a.nf * a.n_sets) return;
    const int c = (int)(gid % a.ncols), ang = (int)((gid / a.ncols) % 64);
    const int z = (int)(gid / per_z), f = z / a.n_sets, k = z - f * a.n_sets;
    const int2 rw = a.rows[f];
    const int rows = rw.y - rw.x, P = dopaz_parts(rows);
    float acc = 0.f;
    for (int p = 0; p < P; ++p) acc += a.part[(((long)z * a.pmax + p) * 64 + ang) * a.ncols + c];
    a.out[k * a.out_set_stride + ((long)f * a.ncols + c) * 64 + ang] = rows > 0 ? acc / (float)rows : __builtin_nanf("");
}

constexpr int DOPAZ_ZB = 64;        // zoom bins of a workgroup: one per lane
constexpr int DOPAZ_ZR = 4;         // rows a wave carries at once

struct DopazZoomArgs {
    const float2 *rng;          // [nf][V][S][C]: range FFT of the windowed cubes
    const double *freq;         // [nf][M] cycles per chirp, NaN = a bin of zeros
    const int2 *rows;           // [nf]
    const int *ants;            // [U]: the antennas some set uses, ascending
    float2 *out;                // [nf][U][rmax][M]
    int U, V, S, C, n_used, M, rmax;
};

inline size_t dopaz_zoom_lds(int n_used) { return (size_t)n_used * DOPAZ_ZB * sizeof(float2); }

// grid (ceil(M / 64), nf), 256 threads.  The workgroup first builds Z[c][k] = exp(-j 2 pi c f_k) for its 64 bins of this frame's
// list in the LDS (phase reduced in float64; a NaN frequency gives a column of zeros, so its outputs are exactly 0), then every
// wave walks the (antenna, row) pairs of the frame's window four at a time: lane = bin, the row's samples are wave-uniform reads,
// Z a conflict-free LDS read.  Only rows [lo, hi) of the antennas in `ants` are read or written.
__global__ __launch_bounds__(256) void k_dopaz_zoom(DopazZoomArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2 *Z = reinterpret_cast<float2 *>(smem);           // [n_used][DOPAZ_ZB]
    const int f = blockIdx.y, b0 = blockIdx.x * DOPAZ_ZB;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int e = threadIdx.x; e < a.n_used * DOPAZ_ZB; e += 256) {
        const int kk = e & (DOPAZ_ZB - 1), i = e / DOPAZ_ZB;
        float2 t = make_float2(0.f, 0.f);
        if (b0 + kk < a.M) {
            const double fr = a.freq[(long)f * a.M + b0 + kk];
            if (fr == fr) {
                double turns = fr * (double)i;
                turns -= rint(turns);
                double sn, cs;
                sincospi(-2.0 * turns, &sn, &cs);
                t = make_float2((float)cs, (float)sn);
            }
        }
        Z[e] = t;
    }
    __syncthreads();
    const int2 rw = a.rows[f];
    const int nr = rw.y - rw.x, Q = a.U * nr, bin = b0 + lane;
    for (int q0 = w * DOPAZ_ZR; q0 < Q; q0 += 4 * DOPAZ_ZR) {
        const float2 *row[DOPAZ_ZR];
        float2 acc[DOPAZ_ZR];
#pragma unroll
        for (int j = 0; j < DOPAZ_ZR; ++j) {
            const int q = min(q0 + j, Q - 1), u = q / nr, r = q - u * nr;      // (a row past the end re-reads the last one)
            row[j] = a.rng + (((long)f * a.V + a.ants[u]) * a.S + rw.x + r) * a.C;
            acc[j] = make_float2(0.f, 0.f);
        }
        for (int i = 0; i < a.n_used; ++i) {
            const float2 t = Z[i * DOPAZ_ZB + lane];
#pragma unroll
            for (int j = 0; j < DOPAZ_ZR; ++j) {
                const float2 v = row[j][i];
                acc[j].x = fmaf(v.x, t.x, fmaf(-v.y, t.y, acc[j].x));
                acc[j].y = fmaf(v.x, t.y, fmaf(v.y, t.x, acc[j].y));
            }
        }
        if (bin < a.M) {
#pragma unroll
            for (int j = 0; j < DOPAZ_ZR; ++j) {
                const int q = q0 + j;
                if (q < Q) {
                    const int u = q / nr, r = q - u * nr;
                    a.out[(((long)f * a.U + u) * a.rmax + r) * a.M + bin] = acc[j];
                }
            }
        }
    }
}

}  // namespace mmw
