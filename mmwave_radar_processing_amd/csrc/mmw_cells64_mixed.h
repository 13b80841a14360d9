// What the dense float64 cell kernels share -- arguments, workgroup constants, LDS sizes, the plan predicate -- and
// k_cells64_mixed<C>, the dense form for the chirp counts other than 128.  Included by mmw_cells64.h (k_cells64<128>, mmw_tu_points.hip)
// and by mmw_tu_cells64.hip, which holds the instantiations of the mixed kernel: nothing here defines a non-template kernel, so
// both translation units can take it.
#pragma once
#include "mmw_ctx.h"
#include "mmw_dft_small.h"

namespace mmw {

struct Cells64Args {
    const float2 *cubes;        // [F][V][S][C] input cube
    const int32_t *dets;        // [F][cap][2] (range bin, fftshifted Doppler index)
    const int32_t *counts;      // [F]
    const int *flagpos;         // [F][cap]: 1 + position in the flagged list (0: not flagged, or beyond dense_cap)
    const int *n_flag;          // flagged evaluations of the call
    int dense_min;              // the dense form runs when *n_flag >= dense_min (the direct kernels when it is below)
    cplx<double> *out;          // [dense_cap][n_ant] float64 cells of the flagged evaluations
    int V, S, cap, n_ant, max_cells;
    AntList ants;
    const double *ws, *wc;      // np.hanning(S), np.hanning(C)
    const cplx<double> *twS, *twC;
};

constexpr int C64_NT = 512, C64_ROWS = 64, C64_PITCH = 137, C64_CELLS = 256, C64_ITEMS = 8 * C64_CELLS / C64_NT;
// LDS: the pass's spectra [64][137], W_S, both windows, the chunk's cells (r << 16 | FFT bin; list position), wave counts
inline size_t cells64_lds(int S, int C, int) {
    return ((size_t)C64_ROWS * C64_PITCH + S) * 16 + ((size_t)S + C) * 8 + (size_t)C64_CELLS * 8 + 64;
}
inline int cells64_max_cells(int S, int C) {        // cells per chunk of a frame (0: the plane's tables do not fit the LDS)
    return C == 128 && cells64_lds(S, C, 0) <= 160 * 1024 - 512 ? C64_CELLS : 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The dense form for planes of OTHER chirp counts: k_cells64_mixed<C>.  None of the reference's shipped cfgs has 128 chirp loops
// (8, 30, 32, 40, 50, 64, 70, 80, 100, 115, 126, 127), so the planes its users run had the direct sums only.  Same arguments,
// chunking of the flagged detections, flagpos lookup and output layout as k_cells64<128>; what differs is the Doppler transform:
//
//   C = R1 * R2, c = n1 + R2 n2: the R2 lanes of a row hold R1 points each.  RegDFT<R1, double> over n2 in registers
//   (mmw_dft_small.h: any small length, built at compile time), the W_C^(n1 k2) twiddles from registers, one exchange through the
//   row's own LDS slab -- element (k2, n) at k2 R2 + (n + k2) mod R2, the rotation that spreads the R2-element runs a lane reads
//   back over the banks as the (n1 + k2) & 7 swizzle of the 128-point kernel does --, then the R1 transforms of length R2
//   (one per k2, bin k = k2 + R1 k1) dealt over the row's lanes: lane n1 takes k2 = n1, n1 + R2, ... < R1.
//
// R2 is 2 .. 16 and mostly no power of two, so rows do not fall on wave boundaries: every exchange phase ends in
// __syncthreads() (the wave-barrier trick of k_cells64<128> needs a row inside one wave).  A pass transforms ROWS = floor(512 / R2) rounded
// down to a multiple of 8 rows; threads past ROWS * R2 sit the transform out, rows past the plane are clamped unconditional
// loads times a zero window.
//
// Pitch: P = (C + 1) | 1 complex128 elements, the smallest ODD pitch above C.  A 16-byte LDS read is served in groups of 16
// lanes, conflict-free when the 16 lanes touch 16 different 16-byte slots of the 256-byte bank row (MI355X: ds_read_b128,
// bank = (a / 4) mod 64).  In the range sums the eight lanes of a cell read the same bin k of rows q, q + 8, ... (q = lane & 7):
// their slots are (q P + k) mod 16, eight different ones exactly when P is odd -- C itself (even for every shipped count) would
// put all eight on TWO slots for C = 8 mod 16 and on ONE for C = 0 mod 16.  The two cells of a 16-lane group then collide at
// most 2-way, by their bins.  The exchange's stores are 8-lane groups over 8 slots (bank mod 32): a row's R2 lanes store R2
// consecutive slots, and neighbouring rows are P apart, odd again.  The 128-point kernel's 137 = 128 + 9 follows the same rule;
// the smallest such pitch keeps every pass below 82 KB (C = 30: 168 rows) and leaves the LDS to W_S of long planes.
//
// Range sums: eight lanes per needed cell as above, lane q owning rows q + 8 t of the pass, so that the twiddle recurrence steps
// by W_S^(8 r); it restarts from the table every 8 steps (the error bound of tests/cells64_mixed_cases.gamma_mixed counts 7).
enum { C64_KIND_NONE = 0, C64_KIND_128 = 1, C64_KIND_MIXED = 2 };

// lanes per row; 0: no instantiation.  R1 = C / R2 points per lane: 4 .. 10 -- with 14 and 16 points per lane (56 = 14 * 4,
// 64 = 16 * 4, 70 = 14 * 5, 80 = 16 * 5, 126 = 14 * 9, 128 = 16 * 8) the samples (2 R1 registers), points (4 R1), twiddles
// (4 R1) and the second level's 4 J2 R2 took all 256 VGPRs and 150 .. 320 bytes of scratch per lane, 20 .. 140 with the
// twiddles in an LDS table; up to 10 points every instantiation is free of scratch (tools/kernel_regs.sh).
// 115 = 5 * 23 would need RegDFT<23> (x[23] + s[11] + d[11] complex128 = 180 VGPRs beside 46 sample registers) and 127 is
// prime: both keep the direct route.
constexpr int c64m_r2(int C) {
    switch (C) {
    case 8: case 10: return 2;
    case 15: case 30: return 3;
    case 32: return 4;
    case 40: case 50: return 5;
    case 56: case 70: return 7;
    case 64: case 80: return 8;
    case 100: return 10;
    case 126: return 14;
    case 128: return 16;
    default: return 0;
    }
}
// shipped chirp counts first, then 128 (through MMW_CELLS64_DENSE_MIXED only: the check against k_cells64<128>) and the
// planes of the tests
#define MMW_CELLS64_MIXED_C(X) X(8) X(30) X(32) X(40) X(50) X(64) X(70) X(80) X(100) X(126) X(128) X(10) X(15) X(56)
constexpr int c64m_rows(int C) { return c64m_r2(C) > 0 ? (C64_NT / c64m_r2(C)) & ~7 : 0; }
constexpr int c64m_pitch(int C) { return (C + 1) | 1; }

struct Cells64Plan {
    int kind, R1, R2, rows, pitch, cells;
    size_t lds;
};
// LDS of the mixed kernel: the pass's spectra [rows][pitch], W_S, both windows, the chunk's cells, wave counts
inline size_t cells64_mixed_lds(int S, int C) {
    return ((size_t)c64m_rows(C) * c64m_pitch(C) + S) * 16 + ((size_t)S + C) * 8 + (size_t)C64_CELLS * 8 + 64;
}
// k_cells64_mixed<C> for this plane (kind NONE: no instantiation, or the tables exceed the LDS); also for C == 128
inline Cells64Plan cells64_mixed_plan(int S, int C) {
    Cells64Plan p{};
    if (S <= 0 || C <= 0 || S > 65535 || c64m_r2(C) == 0) return p;
    const size_t lds = cells64_mixed_lds(S, C);
    if (lds > 160 * 1024 - 512) return p;
    p.kind = C64_KIND_MIXED, p.R2 = c64m_r2(C), p.R1 = C / p.R2, p.rows = c64m_rows(C), p.pitch = c64m_pitch(C);
    p.cells = C64_CELLS, p.lds = lds;
    return p;
}
// which kernel serves the dense refinement of an S x C plane: k_cells64<128> at C == 128 under its own condition, else the mixed one
inline Cells64Plan cells64_plan(int S, int C) {
    if (C != 128) return cells64_mixed_plan(S, C);
    Cells64Plan p{};
    if (S <= 0 || cells64_max_cells(S, C) == 0) return p;
    p.kind = C64_KIND_128, p.R1 = 16, p.R2 = 8, p.rows = C64_ROWS, p.pitch = C64_PITCH, p.cells = C64_CELLS;
    p.lds = cells64_lds(S, C, 0);
    return p;
}

template <int C>
__global__ __launch_bounds__(C64_NT) void k_cells64_mixed(Cells64Args a) {
    constexpr int R2 = c64m_r2(C), R1 = C / R2, ROWS = c64m_rows(C), P = c64m_pitch(C), RPL = ROWS / 8, J2 = (R1 + R2 - 1) / R2;
    static_assert(R2 >= 2 && R1 * R2 == C && R1 <= 10 && ROWS >= 8 && ROWS * R2 <= C64_NT && P > C, "C = R1 * R2: R2 lanes x R1 points per row");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (*a.n_flag < a.dense_min) return;
    const int S = a.S, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n1 = tid % R2, rl = tid / R2;
    const bool rowlane = rl < ROWS;                                     // (threads past the last row of a pass only sum)
    cplx<double> *Z = reinterpret_cast<cplx<double> *>(smem);
    cplx<double> *twS = Z + ROWS * P;
    double *wsl = reinterpret_cast<double *>(twS + S), *wcl = wsl + S;
    unsigned *cell_rk = reinterpret_cast<unsigned *>(wcl + C);
    int *cell_e = reinterpret_cast<int *>(cell_rk + C64_CELLS), *wcnt = cell_e + C64_CELLS;
    const long f = blockIdx.y;
    const int ai = blockIdx.x;
    int n_det = a.counts[f];
    if (n_det > a.cap) n_det = a.cap;
    if (n_det <= 0) return;
    for (int i = tid; i < S; i += C64_NT) {
        twS[i] = a.twS[i];
        wsl[i] = a.ws[i];
    }
    for (int i = tid; i < C; i += C64_NT) wcl[i] = a.wc[i];
    // W_C^(n1 k2), k2 = 1 .. R1 - 1 (n1 k2 < C): the lane's inter-level twiddles, in registers for the whole plane
    cplx<double> tw1[R1];
#pragma unroll
    for (int k2 = 1; k2 < R1; ++k2) tw1[k2] = a.twC[n1 * k2];
    const float2 *plane = a.cubes + (f * a.V + a.ants.idx[ai]) * (long)S * C;
    cplx<double> *slab = Z + (rowlane ? rl : 0) * P;                    // the row's own LDS: (k2, n) rotated first, [k] afterwards
    for (int c0 = 0;; c0 += C64_CELLS) {
        // ---- the chunk's cells: flagged detections with ordinal c0 .. c0 + 255, as in k_cells64<128>
        int running = 0;
        for (int det0 = 0; det0 < n_det; det0 += C64_NT) {
            const int det = det0 + tid;
            const int e = det < n_det ? a.flagpos[f * a.cap + det] - 1 : -1;
            const unsigned long long bal = __ballot(e >= 0);
            if (lane == 0) wcnt[wave] = __popcll(bal);
            __syncthreads();
            int before = running, total = running;
#pragma unroll
            for (int w = 0; w < C64_NT / 64; ++w) {
                const int cw = wcnt[w];
                if (w < wave) before += cw;
                total += cw;
            }
            const int ord = before + __popcll(bal & ((1ull << lane) - 1ull)) - c0;
            if (e >= 0 && ord >= 0 && ord < C64_CELLS) {
                const int r = a.dets[(f * a.cap + det) * 2];
                int k = a.dets[(f * a.cap + det) * 2 + 1] - C / 2;     // FFT bin behind the fftshifted Doppler index: (d - C/2) mod C,
                if (k < 0) k += C;                                      // numpy's fftshift for even and odd C
                if ((unsigned)k >= (unsigned)C) k = 0;                  // (a slot that is no detection must not index past the slab)
                cell_rk[ord] = ((unsigned)r << 16) | (unsigned)k;
                cell_e[ord] = e;
            }
            running = total;
            __syncthreads();
        }
        const int n_cells = running - c0 < C64_CELLS ? running - c0 : C64_CELLS;
        if (n_cells <= 0) break;                                        // (uniform)
        cplx<double> acc[C64_ITEMS];
#pragma unroll
        for (int j = 0; j < C64_ITEMS; ++j) acc[j] = cplx<double>{0.0, 0.0};
        // the samples of the NEXT pass travel while this one is transformed and summed; unconditional clamped loads
        float2 raw[R1];
        auto fetch = [&](int s0) {
            const int s = s0 + (rowlane ? rl : 0), sc = s < S ? s : S - 1;
            const float2 *rowp = plane + (long)sc * C;
#pragma unroll
            for (int n2 = 0; n2 < R1; ++n2) raw[n2] = rowp[n1 + R2 * n2];
        };
        fetch(0);
        for (int s0 = 0; s0 < S; s0 += ROWS) {
            // ---- first level: lane n1 of row rl holds c = n1 + R2 n2; RegDFT over n2, twiddles, rotated store
            if (rowlane) {
                const int s = s0 + rl;
                const double wrow = s < S ? wsl[s] : 0.0;                   // hann(S)[s] rides along; rows past the plane: zero
                cplx<double> x[R1];
#pragma unroll
                for (int n2 = 0; n2 < R1; ++n2) {
                    const double w = wcl[n1 + R2 * n2] * wrow;
                    x[n2] = cplx<double>{(double)raw[n2].x * w, (double)raw[n2].y * w};
                }
                fetch(s0 + ROWS < S ? s0 + ROWS : s0);
                RegDFT<R1, double>::run(x);                                 // natural order: X1[k2] in x[k2]
                int rot = n1;                                               // (n1 + k2) mod R2
                static_for<R1>([&](auto K) {
                    constexpr int k2 = decltype(K)::value;
                    if constexpr (k2 == 0) slab[rot] = x[0];
                    else slab[k2 * R2 + rot] = cmul(x[k2], tw1[k2]);
                    rot = rot + 1 == R2 ? 0 : rot + 1;
                });
            }
            __syncthreads();
            // ---- second level over n1: lane n1 takes k2 = n1 + R2 j (k2 = n1 mod R2, so element n sits at (n + n1) mod R2)
            cplx<double> y[J2][R2];
            if (rowlane) {
                static_for<J2>([&](auto Jj) {
                    constexpr int j = decltype(Jj)::value;
                    const int k2 = n1 + R2 * j, k2c = k2 < R1 ? k2 : 0;    // (clamped into the slab: lanes without a j-th transform --
                                                                            // also j = 0 where R2 > R1 -- read k2 = 0 and write nothing)
                    static_for<R2>([&](auto N) {
                        constexpr int n = decltype(N)::value;
                        const int pos = n + n1 < R2 ? n + n1 : n + n1 - R2;
                        y[j][n] = slab[k2c * R2 + pos];
                    });
                    RegDFT<R2, double>::run(y[j]);
                });
            }
            __syncthreads();
            if (rowlane) {
                static_for<J2>([&](auto Jj) {
                    constexpr int j = decltype(Jj)::value;
                    const int k2 = n1 + R2 * j;
                    if (k2 < R1) static_for<R2>([&](auto K1) { slab[k2 + R1 * decltype(K1)::value] = y[j][decltype(K1)::value]; });
                });
            }
            __syncthreads();
            // ---- range sums of the needed cells over this pass's rows: lane q of a cell owns rows s0 + q + 8 t
#pragma unroll
            for (int j = 0; j < C64_ITEMS; ++j) {
                const int it = tid + j * C64_NT, i = it >> 3, q = it & 7;
                if (i < n_cells) {
                    const unsigned rk = cell_rk[i];
                    const int r = (int)(rk >> 16), k = (int)(rk & 0xffffu);
                    const cplx<double> step = twS[(int)((8L * r) % S)];
                    const cplx<double> *zp = Z + q * P + k;
                    cplx<double> sum = acc[j];
                    for (int t0 = 0; t0 < RPL && s0 + q + 8 * t0 < S; t0 += 8) {       // (rows past the plane hold zeros: skipped)
                        cplx<double> c = twS[(int)(((long)r * (s0 + q + 8 * t0)) % S)];
#pragma unroll
                        for (int t = 0; t < 8; ++t) {
                            if (t0 + t < RPL) {
                                const cplx<double> z = zp[(t0 + t) * 8 * P];
                                sum.x = fma(z.x, c.x, fma(-z.y, c.y, sum.x));
                                sum.y = fma(z.x, c.y, fma(z.y, c.x, sum.y));
                                c = cmul(c, step);
                            }
                        }
                    }
                    acc[j] = sum;
                }
            }
            __syncthreads();
        }
        // ---- the eight parts of a cell sit in adjacent lanes
#pragma unroll
        for (int j = 0; j < C64_ITEMS; ++j) {
            const int it = tid + j * C64_NT, i = it >> 3, q = it & 7;
            cplx<double> s = acc[j];
            for (int d = 1; d < 8; d <<= 1) {
                s.x += __shfl_xor(s.x, d, 64);
                s.y += __shfl_xor(s.y, d, 64);
            }
            if (i < n_cells && q == 0) a.out[(long)cell_e[i] * a.n_ant + ai] = s;
        }
        if (running <= c0 + C64_CELLS) break;                           // (uniform) no further chunk
        __syncthreads();
    }
}

// the launch of k_cells64_mixed<C> (mmw_tu_cells64.hip holds the instantiations); MMW_ERR_UNSUPPORTED without one
int launch_cells64_mixed(mmw_ctx *ctx, const Cells64Args &ca, int C, int n_frames, size_t lds);

}  // namespace mmw
