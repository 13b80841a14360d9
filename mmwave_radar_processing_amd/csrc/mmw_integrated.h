// Antenna-integrated (non-coherent) detection plane in float64: P[f][r][d] = sum over an antenna list, in list order, of
// |RD_v[r][d]|^2, RD_v the plane mmw_range_doppler_mag64 is defined on.  No upstream implementation: the
// reference's detectors threshold antenna 0 alone.
//
//   k_rd_pow64_256x128   256 x 128 planes, one launch: the two phases of k_rd_mag64_256x128 (mmw_cells64.h) -- Doppler FFT of the
//                        rows in passes of 64 into the workgroup's own transposed scratch, range FFT down the columns -- inside a
//                        loop over (frame, antenna of the list).  Phase B writes re^2 + im^2 for the first antenna of the list and
//                        adds to the same address for the others: a lane owns the same 64 cells of the plane for every antenna,
//                        so the read-modify-write is the lane's own program order -- no atomics, nothing crosses a workgroup --
//                        and the 256 KB plane stays in the L2 between antennas.
//   k_pow_accum          d_pow (= | +=) mag^2, element-wise: the tail of the per-antenna route on every other shape.
#pragma once
#include "mmw_ctx.h"
#include "mmw_fft.h"
#include "mmw_cells64_mixed.h"      // C64_NT, C64_ROWS, C64_PITCH: the row form of the Doppler phase

namespace mmw {

struct Pow64Args {
    const float2 *cubes;        // [F][V][256][128]
    long frame_stride;          // complex elements between consecutive frames (V * 256 * 128)
    double *pow;                // [F][256][128]
    cplx<double> *scratch;      // [grid][128][256]
    int n_frames;
    AntList ants;               // the list, in summation order
    const double *ws, *wc;      // np.hanning(256), np.hanning(128)
    const cplx<double> *twS, *twC;
};
constexpr int P64_S = 256, P64_C = 128, P64_COLS = 32, P64_CP = 257;
inline size_t pow64_lds() {
    return (std::max((size_t)C64_ROWS * C64_PITCH, (size_t)P64_COLS * P64_CP) + P64_S + P64_C) * 16 + (P64_S + P64_C) * 8;
}
typedef unsigned pow64_u32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(C64_NT) void k_rd_pow64_256x128(Pow64Args a) {
    constexpr int S = P64_S, C = P64_C, P = C64_PITCH;
    static_assert(C64_NT == 512 && C64_ROWS == 64 && C == 8 * 16 && S == 16 * 16, "8 lanes x 16 points per row, 16 x 16 per column");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    cplx<double> *Z = reinterpret_cast<cplx<double> *>(smem);
    cplx<double> *twl = Z + (C64_ROWS * P > P64_COLS * P64_CP ? C64_ROWS * P : P64_COLS * P64_CP);       // W_256
    cplx<double> *twc = twl + S;                                                                          // W_128
    double *wsl = reinterpret_cast<double *>(twc + C), *wcl = wsl + S;
    for (int i = tid; i < S; i += C64_NT) {
        wsl[i] = a.ws[i];
        twl[i] = a.twS[i];
    }
    for (int i = tid; i < C; i += C64_NT) {
        wcl[i] = a.wc[i];
        twc[i] = a.twC[i];
    }
    cplx<double> *T = a.scratch + (size_t)blockIdx.x * S * C;
    const auto t_rs = __builtin_amdgcn_make_buffer_rsrc(T, 0, S * C * 16, 0x00020000);
    __syncthreads();
    for (long f = blockIdx.x; f < a.n_frames; f += gridDim.x) {
        double *out = a.pow + f * (long)S * C;
        for (int ai = 0; ai < a.ants.n; ++ai) {
            const float2 *plane = a.cubes + f * a.frame_stride + (long)a.ants.idx[ai] * S * C;
            // ---- A: Doppler FFT of the rows, 64 at a time; the spectra leave the LDS transposed, T[k][s]
            {
                const int n1 = tid & 7, rl = tid >> 3;
                cplx<double> *slab = Z + rl * P;
                float2 raw[16];
                auto fetch = [&](int s0) {
                    const float2 *rowp = plane + (long)(s0 + rl) * C;
#pragma unroll
                    for (int n2 = 0; n2 < 16; ++n2) raw[n2] = rowp[n1 + 8 * n2];
                };
                fetch(0);
                for (int s0 = 0; s0 < S; s0 += C64_ROWS) {
                    const double wrow = wsl[s0 + rl];
                    cplx<double> x[16];
#pragma unroll
                    for (int n2 = 0; n2 < 16; ++n2) {
                        const double w = wcl[n1 + 8 * n2] * wrow;
                        x[n2] = cplx<double>{(double)raw[n2].x * w, (double)raw[n2].y * w};
                    }
                    fetch(s0 + C64_ROWS < S ? s0 + C64_ROWS : s0);
                    RegFFT<16, double>::run(x);
                    static_for<16>([&](auto K) {
                        constexpr int k2 = decltype(K)::value;
                        const cplx<double> v = x[bitrev<16>(k2)];
                        slab[k2 * 8 + ((n1 + k2) & 7)] = k2 == 0 ? v : cmul(v, twc[(n1 * k2) & (C - 1)]);
                    });
                    __builtin_amdgcn_wave_barrier();
                    cplx<double> ya[8], yb[8];
#pragma unroll
                    for (int n = 0; n < 8; ++n) {
                        ya[n] = slab[n1 * 8 + ((n + n1) & 7)];
                        yb[n] = slab[(n1 + 8) * 8 + ((n + n1) & 7)];
                    }
                    RegFFT<8, double>::run(ya);
                    RegFFT<8, double>::run(yb);
                    __builtin_amdgcn_wave_barrier();
                    static_for<8>([&](auto K) {
                        constexpr int k1 = decltype(K)::value;
                        slab[n1 + 16 * k1] = ya[bitrev<8>(k1)];
                        slab[n1 + 8 + 16 * k1] = yb[bitrev<8>(k1)];
                    });
                    __syncthreads();
#pragma unroll 4
                    for (int i = tid; i < C * C64_ROWS; i += C64_NT) {
                        const int k = i >> 6, r = i & 63;
                        T[k * S + s0 + r] = Z[r * P + k];
                    }
                    __syncthreads();
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // every wave's stores of T have left ...
            __syncthreads();                                         // ... before any wave reads T
            // ---- B: range FFT, 32 columns at a time; cell (r, d) belongs to the same lane for every antenna of the list
            {
                const int m1 = tid & 15, cl = tid >> 4;
                cplx<double> *slab = Z + cl * P64_CP;
                for (int k0 = 0; k0 < C; k0 += P64_COLS) {
                    const int k = k0 + cl;
                    cplx<double> x[16];
#pragma unroll
                    for (int m2 = 0; m2 < 16; ++m2) {
                        // (sc0: the CU's L1 may still hold the previous plane's lines of T)
                        const pow64_u32x4 v = __builtin_bit_cast(
                            pow64_u32x4, __builtin_amdgcn_raw_buffer_load_b128(t_rs, (unsigned)((k * S + m1 + 16 * m2) * 16), 0, 1));
                        x[m2] = __builtin_bit_cast(cplx<double>, v);
                    }
                    RegFFT<16, double>::run(x);
                    static_for<16>([&](auto Q) {
                        constexpr int q = decltype(Q)::value;
                        const cplx<double> v = x[bitrev<16>(q)];
                        slab[q * 16 + ((m1 + q) & 15)] = q == 0 ? v : cmul(v, twl[(m1 * q) & (S - 1)]);
                    });
                    __builtin_amdgcn_wave_barrier();
                    cplx<double> y[16];
#pragma unroll
                    for (int n = 0; n < 16; ++n) y[n] = slab[m1 * 16 + ((n + m1) & 15)];
                    RegFFT<16, double>::run(y);
                    int d = k + C / 2;
                    if (d >= C) d -= C;
                    double *cell = out + (long)m1 * C + d;
                    if (ai == 0) {                                   // (uniform)
                        static_for<16>([&](auto Pp) {
                            constexpr int p = decltype(Pp)::value;
                            const cplx<double> v = y[bitrev<16>(p)];
                            cell[(long)(16 * p) * C] = v.x * v.x + v.y * v.y;
                        });
                    } else {
                        double prev[16];
#pragma unroll
                        for (int p = 0; p < 16; ++p) prev[p] = cell[(long)(16 * p) * C];
                        static_for<16>([&](auto Pp) {
                            constexpr int p = decltype(Pp)::value;
                            const cplx<double> v = y[bitrev<16>(p)];
                            cell[(long)(16 * p) * C] = prev[p] + (v.x * v.x + v.y * v.y);
                        });
                    }
                    __builtin_amdgcn_wave_barrier();                // (the column's slab is reused by the same lanes in the next round)
                }
            }
            __syncthreads();                                         // the LDS goes back to phase A
        }
    }
}

// pow[i] = mag[i]^2 (first) or pow[i] + mag[i]^2: one antenna's |RD| plane joins the sum (launched per antenna, in list order)
__global__ __launch_bounds__(256) void k_pow_accum(const double *__restrict__ mag, double *__restrict__ pow, size_t n, int first) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const double m = mag[i];
        pow[i] = first ? m * m : pow[i] + m * m;
    }
}

}  // namespace mmw
