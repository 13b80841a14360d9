// Batched micro-Doppler rows (mmw_micro_doppler): one row of C floats per frame,
//   out[f][c] = max_{row_lo <= r <= row_hi} | X_f[r][(c + C - C/2) mod C] |,   X_f = FFT_S FFT_C( x[f][rx] ), no window.
//
// MicroDopplerProcessor.process (processors/micro_doppler_resp.py:91-114) takes |fftshift_C(fft2(x[rx]))|, keeps the range rows
// of its window and reduces them with np.max.  Only the K = row_hi - row_lo + 1 rows of the window are ever used, so the
// fast-time transform is a K-row PARTIAL DFT of the antenna's [S][C] slab -- a [K][S] x [S][C] complex product -- and the
// slow-time transform is K direct DFTs of length C -- a [K][C] x [C][C] product.  Both are direct sums in float32, so every S and
// C runs the same code; nothing but the C floats of a frame is written to global memory (DESIGN.md 4.16 has the error argument
// and the measured rates).
#pragma once
#include "mmw_ctx.h"
#include "mmw_md_core.h"

namespace mmw {

// tw[s][kp] = W_S^((row_lo + kp) s), kp < KP (the window padded to whole chunks; the padding rows are valid twiddles of rows
// that the kernel never reduces): the [K][S] factor of the fast-time product, every entry copied from the exactly rounded table
// W_S^m so that no index arithmetic in floating point stands behind a twiddle.
__global__ __launch_bounds__(256) void k_md_twiddle(const float2 *__restrict__ base, float2 *__restrict__ tw, int S, int row_lo,
                                                    int KP) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= (long)S * KP) return;
    const long s = i / KP, r = (row_lo + i % KP) % S;
    tw[i] = base[(r * s) % S];
}

// One workgroup (4 waves) per frame.  The window is walked in chunks of KT rows; per chunk
//   stage 1  Z[kt][c] = sum_s W_S^((lo + k0 + kt) s) x[s][c]: a lane owns columns c0 = cb + lane and c0 + 64 (8-byte loads, 512
//            contiguous bytes per wave instruction), wave w the samples s = w, w + 4, ...; the twiddle of (s, kt) is the same
//            for every lane of a wave (a wave-uniform read of tw1, no LDS traffic).  Waves 1..3 hand their partial sums to wave 0
//            through the LDS, wave 0 adds them in a fixed order and stores Z[c][kt].
//   stage 2  Y[kt][c'] = sum_c Z[kt][c] W_C^(c c'): a lane owns the outputs c' = cb + lane and c' + 64, wave w the rows
//            kt = w KT/4 ... ; Z is a broadcast LDS read, the twiddle a read of W_C at an index stepped by c' (mod C, exact).
//            |Y|^2 of the rows inside the window goes into the running maximum of its column (an LDS atomic max on the bit
//            pattern: non-negative floats order like their bits, and a NaN stays on top as it does in np.max).
// The slab is read once per chunk (K <= KT: once), from L2 after the first pass.  The order of every sum depends on (S, C, K)
// only, so a frame's row does not depend on the batch it is in.
template <int KT>
__global__ __launch_bounds__(256) void k_micro_doppler(const float2 *__restrict__ cubes, const float2 *__restrict__ tw1,
                                                       const float2 *__restrict__ twc, float *__restrict__ out, int V, int S, int C,
                                                       int rx, int K, int KP) {
    constexpr int KW = KT / 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2 *part = reinterpret_cast<float2 *>(smem);                    // [3][KT][MD_COLS]
    float2 *Z = part + 3 * KT * MD_COLS;                                // [C][KT]
    float2 *twl = Z + (size_t)C * KT;                                   // [C]
    unsigned *omax = reinterpret_cast<unsigned *>(twl + C);             // [C]
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long f = blockIdx.x;
    const float2 *src = cubes + ((f * V + rx) * (long)S) * C;
    for (int c = threadIdx.x; c < C; c += 256) {
        twl[c] = twc[c];
        omax[c] = 0u;
    }
    for (int k0 = 0; k0 < K; k0 += KT) {
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
                const float2 *t = tw1 + (long)s * KP + k0;
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
                            const float2 p = part[(q * KT + kt) * MD_COLS + lane + 64 * j];
                            z.x += p.x;
                            z.y += p.y;
                        }
                        if (j ? v1 : v0) Z[(size_t)(j ? c1 : c0) * KT + kt] = z;
                    }
            }
            __syncthreads();        // Z of this column block is in place; part is free for the next block
        }
        for (int cb = 0; cb < C; cb += MD_COLS) {
            const int c0 = cb + lane, c1 = c0 + 64;
            const bool v0 = c0 < C, v1 = c1 < C;
            const int st0 = v0 ? c0 : 0, st1 = v1 ? c1 : 0;
            int m0 = 0, m1 = 0;
            float2 y[KW][2];
#pragma unroll
            for (int q = 0; q < KW; ++q) y[q][0] = y[q][1] = make_float2(0.f, 0.f);
            for (int c = 0; c < C; ++c) {
                const float2 t0 = twl[m0], t1 = twl[m1];
                m0 += st0;
                m1 += st1;
                if (m0 >= C) m0 -= C;
                if (m1 >= C) m1 -= C;
                const float2 *z = Z + (size_t)c * KT + w * KW;
#pragma unroll
                for (int q = 0; q < KW; ++q) {
                    const float2 zq = z[q];
                    md_cmac(y[q][0], zq, t0);
                    md_cmac(y[q][1], zq, t1);
                }
            }
            unsigned b0 = 0u, b1 = 0u;
#pragma unroll
            for (int q = 0; q < KW; ++q)
                if (k0 + w * KW + q < K) {
                    const unsigned u0 = __float_as_uint(fmaf(y[q][0].x, y[q][0].x, y[q][0].y * y[q][0].y)) & 0x7fffffffu;
                    const unsigned u1 = __float_as_uint(fmaf(y[q][1].x, y[q][1].x, y[q][1].y * y[q][1].y)) & 0x7fffffffu;
                    b0 = u0 > b0 ? u0 : b0;
                    b1 = u1 > b1 ? u1 : b1;
                }
            if (v0) atomicMax(&omax[c0], b0);
            if (v1) atomicMax(&omax[c1], b1);
        }
        // no barrier here: Z is next written by wave 0 behind the first barrier of the next chunk, which every wave reaches
        // only after its stage 2
    }
    __syncthreads();
    // bin k of the FFT is column (k + C/2) mod C of np.fft.fftshift, for odd C too
    for (int c = threadIdx.x; c < C; c += 256) out[f * C + (c + C / 2) % C] = sqrtf(__uint_as_float(omax[c]));
}

}  // namespace mmw
