// Range snapshots for the Capon stage (mmw_range_snapshots): the windowed range FFT of the listed antennas, every chirp kept,
//   out[f][i][r - r_lo][k] = sum_s w[s] x[f][rx[i]][s][k] W_S^(r s),   r_lo <= r < r_hi,   W_S = exp(-2 pi j / S),
// written in the [F][V][R][K] order k_capon_sweep (mmw_beamform.h) reads: K contiguous, one row per antenna and range bin.
//
// A resident cube is [F][V][S][C] with the chirps contiguous, so the transform runs down a column of a [S][C] slab.  One
// workgroup owns one (frame, listed antenna, strip of RS_STRIP consecutive chirps); lanes walk the chirp index, so every global
// load and store of a wave covers whole 128-byte runs of consecutive chirps.  float32 arithmetic on tables made in float64 (long
// double) on the host.
//   k_rs_fft    : S = 16 ... 1024, a power of two.  Thread (b, j) runs an R1-point register FFT (RegFFT) on the samples
//                 R2 n1 + j of chirp b, one exchange through the LDS, then R2-point register FFTs -- k_fft_strided's network
//                 (mmw_fft_generic.h) with the window rows picked at the store.
//   k_rs_direct : every other S up to 1024 (the shipped cfgs have 63, 100, 200, 254 ... samples).  The strip's windowed samples
//                 sit in the LDS; thread (b, kq) accumulates the rows r_lo + kq, + 16, ... four at a time, the twiddle of (r, s)
//                 read from the exactly rounded table W_S^m at m = (r s) mod S, stepped in integers.
// DESIGN.md 4.20 has the reasons for two stages (snapshots through HBM / the Infinity Cache) and the figures.
#pragma once
#include "mmw_ctx.h"

namespace mmw {

constexpr int RS_STRIP = 16;            // chirps of a workgroup: 16 x 8 bytes = one 128-byte run per row
constexpr int RS_MAX_S = 1024;
constexpr int RS_DIRECT_ROWS = 4;       // rows a thread of k_rs_direct carries at once (one LDS read of x feeds all of them)

// What a launch needs to find its block's (frame, antenna, strip) and the rows it writes.
struct RsArgs {
    const float2 *cubes;    // [F][V][S][C]
    float2 *out;            // [F][n_out_rx][r_hi - r_lo][C]
    const float2 *tw;       // W_S^m, m < S
    const float *win;       // hann(S) or nullptr
    int V, S, C;
    int strips;             // ceil(C / RS_STRIP)
    int n_out_rx;           // antennas of the whole call (rows of out per frame)
    int i0;                 // position in the call's list of this launch's first antenna
    int r_lo, r_hi;
    AntList ants;           // this launch's antennas; n == 0: antenna i of the cube is antenna i of the list (n_out_rx = V)
    int n_launch;           // antennas of this launch
};

// block -> (frame, position in the list, antenna of the cube, first chirp)
__device__ __forceinline__ void rs_block(const RsArgs &p, long &f, int &i, int &ant, int &c0) {
    const long blk = blockIdx.x;
    const int strip = (int)(blk % p.strips);
    const long fi = blk / p.strips;
    const int il = (int)(fi % p.n_launch);
    f = fi / p.n_launch;
    i = p.i0 + il;
    ant = p.ants.n ? p.ants.idx[il] : i;
    c0 = strip * RS_STRIP;
}

// LDS image of k_rs_fft: R1 blocks (one per k1) of R2 rows of RS_STRIP chirps, each block followed by RS_STRIP unused entries.
// A wave holds four consecutive j.  The second stage reads the entry (k1 = j + R2 q, n2, b) with ds_read_b64 (banks of 4 bytes,
// 64 of them, conflicts counted inside each half of the wave = two consecutive j): without the padding two consecutive k1 are
// 2 R2 RS_STRIP dwords = a multiple of 64 apart -- a two-way conflict on every read; with it they are 32 dwords further apart and
// the 32 lanes cover the 64 banks once.  The first stage writes (k1, j, b) for one k1: 64 consecutive entries, conflict-free
// either way.
constexpr int rs_block_pitch(int R2) { return R2 * RS_STRIP + RS_STRIP; }
constexpr size_t rs_fft_lds_bytes(int R1, int R2) { return (size_t)R1 * rs_block_pitch(R2) * sizeof(float2); }
inline size_t rs_direct_lds_bytes(int S) { return (size_t)S * RS_STRIP * sizeof(float2); }

template <int N, int R1, int R2>
__global__ __launch_bounds__(RS_STRIP *R2) void k_rs_fft(RsArgs p) {
    static_assert(R1 * R2 == N && R1 >= R2 && R1 % R2 == 0, "N = R1*R2, R1 >= R2");
    constexpr int B = RS_STRIP, PITCH = rs_block_pitch(R2);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cplx<float> *lds = reinterpret_cast<cplx<float> *>(smem);
    const int b = threadIdx.x % B, j = threadIdx.x / B;
    long f;
    int i, ant, c0;
    rs_block(p, f, i, ant, c0);
    const int c = c0 + b;
    const bool active = c < p.C;
    const cplx<float> *src = reinterpret_cast<const cplx<float> *>(p.cubes) + ((f * p.V + ant) * (long)N) * p.C + c;
    const cplx<float> *tw = reinterpret_cast<const cplx<float> *>(p.tw);

    cplx<float> a[R1];
#pragma unroll
    for (int n1 = 0; n1 < R1; ++n1) {
        const int n = R2 * n1 + j;
        cplx<float> v = cplx<float>{0.f, 0.f};
        if (active) v = src[(long)n * p.C] * (p.win ? p.win[n] : 1.f);
        a[n1] = v;
    }
    RegFFT<R1, float>::run(a);
    static_for<R1>([&](auto K1) {
        constexpr int k1 = decltype(K1)::value;
        lds[k1 * PITCH + j * B + b] = cmul(a[bitrev<R1>(k1)], tw[j * k1]);
    });
    __syncthreads();
    const int Rw = p.r_hi - p.r_lo;
    cplx<float> *dst = reinterpret_cast<cplx<float> *>(p.out) + ((f * p.n_out_rx + i) * (long)Rw) * p.C + c;
#pragma unroll
    for (int q = 0; q < R1 / R2; ++q) {
        const int k1 = j + R2 * q;
        // the rows of this thread are k1 + R1 k2: none inside the window -> nothing to transform
        const int first = k1 >= p.r_lo ? k1 : k1 + (p.r_lo - k1 + R1 - 1) / R1 * R1;
        if (!active || first >= p.r_hi) continue;
        cplx<float> t[R2];
#pragma unroll
        for (int n2 = 0; n2 < R2; ++n2) t[n2] = lds[k1 * PITCH + n2 * B + b];
        RegFFT<R2, float>::run(t);
        static_for<R2>([&](auto K2) {
            constexpr int k2 = decltype(K2)::value;
            const int k = k1 + R1 * k2;
            if (k >= p.r_lo && k < p.r_hi) dst[(long)(k - p.r_lo) * p.C] = t[bitrev<R2>(k2)];
        });
    }
}

// acc += x t as four fused multiply-adds in a fixed order: a row's sum does not depend on which slot of which thread carries it,
// so a window's rows are the full transform's rows bit for bit
__device__ __forceinline__ void rs_cmac(float2 &acc, const float2 x, const float2 t) {
    acc.x = fmaf(x.x, t.x, acc.x);
    acc.y = fmaf(x.x, t.y, acc.y);
    acc.x = fmaf(-x.y, t.y, acc.x);
    acc.y = fmaf(x.y, t.x, acc.y);
}

__global__ __launch_bounds__(256) void k_rs_direct(RsArgs p) {
    constexpr int B = RS_STRIP, KT = 256 / RS_STRIP, Q = RS_DIRECT_ROWS;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2 *x = reinterpret_cast<float2 *>(smem);      // [S][B], windowed
    const int b = threadIdx.x % B, kq = threadIdx.x / B;
    long f;
    int i, ant, c0;
    rs_block(p, f, i, ant, c0);
    const int c = c0 + b, S = p.S;
    const bool active = c < p.C;
    const float2 *src = p.cubes + ((f * p.V + ant) * (long)S) * p.C + c;
    for (int s = kq; s < S; s += KT) {
        float2 v = make_float2(0.f, 0.f);
        if (active) {
            const float2 xi = src[(long)s * p.C];
            const float w = p.win ? p.win[s] : 1.f;
            v = make_float2(xi.x * w, xi.y * w);
        }
        x[s * B + b] = v;
    }
    __syncthreads();
    if (!active) return;
    const int Rw = p.r_hi - p.r_lo;
    float2 *dst = p.out + ((f * p.n_out_rx + i) * (long)Rw) * p.C + c;
    for (int r0 = p.r_lo + kq; r0 < p.r_hi; r0 += KT * Q) {
        float2 acc[Q];
        int m[Q], step[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            acc[q] = make_float2(0.f, 0.f);
            m[q] = 0;
            const int r = r0 + q * KT;
            step[q] = r < p.r_hi ? r : 0;        // r < S: the index (r s) mod S advances by r and wraps at most once per step
        }
        for (int s = 0; s < S; ++s) {
            const float2 xs = x[s * B + b];
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                rs_cmac(acc[q], xs, p.tw[m[q]]);
                m[q] += step[q];
                if (m[q] >= S) m[q] -= S;
            }
        }
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int r = r0 + q * KT;
            if (r < p.r_hi) dst[(long)(r - p.r_lo) * p.C] = acc[q];
        }
    }
}

}  // namespace mmw
