// Batched synthetic-array beamforming over resident frames (mmw_synth_array):
//   out_i = FFT_S( hann(S) . ( X_i[S,E] x W_i[E,T] ) ),   W_i[e,t] = hamming(E)[e] exp(j 2 pi d_t.p_{i,e} / lambda)
// the contraction of mmw_beamform.h with the operand X_i never materialised: element e = (h, j) of output i is
//   cubes[h_frames[i] - H + 1 + h][v][s][j k],   h < H frames of history, j < Cv = ceil(C / k) chirps, E = H Cv
// (SyntheticArrayBeamformerProcessor keeps H frames of every k-th chirp of one virtual antenna,
// processors/simple_synthetic_array_beamformer_processor_multiFrame.py:818-872).  A row of X_i is H segments of Cv elements,
// one per frame of the window; a window frame before the buffer is all zeros and is never read, while the Hamming taper and the
// geometry still count its elements.  The kernels are those of mmw_beamform.h instantiated with the policy below.
#pragma once
#include "mmw_ctx.h"
#include "mmw_beamform.h"

namespace mmw {

// ------------------------------------------------------------------ the window arithmetic, on the host
inline int sa_cv(int C, int k) { return (C + k - 1) / k; }

// One run of consecutive elements [e0, e0 + n) of a window row cut at the frame boundaries.
struct SaSegment {
    int slot, frame, j0, count;     // window slot h, resident frame (negative: before the buffer), first chirp index j, elements
};
// Segments of the run [e0, e0 + n) (clipped to E) of output frame `frame`.  *first_live: the first resident frame the run reads
// (-1: none).  *vec16: the run may be read with 16-byte loads in EVERY row -- k == 1, one segment, and both the row pitch
// (C * 8 bytes) and the offset in the row (j0 * 8 bytes) multiples of 16.
inline int sa_segments(int C, int k, int H, int frame, int e0, int n, SaSegment *segs, int cap, int *first_live, int *vec16) {
    const int Cv = sa_cv(C, k);
    const long E = (long)H * Cv;
    int n_seg = 0, first = -1;
    long e = e0, end = std::min<long>((long)e0 + n, E);
    while (e < end) {
        const int h = (int)(e / Cv), j0 = (int)(e - (long)h * Cv);
        const int count = (int)std::min<long>(end - e, Cv - j0), fr = frame - H + 1 + h;
        if (fr >= 0 && first < 0) first = fr;
        if (n_seg < cap) segs[n_seg] = SaSegment{h, fr, j0, count};
        ++n_seg;
        e += count;
    }
    if (first_live) *first_live = first;
    if (vec16) *vec16 = (k == 1 && n_seg == 1 && (C & 1) == 0 && n_seg <= cap && (segs[0].j0 & 1) == 0 && (segs[0].count & 1) == 0) ? 1 : 0;
    return n_seg;
}
// every chunk of 32 elements whole, and every run of n elements that starts at a multiple of n inside one frame and 16-byte
// aligned (n is 16 or 8: a multiple of 2, so the offsets in a row are even once Cv is a multiple of n)
inline bool sa_fast(int C, int k, int H, int n) { return k == 1 && C % n == 0 && ((long)H * C) % 32 == 0; }

// ------------------------------------------------------------------ the operand policy of the contraction kernels
struct AWindow {
    static constexpr bool windowed = true;
    const int *frames;              // device, [n_out]: the newest frame of every window
    int v, S, C, k, H, Cv;
    long fs;                        // elements per resident frame, V S C
    bool al16;                      // the cubes start at a multiple of 16 bytes
    struct Row {
        const cplx<float> *p;       // row s of antenna v in resident frame 0
        int w0;                     // resident frame of window slot 0 (negative: before the buffer)
    };
    __device__ __forceinline__ Row row(const cplx<float> *A, long b, int m, long, int) const {
        return Row{A + ((long)v * S + m) * C, frames[b] - H + 1};
    }
    __device__ __forceinline__ Row row_packed(const cplx<float> *A, long b, int m, int, int) const { return row(A, b, m, 0, 0); }
    // a frame before the buffer is never read: the load goes to frame 0 (always resident) and the bit says "mask it"
    template <int N> __device__ __forceinline__ unsigned run(const Row &r, int k0, int K, cplx<float> (&out)[N]) const {
        const int kk = k0 < K ? k0 : K - 1;
        int h = kk / Cv, j = kk - h * Cv;
        unsigned live = 0u;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int fr = r.w0 + h;
            out[i] = r.p[(long)(fr > 0 ? fr : 0) * fs + (long)j * k];
            live |= (unsigned)(fr >= 0) << i;
            if (k0 + i + 1 < K) {                       // (beyond K: stay on the last element, as the clamp of ARows does)
                ++j;
                if (j == Cv) j = 0, ++h;
            }
        }
        return live;
    }
    template <int N> __device__ __forceinline__ void run16(const Row &r, int k0, f32x4 (&out)[N / 2]) const {
        const int h = k0 / Cv, j = k0 - h * Cv, fr = r.w0 + h;          // (k == 1, the run inside one frame: fast())
        const f32x4 *src = reinterpret_cast<const f32x4 *>(r.p + (long)(fr > 0 ? fr : 0) * fs + j);
        const unsigned m = 0u - (unsigned)(fr >= 0);
#pragma unroll
        for (int i = 0; i < N / 2; ++i) {
            const u32x4 bits = __builtin_bit_cast(u32x4, src[i]) & m;
            out[i] = __builtin_bit_cast(f32x4, bits);
        }
    }
    bool fast(int, int n) const { return al16 && sa_fast(C, k, H, n); }
};

// Everything mmw_synth_array needs in device memory besides the cubes sits at the head of the scratch: P, dirs, frames.
inline size_t sa_head_bytes(int n_out, int E, int T) {
    const size_t b = ((size_t)n_out * 3 * E + (size_t)3 * T) * sizeof(double) + (size_t)n_out * sizeof(int);
    return (b + 255) & ~(size_t)255;
}

// Stages P, dirs and the frame list at the head of the scratch, whose first `head` bytes (>= sa_head_bytes) the caller owns.
struct SaStaged {
    double *d_P, *d_dirs;
    int *d_frames;
};
inline int sa_stage(mmw_ctx *ctx, int S, int E, int T, const int *h_frames, int n_out, const double *h_P, const double *h_dirs,
                    size_t head, SaStaged *st) {
    MMW_TRY(ensure_scratch(ctx, head + bartlett_plan(ctx, n_out, S, E, T).bytes));
    double *d_P = (double *)ctx->scratch, *d_dirs = d_P + (size_t)n_out * 3 * E;
    int *d_frames = (int *)(d_dirs + (size_t)3 * T);
    // (pageable sources: the copies are staged before the calls return, the caller's arrays are free again afterwards)
    MMW_HIP(hipMemcpyAsync(d_P, h_P, (size_t)n_out * 3 * E * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    MMW_HIP(hipMemcpyAsync(d_dirs, h_dirs, (size_t)3 * T * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    MMW_HIP(hipMemcpyAsync(d_frames, h_frames, (size_t)n_out * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    *st = SaStaged{d_P, d_dirs, d_frames};
    return MMW_OK;
}

// The contraction with every table already in device memory: d_P [n_out][3][E] may be the staged table or any other.
inline int synth_array_on(mmw_ctx *ctx, const char *family, const void *d_cubes, int V, int S, int C, int v, int k, int H,
                          const int *d_frames, int n_out, const double *d_P, const double *d_dirs, int T, double lambda_m, void *d_out,
                          size_t head) {
    const int Cv = sa_cv(C, k), E = H * Cv;
    const AWindow ap{d_frames, v, S, C, k, H, Cv, (long)V * S * C, ((size_t)d_cubes & 15) == 0};
    return bartlett_on(ctx, ap, family, d_cubes, d_P, d_dirs, d_out, n_out, S, E, T, lambda_m, head);
}

inline int synth_array(mmw_ctx *ctx, const void *d_cubes, int V, int S, int C, int v, int k, int H, const int *h_frames, int n_out,
                       const double *h_P, const double *h_dirs, int T, double lambda_m, void *d_out) {
    const int E = H * sa_cv(C, k);
    const size_t head = sa_head_bytes(n_out, E, T);
    SaStaged st;
    MMW_TRY(sa_stage(ctx, S, E, T, h_frames, n_out, h_P, h_dirs, head, &st));
    return synth_array_on(ctx, "synth_array", d_cubes, V, S, C, v, k, H, st.d_frames, n_out, st.d_P, st.d_dirs, T, lambda_m, d_out, head);
}

// Every argument of mmw_synth_array is judged here, before the context is touched: the function is not given the context, so a
// refused call cannot enqueue anything and needs no device (tests/cpp/synth_array_sanitize.cpp relies on it).
inline int sa_validate(bool have_ctx, const void *d_cubes, int n_resident, int V, int S, int C, int v, int k, int H, const int *h_frames,
                       int n_out, const double *h_P, const double *h_dirs, int T, double lambda_m, const void *d_out) {
    MMW_REQUIRE(have_ctx && d_cubes && h_frames && h_P && h_dirs && d_out,
                "null argument (ctx %d, d_cubes %d, h_frames %d, h_P %d, h_dirs %d, d_out %d)", (int)have_ctx, d_cubes != nullptr,
                h_frames != nullptr, h_P != nullptr, h_dirs != nullptr, d_out != nullptr);
    MMW_REQUIRE(n_resident >= 0 && V > 0 && S > 0 && C > 0, "bad shape: n_resident %d, V %d, S %d, C %d", n_resident, V, S, C);
    MMW_REQUIRE(v >= 0 && v < V, "antenna v %d is not one of [0, %d)", v, V);
    MMW_REQUIRE(k >= 1, "chirp stride k is %d", k);
    MMW_REQUIRE(H >= 1, "window length H is %d", H);
    MMW_REQUIRE(T >= 1, "T is %d steering directions", T);
    MMW_REQUIRE(lambda_m > 0.0, "lambda_m %g is not positive", lambda_m);      // (a NaN fails too)
    MMW_REQUIRE(n_out >= 0 && n_out <= 65535, "n_out %d is not in [0, 65535]", n_out);
    MMW_REQUIRE((long)H * sa_cv(C, k) <= (1L << 24), "window of %d frames x %d chirps is longer than 2^24 elements", H, sa_cv(C, k));
    for (int i = 0; i < n_out; ++i) {
        MMW_REQUIRE(h_frames[i] >= 0 && h_frames[i] < n_resident, "h_frames[%d] = %d is not a resident frame of [0, %d)", i,
                    h_frames[i], n_resident);
        MMW_REQUIRE(i == 0 || h_frames[i] > h_frames[i - 1], "h_frames is not strictly ascending at %d (%d after %d)", i,
                    h_frames[i], h_frames[i - 1]);
    }
    return MMW_OK;
}

}  // namespace mmw
