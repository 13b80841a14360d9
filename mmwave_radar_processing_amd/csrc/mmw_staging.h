// Kernels that stage data around the FFT chain: synthetic input generation in HBM, the TDM de-interleave, |.|, float32 -> float64
// widening, range-profile averaging, the planes' L1 norms and the HBM-ceiling diagnostic.  (mmw_tu_input.hip)
#pragma once
#include "mmw_ctx.h"

namespace mmw {

// ------------------------------------------------------------------ counter-based RNG
__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ float u01(unsigned long long h) {           // (0, 1]
    return ((float)(h >> 40) + 1.0f) * (1.0f / 16777216.0f);
}

constexpr int SYNTH_MAX_TARGETS = 16;

// One thread per cube element.  Target parameters are re-derived per thread from (seed0 + frame, k)
// so no parameter buffer is needed; values are rounded to integers like a 16-bit ADC.
__global__ __launch_bounds__(256) void k_synth(float2 *cubes, long total, int V, int S, int C,
                                                unsigned long long seed0, int num_targets, float sigma) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total) return;
    const int c = (int)(gid % C);
    const int s = (int)((gid / C) % S);
    const int v = (int)((gid / ((long)C * S)) % V);
    const unsigned long long f = (unsigned long long)(gid / ((long)C * S * V));
    const unsigned long long fs = mix64(seed0 + f);
    float re = 0.f, im = 0.f;
    for (int k = 0; k < num_targets; ++k) {
        const unsigned long long b = mix64(fs ^ (0x1000ull * (k + 1)));
        const float f_r = 0.02f + 0.43f * u01(mix64(b + 1));
        const float f_d = -0.45f + 0.90f * u01(mix64(b + 2));
        const float f_a = -0.40f + 0.80f * u01(mix64(b + 3));
        const float amp = 20.f + 380.f * u01(mix64(b + 4));
        const float phi = u01(mix64(b + 5));
        float ph = f_r * (float)s;
        ph -= floorf(ph);
        float t = f_d * (float)c;
        ph += t - floorf(t);
        t = f_a * (float)v;
        ph += t - floorf(t) + phi;
        ph -= floorf(ph);
        float sn, cs;
        sincospif(2.0f * ph, &sn, &cs);
        re += amp * cs;
        im += amp * sn;
    }
    // noise keyed by (frame seed, element index inside the frame): a frame's bytes do not depend on where in a batch
    // (or on which device of a sharded batch) it is generated
    const unsigned long long e = (unsigned long long)(gid - (long)f * ((long)C * S * V));
    const unsigned long long h = mix64(fs ^ mix64(e * 2 + 0x51ull));
    const float u1 = u01(h), u2 = u01(mix64(h + 7));
    const float rad = sigma * sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincospif(2.0f * u2, &sn, &cs);
    cubes[gid] = make_float2(rintf(re + rad * cs), rintf(im + rad * sn));
}

// raw[F][num_rx][S][num_tx*loops] -> virt[F][num_tx*num_rx][S][loops]; virtual antenna t*num_rx + r
// takes every num_tx-th chirp starting at t (processors/virtual_array_reformater.py:53-63).
__global__ __launch_bounds__(256) void k_reformat(const float2 *raw, float2 *virt, long total,
                                                   int num_rx, int num_tx, int S, int loops) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total) return;
    const int l = (int)(gid % loops);
    const int s = (int)((gid / loops) % S);
    const int va = (int)((gid / ((long)loops * S)) % (num_rx * num_tx));
    const long f = gid / ((long)loops * S * num_rx * num_tx);
    const int t = va / num_rx, r = va % num_rx;
    virt[gid] = raw[((f * num_rx + r) * S + s) * ((long)num_tx * loops) + (long)l * num_tx + t];
}

// The same de-interleave from int16 I/Q samples: raw[F][num_rx][S][num_tx*loops][2] (I, Q) -> complex64 virtual-array cube.
// NO UPSTREAM ORACLE for the sample layout: the reference gets its cubes from the absent cpsl_datasets reader;
// this is "the raw cube mmw_*_raw accepts, with int16 I/Q instead of complex64" -- half the bytes over PCIe and HBM.
__global__ __launch_bounds__(256) void k_reformat_i16(const short2 *raw, float2 *virt, long total, int num_rx, int num_tx, int S,
                                                       int loops) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total) return;
    const int l = (int)(gid % loops);
    const int s = (int)((gid / loops) % S);
    const int va = (int)((gid / ((long)loops * S)) % (num_rx * num_tx));
    const long f = gid / ((long)loops * S * num_rx * num_tx);
    const int t = va / num_rx, r = va % num_rx;
    const short2 v = raw[((f * num_rx + r) * S + s) * ((long)num_tx * loops) + (long)l * num_tx + t];
    virt[gid] = make_float2((float)v.x, (float)v.y);
}

__global__ __launch_bounds__(256) void k_abs_c64(const float2 *in, float *out, size_t n) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (gid < n) {
        const float2 v = in[gid];
        out[gid] = hypotf(v.x, v.y);
    }
}

// float32 -> float64, element by element (complex arrays as pairs): the reference hands back complex128 / float64 arrays,
// and widening 16 MB on one host core (numpy astype, ~5 ms) costs more than moving twice the bytes over PCIe
__global__ __launch_bounds__(256) void k_widen_f32_f64(const float *__restrict__ in, double *__restrict__ out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = (double)in[i];
}

// out[f][s] = mean_v |spec[f][v][s]|   (processors/range_resp.py:55-57; np.mean over axis 0 adds the
// antenna rows in order, which the loop reproduces)
template <typename T>
__global__ __launch_bounds__(256) void k_mean_abs_over_v(const cplx<T> *spec, T *out, int F, int V, int S) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (long)F * S) return;
    const int s = (int)(gid % S);
    const long f = gid / S;
    T acc = (T)0;
    for (int v = 0; v < V; ++v) {
        const cplx<T> x = spec[(f * V + v) * S + s];
        if constexpr (sizeof(T) == 8) acc += hypot(x.x, x.y);
        else acc += hypotf(x.x, x.y);
    }
    out[gid] = acc / (T)V;
}

// ------------------------------------------------------------------ in-situ HBM ceiling (diagnostics)
// mode 0: dst = src (16 B/lane copy)   1: dst = const (write only)   2: read only (sum kept live)
// mode 3: write only, non-temporal   4: write only, 4 stores in flight per lane   5: copy, 4 in flight
typedef float diag_f4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void k_diag_membw(const diag_f4 *src, diag_f4 *dst, size_t n_vec, int mode) {
    const size_t stride = (size_t)gridDim.x * 256;
    const size_t i0 = (size_t)blockIdx.x * 256 + threadIdx.x;
    diag_f4 acc = {0.f, 0.f, 0.f, 0.f};
    const diag_f4 k = {1.f, 2.f, 3.f, 4.f};
    if (mode == 6 || mode == 7) {
        // the angle kernel's store pattern without its arithmetic: every thread owns 16 B of a 256-KiB "plane"
        // and writes the same offset of 64 consecutive planes (mode 7: 4 planes per pass, 16 passes)
        const size_t plane_vec = 16384, frame_vec = 64 * plane_vec;
        const size_t frames = n_vec / frame_vec;
        for (size_t w = (size_t)blockIdx.x * 256 + threadIdx.x; w < frames * plane_vec; w += stride) {
            const size_t f = w / plane_vec, o = w % plane_vec;
            diag_f4 *base = dst + f * frame_vec + o;
#pragma unroll 8
            for (int a = 0; a < 64; ++a) __builtin_nontemporal_store(k, base + (size_t)a * plane_vec);
        }
        return;
    }
    if (mode == 4 || mode == 5) {
        for (size_t i = i0; i + 3 * stride < n_vec; i += 4 * stride) {
            if (mode == 4) {
                dst[i] = k; dst[i + stride] = k; dst[i + 2 * stride] = k; dst[i + 3 * stride] = k;
            } else {
                const diag_f4 a = src[i], b = src[i + stride], c = src[i + 2 * stride], d = src[i + 3 * stride];
                dst[i] = a; dst[i + stride] = b; dst[i + 2 * stride] = c; dst[i + 3 * stride] = d;
            }
        }
        return;
    }
    for (size_t i = i0; i < n_vec; i += stride) {
        if (mode == 0) dst[i] = src[i];
        else if (mode == 1) dst[i] = k;
        else if (mode == 3) __builtin_nontemporal_store(k, dst + i);
        else acc += src[i];
    }
    if (mode == 2 && acc.x + acc.y + acc.z + acc.w == 12345.678f) dst[0] = acc;
}

// l1[plane] = sum over the plane of hann(S)[s] hann(C)[c] (|re| + |im|)  >=  sum |w x|: the scale of the rounding-error
// bound of the float32 range-Doppler cell values (see k_angle_argmax).  One workgroup per plane.
__global__ __launch_bounds__(256) void k_plane_l1(const float2 *__restrict__ in, float *__restrict__ l1, int S, int C,
                                                   const float *__restrict__ ws, const float *__restrict__ wc) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    __shared__ float part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float2 *src = in + (long)blockIdx.x * S * C;
    float acc = 0.f;
    if ((C & 1) == 0) {             // one wave per row, 16-B loads
        const f4 *src4 = reinterpret_cast<const f4 *>(src);
        const int C2 = C >> 1;
        for (int s = wave; s < S; s += 4) {
            float row = 0.f;
            for (int p = lane; p < C2; p += 64) {
                const f4 v = __builtin_nontemporal_load(src4 + (long)s * C2 + p);
                row += wc[2 * p] * (fabsf(v.x) + fabsf(v.y)) + wc[2 * p + 1] * (fabsf(v.z) + fabsf(v.w));
            }
            acc += ws[s] * row;
        }
    } else {
        for (int s = wave; s < S; s += 4) {
            float row = 0.f;
            for (int c = lane; c < C; c += 64) {
                const float2 v = src[(long)s * C + c];
                row += wc[c] * (fabsf(v.x) + fabsf(v.y));
            }
            acc += ws[s] * row;
        }
    }
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) l1[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

}  // namespace mmw
