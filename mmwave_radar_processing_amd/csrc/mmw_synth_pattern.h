// Synthetic-array beam patterns (mmw_synth_array_pattern): the array factor of a geometry with unit signals at
// every element, no taper and no data, per frame i with positions P_i[3][E] and directions d[3][T]:
//   AF[t]      = sum_e exp(j 2 pi d_t . p_e / lambda)                  complex128
//   a[t]       = float32(|AF[t]|)
//   pattern[t] = a[t] / max_t a[t]                                     float32 division, float32 maximum (NaN if any a[t] is)
// -- SyntheticArrayBeamformerProcessor.compute_synthetic_array_pattern
// (processors/simple_synthetic_array_beamformer_processor_multiFrame.py:615-670), a Python double loop over the directions there.
//
// The phase is reduced in cycles before the sine and cosine: t = (d . p) / lambda, t - rint(t) (exact in float64), so positions of
// thousands of wavelengths cost no accuracy.  The sum over the elements of one direction is cut into SAP_SLICES interleaved slices
// (slice q: e = q, q + SAP_SLICES, ...), each summed in ascending e, and the slices are added in ascending q: ONE order, whatever
// the launch shape, so a call repeats bit for bit.  sap_slice_sum below is that accumulation; the kernel calls it with a frame's P
// staged in the LDS, the host-only entry mmw_diag_synth_array_pattern_host with the caller's table.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "mmw_ctx.h"

namespace mmw {

constexpr int SAP_SLICES = 8;           // interleaved slices of the element sum of one direction
constexpr int SAP_DIRS = 32;            // directions per workgroup: SAP_DIRS x SAP_SLICES = 256 threads
constexpr int SAP_CHUNK = 1024;         // elements of P staged in the LDS at a time (3 x 8 KiB)
constexpr double SAP_2PI = 6.283185307179586476925286766559;

// cos and sin of 2 pi f for a reduced phase f in [-0.5, 0.5]
__host__ __device__ inline void sap_cis(double f, double *cs, double *sn) {
#if defined(__HIP_DEVICE_COMPILE__)
    sincospi(2.0 * f, sn, cs);
#else
    *cs = std::cos(SAP_2PI * f);
    *sn = std::sin(SAP_2PI * f);
#endif
}

// Adds the elements e = e0 + q, e0 + q + SAP_SLICES, ... < e0 + count of slice q to (re, im), in ascending e.  px / py / pz point at
// element e0; e0 is a multiple of SAP_SLICES (the chunks of the kernel are), so the slices of a chunk are those of the whole sum.
__host__ __device__ inline void sap_slice_sum(const double *px, const double *py, const double *pz, int count, int q, double dx, double dy,
                                              double dz, double lambda_m, double *re, double *im) {
    double ar = *re, ai = *im;
    for (int e = q; e < count; e += SAP_SLICES) {
        const double t = (dx * px[e] + dy * py[e] + dz * pz[e]) / lambda_m;
        double cs, sn;
        sap_cis(t - rint(t), &cs, &sn);
        ar += cs;
        ai += sn;
    }
    *re = ar, *im = ai;
}

// The slices of one direction added in ascending q: v[0] + v[stride] + ...
__host__ __device__ inline double sap_fold(const double *v, int stride) {
    double s = v[0];
    for (int q = 1; q < SAP_SLICES; ++q) s += v[(long)q * stride];
    return s;
}

// np.max over float32 values: the larger one, and a NaN once either is
__host__ __device__ inline float sap_max(float a, float b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

// Every argument of mmw_synth_array_pattern and of its host-only twin is judged here, before a context is touched: a refused call
// enqueues nothing and needs no device (tests/cpp/synth_array_pattern_sanitize.cpp relies on it).
inline int sap_validate(bool have_ctx, const void *P, int n, int E, const void *dirs, int T, double lambda_m, const void *pattern) {
    MMW_REQUIRE(have_ctx && P && dirs && pattern, "null argument (ctx %d, P %d, dirs %d, pattern %d)", (int)have_ctx, P != nullptr,
                dirs != nullptr, pattern != nullptr);
    MMW_REQUIRE(n >= 0 && E >= 1 && T >= 1, "bad shape: n %d frames, E %d elements, T %d directions", n, E, T);
    MMW_REQUIRE(lambda_m > 0.0 && lambda_m <= DBL_MAX, "lambda_m %g is not a positive finite wavelength", lambda_m);     // (a NaN fails too)
    // (divisions: n x 3 x E of three 31-bit counts does not fit 64 bits)
    MMW_REQUIRE(n == 0 || (T <= INT32_MAX / n && E <= INT32_MAX / 3 / n), "n %d x T %d or n x 3 x E %d is beyond int32", n, T, E);
    return MMW_OK;
}

}  // namespace mmw
