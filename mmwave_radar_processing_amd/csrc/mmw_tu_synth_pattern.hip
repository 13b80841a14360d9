// Translation unit of the synthetic-array beam patterns (mmw_synth_pattern.h): the magnitude kernel (directions split across
// workgroups, a frame's geometry staged in the LDS), the per-frame normalisation enqueued behind it, and the host-only twin.
#include "mmw_ctx.h"
#include "mmw_synth_pattern.h"

using namespace mmw;

namespace {

// a[t] = float32(|AF[t]|) (and AF[t] itself when af is given) of frame blockIdx.x / ntiles for the SAP_DIRS directions of tile
// blockIdx.x % ntiles.  Thread (q, l) = (tid / SAP_DIRS, tid % SAP_DIRS) sums slice q of direction l: the 32 lanes of a half-wave
// read the same element of P (one LDS broadcast per half), the two halves of a wave different ones.  E of any length: P passes
// through the LDS in chunks of SAP_CHUNK elements, a multiple of SAP_SLICES, so the slices and their order do not depend on it.
// A direction past T is clamped to the last one (its threads take part in the barriers) and not stored.
__global__ __launch_bounds__(SAP_DIRS * SAP_SLICES) void k_sap_magnitudes(const double *__restrict__ P, const double *__restrict__ dirs, int E,
                                                                         int T, int ntiles, double lambda_m, float *__restrict__ mag,
                                                                         double2 *__restrict__ af) {
    __shared__ double Ps[3][SAP_CHUNK];
    __shared__ double part[2][SAP_SLICES][SAP_DIRS];
    constexpr int NT = SAP_DIRS * SAP_SLICES;
    const int tid = threadIdx.x, q = tid / SAP_DIRS, l = tid - q * SAP_DIRS;
    const int frame = blockIdx.x / ntiles, tile = blockIdx.x - frame * ntiles;
    const long t = (long)tile * SAP_DIRS + l, tc = t < T ? t : T - 1;
    const double dx = dirs[tc], dy = dirs[(long)T + tc], dz = dirs[2L * T + tc];
    const double *Pi = P + (long)frame * 3 * E;
    double re = 0.0, im = 0.0;
    for (int e0 = 0; e0 < E; e0 += SAP_CHUNK) {
        const int cnt = E - e0 < SAP_CHUNK ? E - e0 : SAP_CHUNK;
        if (e0) __syncthreads();        // the chunk before has been read
        for (int c = 0; c < 3; ++c)
            for (int j = tid; j < cnt; j += NT) Ps[c][j] = Pi[(long)c * E + e0 + j];
        __syncthreads();
        sap_slice_sum(Ps[0], Ps[1], Ps[2], cnt, q, dx, dy, dz, lambda_m, &re, &im);
    }
    part[0][q][l] = re;
    part[1][q][l] = im;
    __syncthreads();
    if (q != 0 || t >= T) return;
    re = sap_fold(&part[0][0][l], SAP_DIRS);
    im = sap_fold(&part[1][0][l], SAP_DIRS);
    mag[(long)frame * T + t] = (float)hypot(re, im);
    if (af) af[(long)frame * T + t] = make_double2(re, im);
}

// pattern[t] = a[t] / max_t a[t] of frame blockIdx.x, in place.  The maximum is taken in float32 and is a NaN once any a[t] is
// (np.max); a maximum does not depend on the order it is taken in.
__global__ __launch_bounds__(256) void k_sap_normalise(float *__restrict__ pattern, int T) {
    __shared__ float sh[256];
    float *row = pattern + (long)blockIdx.x * T;
    float m = -HUGE_VALF;
    for (int t = threadIdx.x; t < T; t += 256) m = sap_max(m, row[t]);
    sh[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = sap_max(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    m = sh[0];
    for (int t = threadIdx.x; t < T; t += 256) row[t] = row[t] / m;
}

}  // namespace

extern "C" {

int mmw_synth_array_pattern(mmw_ctx *ctx, const double *d_P, int n, int E, const double *h_dirs, int T, double lambda_m, float *d_pattern,
                            void *d_af) {
    MMW_TRY(sap_validate(ctx != nullptr, d_P, n, E, h_dirs, T, lambda_m, d_pattern));
    if (n == 0) return MMW_OK;
    MMW_JOIN(ctx);
    ProfScope ps(ctx, "synth_pattern");
    MMW_TRY(ensure_scratch(ctx, (size_t)3 * T * sizeof(double)));
    double *d_dirs = (double *)ctx->scratch;
    // (a pageable source: the copy is staged before the call returns, the caller's array is free again afterwards)
    MMW_HIP(hipMemcpyAsync(d_dirs, h_dirs, (size_t)3 * T * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    const int ntiles = (T + SAP_DIRS - 1) / SAP_DIRS;          // n ntiles <= n T: inside int32
    hipLaunchKernelGGL(k_sap_magnitudes, dim3((unsigned)((long)n * ntiles)), dim3(SAP_DIRS * SAP_SLICES), 0, ctx->stream, d_P, d_dirs, E, T,
                       ntiles, lambda_m, d_pattern, (double2 *)d_af);
    MMW_TRY(check_launch("sap_magnitudes"));
    hipLaunchKernelGGL(k_sap_normalise, dim3((unsigned)n), dim3(256), 0, ctx->stream, d_pattern, T);
    return check_launch("sap_normalise");
}

// The same accumulation (sap_slice_sum, sap_fold, sap_max of mmw_synth_pattern.h) on host pointers: no device, no context.
int mmw_diag_synth_array_pattern_host(const double *h_P, int n, int E, const double *h_dirs, int T, double lambda_m, float *h_pattern,
                                      void *h_af) {
    MMW_TRY(sap_validate(true, h_P, n, E, h_dirs, T, lambda_m, h_pattern));
    double *af = (double *)h_af;
    for (long i = 0; i < n; ++i) {
        const double *Pi = h_P + i * 3 * E;
        float *row = h_pattern + i * T;
        float m = -HUGE_VALF;
        for (long t = 0; t < T; ++t) {
            double part[2][SAP_SLICES];
            for (int q = 0; q < SAP_SLICES; ++q) {
                part[0][q] = part[1][q] = 0.0;
                sap_slice_sum(Pi, Pi + E, Pi + 2L * E, E, q, h_dirs[t], h_dirs[(long)T + t], h_dirs[2L * T + t], lambda_m, &part[0][q],
                              &part[1][q]);
            }
            const double re = sap_fold(part[0], 1), im = sap_fold(part[1], 1);
            row[t] = (float)std::hypot(re, im);
            m = sap_max(m, row[t]);
            if (af) af[2 * (i * T + t)] = re, af[2 * (i * T + t) + 1] = im;
        }
        for (long t = 0; t < T; ++t) row[t] = row[t] / m;
    }
    return MMW_OK;
}

}  // extern "C"
