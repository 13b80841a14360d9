// Translation unit of the beamformers and of the MFMA peak diagnostic (mmw_beamform.h).
#include "mmw_ctx.h"
#include "mmw_launch.h"     // before mmw_beamform.h: its axis FFTs link to mmw_tu_generic.hip's instances
#include "mmw_beamform.h"

#include <cmath>

using namespace mmw;

extern "C" {

// ------------------------------------------------------------------ beamformers
int mmw_bartlett(mmw_ctx *ctx, const void *d_X, const double *d_P, const double *d_dirs, void *d_out, int n_frames, int S,
                 int E, int T, double lambda_m) {
    MMW_REQUIRE(ctx && d_X && d_P && d_dirs && d_out, "null argument");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_frames >= 0 && n_frames <= 65535 && S > 0 && E > 0 && T > 0 && lambda_m > 0, "bad shape");
    if (n_frames == 0) return MMW_OK;
    return bartlett(ctx, d_X, d_P, d_dirs, d_out, n_frames, S, E, T, lambda_m);
}

int mmw_capon(mmw_ctx *ctx, const void *d_X, const double *h_thetas, float *d_out, int n_frames, int V, int R, int K,
              int T, double delta) {
    MMW_REQUIRE(ctx && d_X && h_thetas && d_out, "null argument");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_frames >= 0 && V > 0 && V <= 16 && R > 0 && K > 0 && T > 0, "bad shape (V <= 16)");
    MMW_REQUIRE(delta >= 0.0 && std::isfinite(delta), "diagonal loading %g is not a finite number >= 0", delta);
    if (n_frames == 0) return MMW_OK;
    return capon(ctx, d_X, h_thetas, d_out, n_frames, V, R, K, T, delta);
}

int mmw_diag_mfma_peak(mmw_ctx *ctx, int kind, double *tflops) {
    MMW_REQUIRE(ctx && tflops && kind >= 0 && kind <= 7, "bad argument");
    MMW_JOIN(ctx);
    MMW_TRY(ensure_scratch(ctx, 256));
    // kinds 4 / 5: kinds 2 / 3 (vector FMAs between the MFMAs) with ONE wave per SIMD
    // kinds 6 / 7: v_mfma_f32_32x32x16_bf16 alone / with 8 float32 FMAs after every MFMA (two waves per SIMD)
    const int iters = 1 << 15, wgs = ctx->num_cu * (kind == 4 || kind == 5 ? 1 : 2);            // 8 waves per CU = 2 per SIMD
    if (kind == 4 || kind == 5) kind -= 2;
    hipLaunchKernelGGL(k_diag_mfma, dim3(wgs), dim3(256), 0, ctx->stream, (float *)ctx->scratch, 256, kind);    // warm-up
    MMW_HIP(hipEventRecord(ctx->t0, ctx->stream));
    hipLaunchKernelGGL(k_diag_mfma, dim3(wgs), dim3(256), 0, ctx->stream, (float *)ctx->scratch, iters, kind);
    MMW_TRY(check_launch("diag_mfma"));
    MMW_HIP(hipEventRecord(ctx->t1, ctx->stream));
    MMW_HIP(hipEventSynchronize(ctx->t1));
    float ms = 0.f;
    MMW_HIP(hipEventElapsedTime(&ms, ctx->t0, ctx->t1));
    const double flops_per_mfma = kind >= 6 ? 2.0 * 32 * 32 * 16 : kind != 1 ? 2.0 * 32 * 32 * 2 : 2.0 * 16 * 16 * 4;
    *tflops = (double)wgs * 4 * iters * 4 * flops_per_mfma / (ms * 1e-3) / 1e12;
    return MMW_OK;
}

}  // extern "C"
