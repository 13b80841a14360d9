// Translation unit of the Doppler-azimuth velocity estimator's RANSAC stage (mmw_dopaz_velocity.h).
#include <algorithm>
#include <climits>

#include "mmw_ctx.h"
#include "mmw_dopaz_velocity.h"

using namespace mmw;

namespace {

// Every argument is judged here, before the context is touched: the function is not given the context, so a refused call cannot
// enqueue anything and needs no device (tests/cpp/doppler_azimuth_velocity_sanitize.cpp relies on it).
int dzv_validate(bool need_ctx, bool have_ctx, const int32_t *row_peak, const int32_t *zero, int G, int F, int n_rows,
                 const int32_t *h_m, const double *vel, int vel_len, int vel_per_frame, const double *cos_t, const double *sin_t,
                 const double *theta, int n_cols, const int32_t *subsets, const int32_t *trials, int n_tab, int trials_len, int g_az,
                 int g_el, int mode, double thr_standard, double thr_small_vx, double min_R2, double min_inlier_share,
                 const double *out, const int32_t *flags) {
    MMW_REQUIRE((have_ctx || !need_ctx) && row_peak && zero && vel && cos_t && sin_t && theta && subsets && trials && out && flags,
                "null argument (ctx %d, row_peak %d, zero %d, vel %d, cos %d, sin %d, theta %d, subsets %d, trials %d, out %d, flags %d)",
                (int)(have_ctx || !need_ctx), row_peak != nullptr, zero != nullptr, vel != nullptr, cos_t != nullptr,
                sin_t != nullptr, theta != nullptr, subsets != nullptr, trials != nullptr, out != nullptr, flags != nullptr);
    MMW_REQUIRE(G >= 0 && F >= 0 && n_rows >= 0 && vel_len >= 0 && n_tab >= 0 && trials_len >= 0,
                "negative count: G %d, F %d, n_rows %d, vel_len %d, n_tab %d, trials_len %d", G, F, n_rows, vel_len, n_tab, trials_len);
    MMW_REQUIRE(n_cols >= 1, "n_cols is %d angle columns", n_cols);
    MMW_REQUIRE(vel_per_frame == 0 || vel_per_frame == 1, "vel_per_frame %d is neither 0 (one table) nor 1 (one per frame)",
                vel_per_frame);
    MMW_REQUIRE((mode & ~MMW_DOPAZ_RANSAC_VX_ONLY) == 0, "mode %d holds bits other than MMW_DOPAZ_RANSAC_VX_ONLY", mode);
    MMW_REQUIRE(std::isfinite(thr_standard) && std::isfinite(thr_small_vx) && std::isfinite(min_R2) && std::isfinite(min_inlier_share),
                "threshold not finite: thr_standard %g, thr_small_vx %g, min_R2 %g, min_inlier_share %g", thr_standard, thr_small_vx,
                min_R2, min_inlier_share);
    if (G > 0) {
        MMW_REQUIRE(g_az >= 0 && g_az < G, "g_az %d is not a group of [0, %d)", g_az, G);
        MMW_REQUIRE(g_el >= -1 && g_el < G, "g_el %d is neither -1 nor a group of [0, %d)", g_el, G);
    }
    for (int f = 0; h_m && f < F; ++f) MMW_REQUIRE(h_m[f] >= 0 && h_m[f] <= n_rows, "frame %d: m is %d rows of %d", f, h_m[f], n_rows);
    MMW_REQUIRE(vel_len >= n_rows, "a velocity table of %d entries does not serve %d rows", vel_len, n_rows);
    const int need_tab = n_rows >= DZV_MIN_SAMPLES ? n_rows - DZV_MIN_SAMPLES + 1 : 0;
    MMW_REQUIRE(n_tab >= need_tab, "subset tables for %d point counts do not serve n_rows %d (N = 10 .. %d: %d)", n_tab, n_rows, n_rows,
                need_tab);
    MMW_REQUIRE((double)G * F * std::max(n_rows, 4) <= (double)INT_MAX && (double)F * vel_len <= (double)INT_MAX &&
                    (double)n_tab * DZV_TRIALS * DZV_MIN_SAMPLES <= (double)INT_MAX,
                "%d groups x %d frames x %d rows (velocity tables of %d, %d subset tables) do not fit a 32-bit element index", G, F, n_rows,
                vel_len, n_tab);
    MMW_REQUIRE((long)trials_len >= dzv_trials_off(DZV_MIN_SAMPLES + n_tab),
                "a trial table of %d entries does not hold the caps of N = 10 .. %d (%ld entries)", trials_len,
                DZV_MIN_SAMPLES + n_tab - 1, dzv_trials_off(DZV_MIN_SAMPLES + n_tab));
    if (n_rows > MMW_DOPAZ_RANSAC_MAX_ROWS)
        return set_error(MMW_ERR_UNSUPPORTED, "the Doppler-azimuth RANSAC holds a pair's rows in one wavefront: n_rows %d is beyond %d",
                         n_rows, MMW_DOPAZ_RANSAC_MAX_ROWS);
    return MMW_OK;
}

size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

DzvArgs dzv_args(const int32_t *row_peak, const int32_t *zero, int G, int F, int n_rows, const int32_t *m, const double *vel,
                 int vel_len, int vel_per_frame, const double *cos_t, const double *sin_t, const double *theta, int n_cols,
                 const int32_t *subsets, const int32_t *trials, int n_tab, int g_az, int g_el, int mode, double thr_standard,
                 double thr_small_vx, double min_R2, double min_inlier_share, double *out, int32_t *flags) {
    DzvArgs a{};
    a.row_peak = row_peak, a.zero = zero, a.m = m;
    a.vel = vel, a.vel_frame_stride = vel_per_frame ? vel_len : 0;
    a.cos_t = cos_t, a.sin_t = sin_t, a.theta = theta;
    a.subsets = subsets, a.trials = trials;
    a.G = G, a.F = F, a.n_rows = n_rows, a.n_cols = n_cols, a.n_tab = n_tab, a.g_az = g_az, a.g_el = g_el, a.mode = mode;
    a.thr_standard = thr_standard, a.thr_small_vx = thr_small_vx, a.r2_thr = min_R2, a.share_thr = min_inlier_share;
    a.out = out, a.flags = flags;
    return a;
}

}  // namespace

extern "C" {

int mmw_doppler_azimuth_ransac(mmw_ctx *ctx, const int32_t *d_row_peak, const int32_t *d_zero, int G, int F, int n_rows,
                               const int32_t *h_m, const double *d_vel, int vel_len, int vel_per_frame, const double *d_cos,
                               const double *d_sin, const double *d_theta, int n_cols, const int32_t *d_subsets,
                               const int32_t *d_trials, int n_tab, int trials_len, int g_az, int g_el, int mode,
                               double thr_standard, double thr_small_vx, double min_R2, double min_inlier_share, double *d_out,
                               int32_t *d_flags) {
    MMW_TRY(dzv_validate(true, ctx != nullptr, d_row_peak, d_zero, G, F, n_rows, h_m, d_vel, vel_len, vel_per_frame, d_cos, d_sin,
                         d_theta, n_cols, d_subsets, d_trials, n_tab, trials_len, g_az, g_el, mode, thr_standard, thr_small_vx, min_R2,
                         min_inlier_share, d_out, d_flags));
    if (F == 0 || G == 0) return MMW_OK;
    MMW_JOIN(ctx);
    ProfScope ps(ctx, "dopaz_ransac");
    const int32_t *d_m = nullptr;
    if (h_m) {                                          // the one host table of this call -> the head of the scratch
        const size_t m_bytes = (size_t)F * sizeof(int32_t);
        MMW_TRY(ensure_scratch(ctx, up256(m_bytes)));
        MMW_HIP(hipMemcpyAsync(ctx->scratch, h_m, m_bytes, hipMemcpyHostToDevice, ctx->stream));
        MMW_HIP(hipStreamSynchronize(ctx->stream));     // the table is host memory of this call
        d_m = (const int32_t *)ctx->scratch;
    }
    const DzvArgs a = dzv_args(d_row_peak, d_zero, G, F, n_rows, d_m, d_vel, vel_len, vel_per_frame, d_cos, d_sin, d_theta, n_cols,
                               d_subsets, d_trials, n_tab, g_az, g_el, mode, thr_standard, thr_small_vx, min_R2, min_inlier_share,
                               d_out, d_flags);
    const long pairs = (long)G * F;
    hipLaunchKernelGGL(k_dopaz_ransac, dim3((unsigned)((pairs + 3) / 4)), dim3(256), dopaz_ransac_lds(n_rows), ctx->stream, a);
    return check_launch("dopaz_ransac");
}

int mmw_diag_doppler_azimuth_ransac_host(const int32_t *h_row_peak, const int32_t *h_zero, int G, int F, int n_rows,
                                         const int32_t *h_m, const double *h_vel, int vel_len, int vel_per_frame,
                                         const double *h_cos, const double *h_sin, const double *h_theta, int n_cols,
                                         const int32_t *h_subsets, const int32_t *h_trials, int n_tab, int trials_len, int g_az,
                                         int g_el, int mode, double thr_standard, double thr_small_vx, double min_R2,
                                         double min_inlier_share, double *h_out, int32_t *h_flags) {
    MMW_TRY(dzv_validate(false, false, h_row_peak, h_zero, G, F, n_rows, h_m, h_vel, vel_len, vel_per_frame, h_cos, h_sin, h_theta,
                         n_cols, h_subsets, h_trials, n_tab, trials_len, g_az, g_el, mode, thr_standard, thr_small_vx, min_R2,
                         min_inlier_share, h_out, h_flags));
    const DzvArgs a = dzv_args(h_row_peak, h_zero, G, F, n_rows, h_m, h_vel, vel_len, vel_per_frame, h_cos, h_sin, h_theta, n_cols,
                               h_subsets, h_trials, n_tab, g_az, g_el, mode, thr_standard, thr_small_vx, min_R2, min_inlier_share,
                               h_out, h_flags);
    std::vector<double> list((size_t)2 * std::max(n_rows, 1));
    for (int g = 0; g < G; ++g)
        for (int f = 0; f < F; ++f) dzv_pair(DzvWaveHost{}, a, g, f, list.data(), list.data() + std::max(n_rows, 1));
    return MMW_OK;
}

}  // extern "C"
