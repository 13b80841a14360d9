// Translation unit of the vehicle velocity estimator's batched RANSAC (mmw_vehicle_vel.h).  Built with -ffp-contract=off
// (Makefile): H = p / |p| must round as the host's NumPy expression does, and the bands assume one rounding per operation.
#include <cmath>

#include "mmw_ctx.h"
#include "mmw_vehicle_vel.h"

using namespace mmw;

namespace {

// Every argument is judged here, before the context is touched: the function is not given the context, so a refused call cannot
// enqueue anything and needs no device (tests/cpp/vehicle_vel_sanitize.cpp relies on it).
int vv_validate(bool have_ctx, const double *d_points, const int32_t *d_counts, int n_frames, int cap, int dim, int points_per_fit,
                int max_iters, double fit_thresh, int num_close_pts, double static_vel_thresh, const int32_t *d_draws, int n_tab,
                int chain, const double *d_out, const int32_t *d_status, const int32_t *d_flags) {
    MMW_REQUIRE(have_ctx && d_points && d_counts && d_draws && d_out && d_status && d_flags,
                "null argument (ctx %d, d_points %d, d_counts %d, d_draws %d, d_out %d, d_status %d, d_flags %d)", (int)have_ctx,
                d_points != nullptr, d_counts != nullptr, d_draws != nullptr, d_out != nullptr, d_status != nullptr, d_flags != nullptr);
    MMW_REQUIRE(n_frames >= 0 && cap > 0 && n_tab >= 0, "bad extent: n_frames %d, cap %d, n_tab %d", n_frames, cap, n_tab);
    MMW_REQUIRE(dim == 2 || dim == 3, "dim must be 2 or 3, got %d", dim);
    MMW_REQUIRE(points_per_fit >= dim, "points_per_fit %d cannot fit %d coefficients", points_per_fit, dim);
    MMW_REQUIRE(num_close_pts >= points_per_fit, "num_close_pts %d is below points_per_fit %d", num_close_pts, points_per_fit);
    MMW_REQUIRE(max_iters >= 1, "max_iters is %d", max_iters);
    MMW_REQUIRE(std::isfinite(fit_thresh) && std::isfinite(static_vel_thresh), "threshold not finite: fit_thresh %g, static_vel_thresh %g",
                fit_thresh, static_vel_thresh);
    MMW_REQUIRE(chain == 0 || chain == 1, "chain %d is neither 0 (a batch) nor 1 (one chain through the frames)", chain);
    const size_t lds = vehicle_lds_bytes(cap, max_iters);
    if (lds > 160 * 1024)
        return set_error(MMW_ERR_UNSUPPORTED, "vehicle velocity kernel: %d points per frame and %d iterations need %zu bytes of LDS "
                         "(at most 160 KiB): lower the capacity or max_iters", cap, max_iters, lds);
    return MMW_OK;
}

template <int NW> int vv_launch(mmw_ctx *ctx, const VvArgs &a, unsigned grid, size_t lds) {
    if (lds > 64 * 1024)
        MMW_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_vehicle_ransac<NW>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds));         // per device, so on every call
    hipLaunchKernelGGL(k_vehicle_ransac<NW>, dim3(grid), dim3(NW * 64), lds, ctx->stream, a);
    return check_launch("vehicle_ransac");
}

}  // namespace

extern "C" {

int mmw_vehicle_velocity_ransac(mmw_ctx *ctx, const double *d_points, const int32_t *d_counts, int n_frames, int cap, int dim,
                                int points_per_fit, int max_iters, double fit_thresh, int num_close_pts, double static_vel_thresh,
                                const double *d_init, const int32_t *d_draws, int n_tab, int chain, double *d_out, int32_t *d_status,
                                int32_t *d_flags) {
    MMW_TRY(vv_validate(ctx != nullptr, d_points, d_counts, n_frames, cap, dim, points_per_fit, max_iters, fit_thresh, num_close_pts,
                        static_vel_thresh, d_draws, n_tab, chain, d_out, d_status, d_flags));
    if (n_frames == 0) return MMW_OK;
    MMW_JOIN(ctx);
    VvArgs a{};
    a.points = d_points, a.counts = d_counts, a.init = d_init, a.draws = d_draws;
    a.out = d_out, a.status = d_status, a.flags = d_flags;
    a.F = n_frames, a.cap = cap, a.dim = dim, a.ppf = points_per_fit, a.max_iters = max_iters, a.ncp = num_close_pts;
    a.n_tab = n_tab, a.chain = chain;
    a.fit_thr = fit_thresh, a.static_thr = static_vel_thresh;
    const size_t lds = vehicle_lds_bytes(cap, max_iters);
    ProfScope ps(ctx, "vehicle_vel");
    if (chain) return vv_launch<VV_WAVES_CHAIN>(ctx, a, 1u, lds);
    return vv_launch<VV_WAVES_BATCH>(ctx, a, (unsigned)(n_frames < VV_GRID_MAX ? n_frames : VV_GRID_MAX), lds);
}

}  // extern "C"
