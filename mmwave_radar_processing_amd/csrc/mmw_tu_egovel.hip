// Translation unit of the device point clouds and the batched ego-velocity RANSAC (mmw_egovel.h).  Built with
// -ffp-contract=off (Makefile): the point products and H = p / |p| must round as the host's NumPy expressions do.
#include "mmw_ctx.h"
#include "mmw_egovel.h"

using namespace mmw;

extern "C" {

int mmw_point_cloud(mmw_ctx *ctx, const int32_t *d_dets, const int32_t *d_counts, const int32_t *d_az_idx, const int32_t *d_el_idx,
                    const double *d_range_bins, const double *d_vel_bins, const double *d_cos, const double *d_sin,
                    double *d_points, int n_frames, int cap, int S, int C, int A) {
    MMW_REQUIRE(ctx && d_dets && d_counts && d_range_bins && d_vel_bins && d_points, "null argument");
    MMW_REQUIRE((!d_az_idx && !d_el_idx) || (d_cos && d_sin), "angle bins without the cos / sin tables");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_frames >= 0 && n_frames <= 65535 && cap > 0 && S > 0 && C > 0 && A > 0, "bad shape");
    if (n_frames == 0) return MMW_OK;
    PointCloudArgs a{d_dets, d_counts, d_az_idx, d_el_idx, d_range_bins, d_vel_bins, d_cos, d_sin, d_points, cap, S, C, A};
    ProfScope ps(ctx, "egovel");
    hipLaunchKernelGGL(k_point_cloud, dim3((unsigned)((cap + 255) / 256), n_frames), dim3(256), 0, ctx->stream, a);
    return check_launch("point_cloud");
}

int mmw_ego_velocity_ransac(mmw_ctx *ctx, const double *d_points, const int32_t *d_counts, int n_frames, int cap, int dim,
                            double thr, double r2_thr, const int32_t *d_subsets, const int32_t *d_subset_row, int n_rows,
                            const int32_t *d_trials_tab, int tab_len, const int32_t *d_trials_off, double *d_out,
                            int32_t *d_flags, uint8_t *d_inlier_mask) {
    MMW_REQUIRE(ctx && d_points && d_counts && d_subset_row && d_out && d_flags, "null argument");
    MMW_REQUIRE(n_rows == 0 || (d_subsets && d_trials_tab && d_trials_off), "table rows without tables");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_frames >= 0 && n_frames <= 65535 && cap > 0 && n_rows >= 0 && tab_len >= 0, "bad shape");
    MMW_REQUIRE(dim == 2 || dim == 3, "dim must be 2 (standard array) or 3 (ods), got %d", dim);
    MMW_REQUIRE(thr >= 0.0, "negative residual threshold");
    const size_t lds = ego_lds_bytes(cap);
    if (lds > 160 * 1024)
        return set_error(MMW_ERR_UNSUPPORTED, "ego-velocity kernel: %d points per frame need %zu bytes of LDS (at most 160 KiB): "
                         "lower the capacity", cap, lds);
    if (n_frames == 0) return MMW_OK;
    EgoArgs a{d_points, d_counts, d_subsets, d_subset_row, d_trials_tab, d_trials_off, d_out, d_flags, d_inlier_mask,
              cap, dim, n_rows, tab_len, thr, r2_thr};
    if (lds > 64 * 1024)
        MMW_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_ego_ransac), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds));         // per device, so on every call
    ProfScope ps(ctx, "egovel");
    hipLaunchKernelGGL(k_ego_ransac, dim3(n_frames), dim3(256), lds, ctx->stream, a);
    return check_launch("ego_ransac");
}

}  // extern "C"
