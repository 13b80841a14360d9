// Host functions that one translation unit of the entry points calls in another.  Each is defined once, with external linkage, in
// the unit named above it; what only one unit uses stays file-local there.  (chain_settle is declared in mmw_ctx.h, beside the
// join_pipe that calls it; mmw_launch.h declares the kernel launchers.)
#pragma once
#include "mmw_ctx.h"
#include "mmw_fft_fused.h"      // RawView

namespace mmw {

// mmwgpu.hip
int env_int(const char *name, int dflt);

// mmw_tu_input.hip
bool fused_rd_ok(int S, int C);
// the fused 256 x 128 range-Doppler kernel runs (range_doppler_impl's first choice)
bool fused_rd_runs(int S, int C);
// the range-Doppler stage touches no scratch: the fused kernel, or a compile-time mixed-radix one (tables only)
bool rd_needs_no_scratch(int S, int C);
// d_l1 != nullptr: also the per-plane L1 norms of the windowed input (mmw_plane_l1)
int range_doppler_impl(mmw_ctx *ctx, const void *d_cubes, void *d_out, void *d_mag_f32, int n_frames, int V, int S, int C,
                       RawView rv = RawView{1, 0}, float *d_l1 = nullptr);
// rounding-error budget of range_doppler_impl's float32 cells on an S x C plane, in units of 2^-24 of the plane's L1 norm
int rd_error_ulps(int S, int C);
int range_doppler_mag64_impl(mmw_ctx *ctx, const void *d_cubes, double *d_mag, int n_frames, int V, int S, int C, int rx_idx);
// bytes of ctx->scratch that call touches (from its start)
size_t rd_mag64_scratch_bytes(mmw_ctx *ctx, int n_frames, int S, int C);
// instantiated there for float and double
template <typename T>
int range_profile_impl(mmw_ctx *ctx, const void *d_cubes, T *d_out, int n_frames, int V, int S, int C, int chirp_idx);
// d_out[f][s] = mean_v |d_spec[f][v][s]| on ctx->stream (k_mean_abs_over_v); instantiated there for float
template <typename T>
int mean_abs_over_v_impl(mmw_ctx *ctx, const void *d_spec, T *d_out, int n_frames, int V, int S);

// mmw_tu_points.hip
// the one-launch float64 |range-Doppler| plane of mmw_cells64.h (k_rd_mag64_256x128): the shape it exists for, and its launch
bool rd_mag64_fused_ok(int S, int C);
int launch_rd_mag64_fused(mmw_ctx *ctx, const void *d_cubes, double *d_mag, int n_frames, int V, int rx_idx);

// mmw_tu_cfar.hip
// the 2-D CFAR of any float64 plane and the ordered compaction of its mask, on ctx->stream (mmw_cfar2d / mmw_compact2d without the join)
int cfar2d_impl(mmw_ctx *ctx, const double *d_X, double *d_thr, double *d_noise, uint8_t *d_mask, int n_frames, int R, int D,
                int kind, int train_r, int train_d, int guard_r, int guard_d, double scale, int k_rank);
int compact2d_impl(mmw_ctx *ctx, const uint8_t *d_mask, int32_t *d_dets, int32_t *d_counts, int n_frames, int R, int D, int cap);

// mmw_tu_chain.hip
int angle_fft_impl(mmw_ctx *ctx, const void *d_rd, void *d_out, int n_frames, int V, int S, int C, int A, int flags);
void sync_slot_forget(mmw_ctx *ctx);

}  // namespace mmw
