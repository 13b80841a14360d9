// Host functions that one translation unit of the entry points calls in another.  Each is defined once, with external linkage, in
// the unit named above it; what only one unit uses stays file-local there.  (chain_settle is declared in mmw_ctx.h, beside the
// join_pipe that calls it; mmw_launch.h declares the kernel launchers.)
#pragma once
#include "mmw_ctx.h"
#include "mmw_fft_fused.h"      // RawView

namespace mmw {

// mmwgpu.hip
int env_int(const char *name, int dflt);

// mmw_tu_misc.hip
bool fused_rd_ok(int S, int C);
// d_l1 != nullptr: also the per-plane L1 norms of the windowed input (mmw_plane_l1)
int range_doppler_impl(mmw_ctx *ctx, const void *d_cubes, void *d_out, void *d_mag_f32, int n_frames, int V, int S, int C,
                       RawView rv = RawView{1, 0}, float *d_l1 = nullptr);
int range_doppler_mag64_impl(mmw_ctx *ctx, const void *d_cubes, double *d_mag, int n_frames, int V, int S, int C, int rx_idx);
// instantiated there for float and double
template <typename T>
int range_profile_impl(mmw_ctx *ctx, const void *d_cubes, T *d_out, int n_frames, int V, int S, int C, int chirp_idx);

// mmw_tu_chain.hip
int angle_fft_impl(mmw_ctx *ctx, const void *d_rd, void *d_out, int n_frames, int V, int S, int C, int A, int flags);
void sync_slot_forget(mmw_ctx *ctx);

}  // namespace mmw
