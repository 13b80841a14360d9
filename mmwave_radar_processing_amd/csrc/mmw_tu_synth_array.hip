// Translation unit of the batched synthetic-array beamformer (mmw_synth_array.h): the contraction kernels of mmw_beamform.h
// instantiated for the windowed operand.
#include "mmw_ctx.h"
#include "mmw_fft_generic.h"
namespace mmw {
extern template int launch_fft_axis<float, float>(mmw_ctx *, FftArgs, int, bool);      // mmw_tu_generic.hip
}
#include "mmw_synth_array.h"

using namespace mmw;

// The contraction for other units (mmw_tu_synth_calib.hip), so that the kernels are instantiated once, here.
namespace mmw {
int synth_array_contract(mmw_ctx *ctx, const char *family, const void *d_cubes, int V, int S, int C, int v, int k, int H, const int *d_frames,
                         int n_out, const double *d_P, const double *d_dirs, int T, double lambda_m, void *d_out, size_t head) {
    return synth_array_on(ctx, family, d_cubes, V, S, C, v, k, H, d_frames, n_out, d_P, d_dirs, T, lambda_m, d_out, head);
}
}  // namespace mmw

extern "C" {

int mmw_synth_array(mmw_ctx *ctx, const void *d_cubes, int n_resident, int V, int S, int C, int v, int k, int H, const int32_t *h_frames,
                    int n_out, const double *h_P, const double *h_dirs, int T, double lambda_m, void *d_out) {
    MMW_TRY(sa_validate(ctx != nullptr, d_cubes, n_resident, V, S, C, v, k, H, h_frames, n_out, h_P, h_dirs, T, lambda_m, d_out));
    if (n_out == 0) return MMW_OK;
    MMW_JOIN(ctx);
    return synth_array(ctx, d_cubes, V, S, C, v, k, H, h_frames, n_out, h_P, h_dirs, T, lambda_m, d_out);
}

// The window arithmetic of mmw_synth_array.h for a run of n elements from e0 of output frame `frame` (no device, no context):
// h_segs gets (slot, frame, j0, count) per segment, up to cap of them; info = {segments, first resident frame read or -1,
// 16-byte loads legal for this run, the tile kernels' fast path legal for runs of n at this (C, k, H)}.
int mmw_diag_synth_array_window(int C, int k, int H, int frame, int e0, int n, int32_t *h_segs, int cap, int32_t info[4]) {
    MMW_REQUIRE(info && C > 0 && k >= 1 && H >= 1 && frame >= 0 && e0 >= 0 && n >= 1 && cap >= 1 && h_segs, "bad argument");
    MMW_REQUIRE((long)H * sa_cv(C, k) <= (1L << 24), "window longer than 2^24 elements");
    std::vector<SaSegment> segs((size_t)cap);
    int first = -1, vec16 = 0;
    const int ns = sa_segments(C, k, H, frame, e0, n, segs.data(), cap, &first, &vec16);
    for (int i = 0; i < ns && i < cap; ++i) {
        h_segs[4 * i] = segs[i].slot;
        h_segs[4 * i + 1] = segs[i].frame;
        h_segs[4 * i + 2] = segs[i].j0;
        h_segs[4 * i + 3] = segs[i].count;
    }
    info[0] = ns;
    info[1] = first;
    info[2] = vec16;
    info[3] = sa_fast(C, k, H, n) ? 1 : 0;
    return MMW_OK;
}

}  // extern "C"
