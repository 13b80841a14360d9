// Translation unit of the batched synthetic-array beamformer (mmw_synth_array.h): the contraction kernels of mmw_beamform.h
// instantiated for the windowed operand.
#include "mmw_ctx.h"
#include "mmw_fft_generic.h"
namespace mmw {
extern template int launch_fft_axis<float, float>(mmw_ctx *, FftArgs, int, bool);      // mmw_tu_generic.hip
}
#include "mmw_synth_array.h"

using namespace mmw;

// Every argument is judged here, before the context is touched: the function is not given the context, so a refused call cannot
// enqueue anything and needs no device (tests/cpp/synth_array_sanitize.cpp relies on it).
static int sa_validate(bool have_ctx, const void *d_cubes, int n_resident, int V, int S, int C, int v, int k, int H, const int *h_frames,
                       int n_out, const double *h_P, const double *h_dirs, int T, double lambda_m, const void *d_out) {
    MMW_REQUIRE(have_ctx && d_cubes && h_frames && h_P && h_dirs && d_out,
                "null argument (ctx %d, d_cubes %d, h_frames %d, h_P %d, h_dirs %d, d_out %d)", (int)have_ctx, d_cubes != nullptr,
                h_frames != nullptr, h_P != nullptr, h_dirs != nullptr, d_out != nullptr);
    MMW_REQUIRE(n_resident >= 0 && V > 0 && S > 0 && C > 0, "bad shape: n_resident %d, V %d, S %d, C %d", n_resident, V, S, C);
    MMW_REQUIRE(v >= 0 && v < V, "antenna v %d is not one of [0, %d)", v, V);
    MMW_REQUIRE(k >= 1, "chirp stride k is %d", k);
    MMW_REQUIRE(H >= 1, "window length H is %d", H);
    MMW_REQUIRE(T >= 1, "T is %d steering directions", T);
    MMW_REQUIRE(lambda_m > 0.0, "lambda_m %g is not positive", lambda_m);      // (a NaN fails too)
    MMW_REQUIRE(n_out >= 0 && n_out <= 65535, "n_out %d is not in [0, 65535]", n_out);
    MMW_REQUIRE((long)H * sa_cv(C, k) <= (1L << 24), "window of %d frames x %d chirps is longer than 2^24 elements", H, sa_cv(C, k));
    for (int i = 0; i < n_out; ++i) {
        MMW_REQUIRE(h_frames[i] >= 0 && h_frames[i] < n_resident, "h_frames[%d] = %d is not a resident frame of [0, %d)", i,
                    h_frames[i], n_resident);
        MMW_REQUIRE(i == 0 || h_frames[i] > h_frames[i - 1], "h_frames is not strictly ascending at %d (%d after %d)", i,
                    h_frames[i], h_frames[i - 1]);
    }
    return MMW_OK;
}

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
