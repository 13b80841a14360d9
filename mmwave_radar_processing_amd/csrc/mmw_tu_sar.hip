// Translation unit of the strip-map SAR slices (mmw_sar.h).
#include "mmw_ctx.h"
#include "mmw_sar.h"

#include <algorithm>

using namespace mmw;

static size_t sar_up256(size_t b) { return (b + 255) & ~(size_t)255; }

template <int KT>
static int launch_sar_slices(mmw_ctx *ctx, const SarArgs &a) {
    const size_t lds = md_lds_bytes(KT, a.C);
    if (lds > 64 * 1024)
        MMW_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_sar_slices<KT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds));         // per device, so on every call
    const unsigned grid = (unsigned)std::min(a.n_frames, SAR_GRID_MAX);
    hipLaunchKernelGGL(k_sar_slices<KT>, dim3(grid), dim3(256), lds, ctx->stream, a);
    return check_launch("sar_slices");
}

// Every argument is judged here, before the context is touched: the function is not given the context, so a refused call cannot
// enqueue anything and needs no device (tests/cpp/sar_range_sanitize.cpp relies on it).  rows[2]: the union of the row windows of
// the frames that write something (rows[0] > rows[1]: there is none).
static int sar_validate(bool have_ctx, const void *d_cubes, int n_frames, int V, int S, int C, int rx_idx, const int32_t *h_win,
                        const int64_t *h_off, const void *d_out, int rows[2]) {
    MMW_REQUIRE(have_ctx && d_cubes && h_win && h_off && d_out, "null argument (ctx %d, d_cubes %d, h_win %d, h_off %d, d_out %d)",
                (int)have_ctx, d_cubes != nullptr, h_win != nullptr, h_off != nullptr, d_out != nullptr);
    MMW_REQUIRE(n_frames >= 0, "n_frames is %d", n_frames);
    MMW_REQUIRE(V > 0 && S > 0 && C > 0, "bad shape: V %d, S %d, C %d must all be positive", V, S, C);
    MMW_REQUIRE(rx_idx >= 0 && rx_idx < V, "rx_idx %d is not an antenna of [0, %d)", rx_idx, V);
    MMW_REQUIRE(h_off[0] == 0, "h_off[0] is %lld, the first block starts at 0", (long long)h_off[0]);
    rows[0] = S, rows[1] = 0;
    for (int f = 0; f < n_frames; ++f) {
        const int32_t *w = h_win + 4 * (size_t)f;
        MMW_REQUIRE(w[0] >= 0 && w[0] <= w[1] && w[1] <= S, "frame %d: rows [%d, %d) are reversed or leave [0, %d]", f, w[0], w[1], S);
        MMW_REQUIRE(w[2] >= 0 && w[2] <= w[3] && w[3] <= C, "frame %d: columns [%d, %d) are reversed or leave [0, %d]", f, w[2], w[3], C);
        const int64_t area = (int64_t)(w[1] - w[0]) * (w[3] - w[2]);
        // compared as written, without a subtraction that could overflow on hostile offsets
        MMW_REQUIRE(h_off[f] >= 0 && h_off[f] <= INT64_MAX - area && h_off[f + 1] == h_off[f] + area,
                    "frame %d: h_off steps from %lld to %lld, the window holds %lld elements", f, (long long)h_off[f],
                    (long long)h_off[f + 1], (long long)area);
        if (area) rows[0] = std::min(rows[0], (int)w[0]), rows[1] = std::max(rows[1], (int)w[1]);
    }
    return MMW_OK;
}

extern "C" {

int mmw_sar_slices(mmw_ctx *ctx, const void *d_cubes, int n_frames, int V, int S, int C, int rx_idx, const int32_t *h_win,
                   const int64_t *h_off, void *d_out) {
    int rows[2];
    MMW_TRY(sar_validate(ctx != nullptr, d_cubes, n_frames, V, S, C, rx_idx, h_win, h_off, d_out, rows));
    if (n_frames == 0) return MMW_OK;
    const int Kmax = std::max(rows[1] - rows[0], 1);
    const int KT = md_pick_kt(Kmax, C, opt_int(ctx, "MMW_SAR_KT", 0));
    if (!KT)
        return set_error(MMW_ERR_UNSUPPORTED, "SAR slice kernel: %d chirps need %zu bytes of LDS with 4 rows in flight (at most 160 KiB, "
                         "3444 chirps)", C, md_lds_bytes(4, C));
    if (rows[0] >= rows[1]) return MMW_OK;          // every window is empty: nothing to write
    MMW_JOIN(ctx);
    const int KP = rows[1] - rows[0] + KT;          // the union plus the padding of a last chunk
    const float2 *tws = nullptr, *twc = nullptr;
    MMW_TRY(get_table<float>(ctx, TAB_TWIDDLE, S, (const void **)&tws));
    MMW_TRY(get_table<float>(ctx, TAB_TWIDDLE, C, (const void **)&twc));
    const size_t tw_bytes = sar_up256((size_t)S * KP * sizeof(float2)), win_bytes = sar_up256((size_t)n_frames * sizeof(int4));
    MMW_TRY(ensure_scratch(ctx, tw_bytes + win_bytes + (size_t)n_frames * sizeof(int64_t)));
    char *scr = (char *)ctx->scratch;
    SarArgs a{};
    a.cubes = (const float2 *)d_cubes;
    a.tw1 = (const float2 *)scr;
    a.twc = twc;
    a.win = (const int4 *)(scr + tw_bytes);
    a.off = (const long long *)(scr + tw_bytes + win_bytes);
    a.out = (float2 *)d_out;
    a.n_frames = n_frames, a.V = V, a.S = S, a.C = C, a.rx = rx_idx, a.row0 = rows[0], a.KP = KP;
    MMW_HIP(hipMemcpyAsync((void *)a.win, h_win, (size_t)n_frames * sizeof(int4), hipMemcpyHostToDevice, ctx->stream));
    MMW_HIP(hipMemcpyAsync((void *)a.off, h_off, (size_t)n_frames * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    MMW_HIP(hipStreamSynchronize(ctx->stream));     // the tables are host memory of this call
    ProfScope ps(ctx, "sar_slices");
    hipLaunchKernelGGL(k_sar_twiddle, dim3((unsigned)(((long)S * KP + 255) / 256)), dim3(256), 0, ctx->stream, tws, (float2 *)scr, S,
                       rows[0], KP);
    MMW_TRY(check_launch("sar_twiddle"));
    if (KT == 16) return launch_sar_slices<16>(ctx, a);
    if (KT == 8) return launch_sar_slices<8>(ctx, a);
    return launch_sar_slices<4>(ctx, a);
}

}  // extern "C"
