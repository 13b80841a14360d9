// Translation unit of the batched micro-Doppler rows (mmw_micro_doppler.h).
#include "mmw_ctx.h"
#include "mmw_micro_doppler.h"

using namespace mmw;

template <int KT>
static int launch_micro_doppler(mmw_ctx *ctx, const float2 *cubes, const float2 *tw1, const float2 *twc, float *out, int n_frames,
                                int V, int S, int C, int rx, int K, int KP) {
    const size_t lds = md_lds_bytes(KT, C);
    if (lds > 64 * 1024)
        MMW_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_micro_doppler<KT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds));         // per device, so on every call
    hipLaunchKernelGGL(k_micro_doppler<KT>, dim3((unsigned)n_frames), dim3(256), lds, ctx->stream, cubes, tw1, twc, out, V, S, C, rx,
                       K, KP);
    return check_launch("micro_doppler");
}

// Every argument is judged here, before the context is touched: the function is not given the context, so a refused call cannot
// enqueue anything and needs no device (tests/cpp/micro_doppler_sanitize.cpp relies on it).
static int md_validate(bool have_ctx, const void *d_cubes, const float *d_out, int n_frames, int V, int S, int C, int rx_idx, int row_lo,
                       int row_hi) {
    MMW_REQUIRE(have_ctx && d_cubes && d_out, "null argument (ctx %d, d_cubes %d, d_out %d)", (int)have_ctx, d_cubes != nullptr,
                d_out != nullptr);
    MMW_REQUIRE(n_frames >= 0, "n_frames is %d", n_frames);
    MMW_REQUIRE(V > 0 && S > 0 && C > 0, "bad shape: V %d, S %d, C %d must all be positive", V, S, C);
    MMW_REQUIRE(rx_idx >= 0 && rx_idx < V, "rx_idx %d is not an antenna of [0, %d)", rx_idx, V);
    MMW_REQUIRE(row_lo <= row_hi, "empty range window: row_lo %d > row_hi %d", row_lo, row_hi);
    MMW_REQUIRE(row_lo >= 0 && row_hi < S, "range window [%d, %d] leaves the %d range rows", row_lo, row_hi, S);
    return MMW_OK;
}

extern "C" {

int mmw_micro_doppler(mmw_ctx *ctx, const void *d_cubes, float *d_out, int n_frames, int V, int S, int C, int rx_idx, int row_lo,
                      int row_hi) {
    MMW_TRY(md_validate(ctx != nullptr, d_cubes, d_out, n_frames, V, S, C, rx_idx, row_lo, row_hi));
    if (n_frames == 0) return MMW_OK;
    const int K = row_hi - row_lo + 1;
    const int KT = md_pick_kt(K, C, opt_int(ctx, "MMW_MD_KT", 0));
    if (!KT)
        return set_error(MMW_ERR_UNSUPPORTED, "micro-Doppler kernel: %d chirps need %zu bytes of LDS with 4 rows in flight (at most "
                         "160 KiB)", C, md_lds_bytes(4, C));
    MMW_JOIN(ctx);
    const int KP = (K + KT - 1) / KT * KT;
    const float2 *tws = nullptr, *twc = nullptr;
    MMW_TRY(get_table<float>(ctx, TAB_TWIDDLE, S, (const void **)&tws));
    MMW_TRY(get_table<float>(ctx, TAB_TWIDDLE, C, (const void **)&twc));
    MMW_TRY(ensure_scratch(ctx, (size_t)S * KP * sizeof(float2)));
    float2 *tw1 = (float2 *)ctx->scratch;
    ProfScope ps(ctx, "micro_doppler");
    hipLaunchKernelGGL(k_md_twiddle, dim3((unsigned)(((long)S * KP + 255) / 256)), dim3(256), 0, ctx->stream, tws, tw1, S, row_lo, KP);
    MMW_TRY(check_launch("md_twiddle"));
    const float2 *cubes = (const float2 *)d_cubes;
    if (KT == 16) return launch_micro_doppler<16>(ctx, cubes, tw1, twc, d_out, n_frames, V, S, C, rx_idx, K, KP);
    if (KT == 8) return launch_micro_doppler<8>(ctx, cubes, tw1, twc, d_out, n_frames, V, S, C, rx_idx, K, KP);
    return launch_micro_doppler<4>(ctx, cubes, tw1, twc, d_out, n_frames, V, S, C, rx_idx, K, KP);
}

}  // extern "C"
