// Translation unit of the range snapshots for the Capon stage (mmw_range_snapshots.h).
#include "mmw_ctx.h"
#include "mmw_range_snapshots.h"

using namespace mmw;

template <int N, int R1, int R2> static int launch_rs_fft(mmw_ctx *ctx, const RsArgs &p, long blocks) {
    constexpr size_t lds = rs_fft_lds_bytes(R1, R2);
    if (lds > 64 * 1024)
        MMW_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_rs_fft<N, R1, R2>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds));         // per device, so on every call
    hipLaunchKernelGGL((k_rs_fft<N, R1, R2>), dim3((unsigned)blocks), dim3(RS_STRIP * R2), lds, ctx->stream, p);
    return check_launch("range_snapshots_fft");
}

static int launch_rs(mmw_ctx *ctx, const RsArgs &p, long blocks) {
    switch (p.S) {
        case 16: return launch_rs_fft<16, 4, 4>(ctx, p, blocks);
        case 32: return launch_rs_fft<32, 8, 4>(ctx, p, blocks);
        case 64: return launch_rs_fft<64, 8, 8>(ctx, p, blocks);
        case 128: return launch_rs_fft<128, 16, 8>(ctx, p, blocks);
        case 256: return launch_rs_fft<256, 16, 16>(ctx, p, blocks);
        case 512: return launch_rs_fft<512, 32, 16>(ctx, p, blocks);
        case 1024: return launch_rs_fft<1024, 32, 32>(ctx, p, blocks);
        default: break;
    }
    const size_t lds = rs_direct_lds_bytes(p.S);
    if (lds > 64 * 1024)
        MMW_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_rs_direct), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_rs_direct, dim3((unsigned)blocks), dim3(256), lds, ctx->stream, p);
    return check_launch("range_snapshots_direct");
}

// Every argument is judged here, before the context is touched: the function is not given the context, so a refused call cannot
// enqueue anything and needs no device (tests/cpp/range_snapshots_sanitize.cpp relies on it).
static int rs_validate(bool have_ctx, const void *d_cubes, const void *d_out, int n_frames, int V, int S, int C, const int *h_rx,
                       int n_rx, int r_lo, int r_hi) {
    MMW_REQUIRE(have_ctx && d_cubes && d_out, "null argument (ctx %d, d_cubes %d, d_out %d)", (int)have_ctx, d_cubes != nullptr,
                d_out != nullptr);
    MMW_REQUIRE(n_frames >= 0, "n_frames is %d", n_frames);
    MMW_REQUIRE(V > 0 && S > 0 && C > 0, "bad shape: V %d, S %d, C %d must all be positive", V, S, C);
    MMW_REQUIRE(n_rx >= 0, "n_rx is %d", n_rx);
    MMW_REQUIRE(n_rx == 0 || h_rx, "h_rx is null with n_rx %d", n_rx);
    for (int i = 0; i < n_rx; ++i)
        MMW_REQUIRE(h_rx[i] >= 0 && h_rx[i] < V, "h_rx[%d] = %d is not an antenna of [0, %d)", i, h_rx[i], V);
    MMW_REQUIRE(r_lo >= 0 && r_lo < r_hi && r_hi <= S, "range window [%d, %d) is not 0 <= r_lo < r_hi <= %d", r_lo, r_hi, S);
    if (S > RS_MAX_S)
        return set_error(MMW_ERR_UNSUPPORTED, "range snapshots: %d samples per chirp (at most %d: a strip of %d chirps lives in the LDS)",
                         S, RS_MAX_S, RS_STRIP);
    return MMW_OK;
}

extern "C" {

int mmw_range_snapshots(mmw_ctx *ctx, const void *d_cubes, void *d_out, int n_frames, int V, int S, int C, const int *h_rx, int n_rx,
                        int r_lo, int r_hi, int perform_windowing) {
    MMW_TRY(rs_validate(ctx != nullptr, d_cubes, d_out, n_frames, V, S, C, h_rx, n_rx, r_lo, r_hi));
    if (n_frames == 0) return MMW_OK;
    RsArgs p{};
    p.cubes = (const float2 *)d_cubes;
    p.out = (float2 *)d_out;
    p.V = V, p.S = S, p.C = C;
    p.strips = C / RS_STRIP + (C % RS_STRIP != 0);
    p.n_out_rx = n_rx ? n_rx : V;
    p.r_lo = r_lo, p.r_hi = r_hi;
    // the kernel arguments hold MAX_ANT antennas: a longer list goes in several launches (all V antennas in order need no list)
    const int per_launch = n_rx ? std::min(n_rx, MAX_ANT) : V;
    if ((long)per_launch * p.strips > 2147483647L / n_frames)
        return set_error(MMW_ERR_UNSUPPORTED, "range snapshots: %d frames x %d antennas x %d strips of chirps exceed one launch grid",
                         n_frames, per_launch, p.strips);
    MMW_JOIN(ctx);
    MMW_TRY(get_table<float>(ctx, TAB_TWIDDLE, S, (const void **)&p.tw));
    if (perform_windowing) MMW_TRY(get_table<float>(ctx, TAB_HANN, S, (const void **)&p.win));
    ProfScope ps(ctx, "range_snapshots");
    for (int i0 = 0; i0 < p.n_out_rx; i0 += per_launch) {
        p.i0 = i0;
        p.n_launch = std::min(per_launch, p.n_out_rx - i0);
        p.ants.n = n_rx ? p.n_launch : 0;
        for (int i = 0; i < p.ants.n; ++i) p.ants.idx[i] = h_rx[i0 + i];
        MMW_TRY(launch_rs(ctx, p, (long)n_frames * p.n_launch * p.strips));
    }
    return MMW_OK;
}

}  // extern "C"
