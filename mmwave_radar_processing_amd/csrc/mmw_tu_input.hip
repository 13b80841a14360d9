// Translation unit of the entry points whose kernels are in mmw_staging.h: input staging, the range-Doppler dispatch with its float64
// plane and its rounding-error budget, the range profiles, mmw_plane_l1, |.|, the float64 widening and the diagnostics of both.
#include "mmw_entry.h"
#include "mmw_launch.h"
#include "mmw_staging.h"

#include <algorithm>

using namespace mmw;

bool mmw::fused_rd_ok(int S, int C) { return rd_fused_supported(S, C); }

// the fused 256 x 128 range-Doppler kernel runs (range_doppler_impl's first choice)
bool mmw::fused_rd_runs(int S, int C) { return fused_rd_ok(S, C) && !env_int("MMW_NO_FUSED_RD", 0); }
// the range-Doppler stage touches no scratch: the fused kernel, or a compile-time mixed-radix one (tables only)
bool mmw::rd_needs_no_scratch(int S, int C) {
    return fused_rd_runs(S, C) || (!fused_rd_ok(S, C) && rd_mixed_ct_supported(S, C) && !env_int("MMW_NO_MIXED_RD", 0));
}

namespace {

int abs_c64(mmw_ctx *ctx, const void *d_in, float *d_out, size_t n) {
    if (n == 0) return MMW_OK;
    hipLaunchKernelGGL(k_abs_c64, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                       (const float2 *)d_in, d_out, n);
    return check_launch("abs_c64");
}

// Range FFT (windows on both axes folded into the load) then in-place Doppler FFT + fftshift.
// Frames go through in chunks of ~96 MB of output so that the Doppler pass finds the range
// pass's result still in the 256 MB Infinity Cache instead of re-reading it from HBM.
static int range_doppler_generic_chunk(mmw_ctx *ctx, const void *d_cubes, void *d_out, int F, int V, int S, int C) {
    FftArgs a{};
    a.in = d_cubes;
    a.out = d_out;
    a.outer = F * V;
    a.inner = C;
    a.n_in = S;
    a.in_outer_stride = a.out_outer_stride = (long)S * C;
    a.in_axis_stride = a.out_axis_stride = C;
    a.in_inner_stride = a.out_inner_stride = 1;
    MMW_TRY(get_table<float>(ctx, TAB_HANN, S, &a.win_axis));
    MMW_TRY(get_table<float>(ctx, TAB_HANN, C, &a.win_inner));
    a.scale = 1.0;
    MMW_TRY((launch_fft_axis<float, float>(ctx, a, S, false)));
    FftArgs b{};
    b.in = d_out;
    b.out = d_out;  // each workgroup reads its rows completely before it writes them
    b.outer = F * V * S;
    b.inner = 1;
    b.n_in = C;
    b.in_outer_stride = b.out_outer_stride = C;
    b.in_axis_stride = b.out_axis_stride = 1;
    b.scale = 1.0;
    b.shift = 1;
    return launch_fft_axis<float, float>(ctx, b, C, true);
}

int range_doppler_generic(mmw_ctx *ctx, const void *d_cubes, void *d_out, int F, int V, int S, int C) {
    const size_t cube_bytes = (size_t)V * S * C * sizeof(float2);
    long chunk = (long)(((size_t)96 << 20) / cube_bytes);
    if (chunk < 1) chunk = 1;
    for (long f0 = 0; f0 < F; f0 += chunk) {
        const int nf = (int)((F - f0 < chunk) ? F - f0 : chunk);
        MMW_TRY(range_doppler_generic_chunk(ctx, (const char *)d_cubes + (size_t)f0 * cube_bytes,
                                            (char *)d_out + (size_t)f0 * cube_bytes, nf, V, S, C));
    }
    return MMW_OK;
}

}  // namespace

template <typename T>
int mmw::mean_abs_over_v_impl(mmw_ctx *ctx, const void *d_spec, T *d_out, int n_frames, int V, int S) {
    const long n = (long)n_frames * S;
    hipLaunchKernelGGL((k_mean_abs_over_v<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                       (const cplx<T> *)d_spec, d_out, n_frames, V, S);
    return check_launch("mean_abs_over_v");
}
template int mmw::mean_abs_over_v_impl<float>(mmw_ctx *, const void *, float *, int, int, int);     // also mmw_range_zoom's (mmw_tu_maps.hip)

template <typename T>
int mmw::range_profile_impl(mmw_ctx *ctx, const void *d_cubes, T *d_out, int n_frames, int V, int S, int C,
                            int chirp_idx) {
    MMW_REQUIRE(ctx && d_cubes && d_out, "null argument");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_frames >= 0 && V > 0 && S > 0 && C > 0, "bad shape");
    MMW_REQUIRE(chirp_idx >= -C && chirp_idx < C, "chirp_idx %d out of range", chirp_idx);
    if (chirp_idx < 0) chirp_idx += C;  // numpy negative indexing
    if (n_frames == 0) return MMW_OK;
    MMW_TRY(ensure_scratch(ctx, (size_t)n_frames * V * S * sizeof(cplx<T>)));
    FftArgs a{};
    a.in = (const cplx<float> *)d_cubes + chirp_idx;
    a.out = ctx->scratch;
    a.outer = n_frames * V;
    a.inner = 1;
    a.n_in = S;
    a.in_outer_stride = (long)S * C;
    a.in_axis_stride = C;
    a.in_inner_stride = 1;
    a.out_outer_stride = S;
    a.out_axis_stride = 1;
    a.out_inner_stride = 1;
    MMW_TRY(get_table<T>(ctx, TAB_HANN, S, &a.win_axis));
    a.scale = 1.0;
    MMW_TRY((launch_fft_axis<T, float>(ctx, a, S, false)));
    return mean_abs_over_v_impl<T>(ctx, ctx->scratch, d_out, n_frames, V, S);
}
template int mmw::range_profile_impl<float>(mmw_ctx *, const void *, float *, int, int, int, int, int);
template int mmw::range_profile_impl<double>(mmw_ctx *, const void *, double *, int, int, int, int, int);     // also mmw_tu_cfar.hip's

static int plane_l1_impl(mmw_ctx *ctx, const void *d_cubes, float *d_l1, int n_frames, int V, int S, int C) {
    if (n_frames == 0) return MMW_OK;
    const void *ws, *wc;
    MMW_TRY(get_table<float>(ctx, TAB_HANN, S, &ws));
    MMW_TRY(get_table<float>(ctx, TAB_HANN, C, &wc));
    ProfScope ps(ctx, "plane_l1");
    hipLaunchKernelGGL(k_plane_l1, dim3((unsigned)(n_frames * V)), dim3(256), 0, ctx->stream, (const float2 *)d_cubes, d_l1, S,
                       C, (const float *)ws, (const float *)wc);
    return check_launch("plane_l1");
}

// ------------------------------------------------------------------ range-Doppler dispatch
// rv.ntx > 1: d_cubes is the raw [F][num_rx][S][num_tx * C] cube and the virtual-array de-interleave is folded into
// the load of the single-pass kernels (V == rv.ntx * rv.nrx).
// d_l1 != nullptr: also the per-plane L1 norms of the windowed input (mmw_plane_l1), from inside the RD kernel where it
// can produce them, else by a pass of k_plane_l1.
int mmw::range_doppler_impl(mmw_ctx *ctx, const void *d_cubes, void *d_out, void *d_mag_f32, int n_frames, int V, int S, int C,
                            RawView rv, float *d_l1) {
    MMW_REQUIRE(ctx && d_cubes && d_out, "null argument");
    MMW_REQUIRE(n_frames >= 0 && V > 0 && S > 0 && C > 0, "bad shape");
    if (n_frames == 0) return MMW_OK;
    {
        ProfScope ps(ctx, "rd");
        bool l1_done = false;
        // int16 raw cubes: folded into the loads of the 256 x 128 kernel and of the compile-time mixed-radix kernels (the
        // plane shapes of every shipped cfg); anything else converts + de-interleaves first (one extra pass)
        const bool i16_folded = rv.i16 && rv.ntx > 1 &&
                                (fused_rd_runs(S, C) ||
                                 (rd_mixed_ct_supported(S, C) && !env_int("MMW_NO_MIXED_RD", 0)));
        if (rv.i16 && !i16_folded) {
            MMW_REQUIRE(rv.ntx >= 1 && rv.nrx >= 1, "int16 cubes are raw cubes");
            const long total = (long)n_frames * V * S * C;
            hipLaunchKernelGGL(k_reformat_i16, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream,
                               (const short2 *)d_cubes, (float2 *)d_out, total, rv.nrx, rv.ntx, S, C);
            MMW_TRY(check_launch("reformat_i16"));
            // every kernel below may run in place on a virtual-array cube: a workgroup has read all of its plane (and a
            // persistent one prefetches only planes it will write itself) before it stores
            d_cubes = d_out;
            rv = RawView{1, 0, rv.vskip, 0};
        }
        if (fused_rd_runs(S, C))
            MMW_TRY(launch_rd_fused(ctx, d_cubes, d_out, n_frames * V, S, C, rv, rv.ntx > 1 ? nullptr : d_l1, &l1_done));
        else if (rd_lds_supported(S, C) && !env_int("MMW_NO_FUSED_RD", 0) && !rd_mixed_ct_supported(S, C))      // the compile-time kernel is faster where both exist (64 x 64: 6.0 vs 4.4 TB/s)
            MMW_TRY(launch_rd_lds(ctx, d_cubes, d_out, n_frames * V, S, C, rv));
        else if (rd_mixed_ct_supported(S, C) && !env_int("MMW_NO_MIXED_RD", 0)) {
            // compile-time kernel; on virtual-array cubes it also leaves the planes' L1 norms when asked
            float *l1 = rv.ntx > 1 ? nullptr : d_l1;
            MMW_TRY(launch_rd_mixed_ct(ctx, d_cubes, (long)S * C, d_out, n_frames * V, S, C, rv, nullptr, 0, nullptr, false, l1));
            l1_done = l1 != nullptr;
        } else if (rd_mixed_supported(S, C) && !env_int("MMW_NO_MIXED_RD", 0))
            MMW_TRY((launch_rd_mixed<float, false>(ctx, d_cubes, (long)S * C, d_out, n_frames * V, S, C, rv)));
        else if (rv.ntx <= 1 && rd_split_ct_supported(S, C) && !env_int("MMW_NO_SPLIT_RD", 0))
            MMW_TRY(launch_rd_split_ct(ctx, d_cubes, d_out, n_frames * V, S, C, rv));
        else if (rv.ntx > 1) {
            // no single-pass kernel for this plane: de-interleave into the output buffer, then transform it in place
            const long total = (long)n_frames * V * S * C;
            hipLaunchKernelGGL(k_reformat, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream,
                               (const float2 *)d_cubes, (float2 *)d_out, total, rv.nrx, rv.ntx, S, C);
            MMW_TRY(check_launch("reformat"));
            // (the split kernel reads its whole plane before its first store, so it may run in place as well)
            if (rd_split_ct_supported(S, C) && !env_int("MMW_NO_SPLIT_RD", 0))
                MMW_TRY(launch_rd_split_ct(ctx, d_out, d_out, n_frames * V, S, C, RawView{1, 0, rv.vskip}));
            else
                MMW_TRY(range_doppler_generic(ctx, d_out, d_out, n_frames, V, S, C));
        } else
            MMW_TRY(range_doppler_generic(ctx, d_cubes, d_out, n_frames, V, S, C));
        if (d_l1 && !l1_done) {
            MMW_REQUIRE(rv.ntx <= 1, "plane L1 norms are defined on virtual-array cubes");
            MMW_TRY(plane_l1_impl(ctx, d_cubes, d_l1, n_frames, V, S, C));
        }
    }
    if (d_mag_f32) MMW_TRY(abs_c64(ctx, d_out, (float *)d_mag_f32, (size_t)n_frames * V * S * C));
    return MMW_OK;
}

// Rounding-error budget of the float32 range-Doppler cell values, in units of eps = 2^-24 of the plane's L1 norm
// (|rd32 - rd64| <= ulps * eps * sum |w x|), for whichever kernel range_doppler_impl runs on an S x C plane.
//   windows: two products with table values, <= 8.
//   structured transforms (k_rd_fused_256x128, k_rd_lds, k_rd_mixed_ct, k_rd_split2_ct: RegFFT / RegDFT levels): per
//     prime factor p of the axis length one twiddle / inter-level product (complex FMA product + table value, <= 4) plus
//     p == 2: the butterfly's add (inside the 4);  odd p: the real-symmetric form of RegDFT -- pair sums (1), a
//     (p - 1) / 2-term FMA chain with literal coefficients ((p + 1) / 2), the +- i combine (1): <= (p + 7) / 2 + 1.
//     The 127-point level of 63 x 127 / 127 x 32 / 254 x 50 is that form on MFMA tiles (64-term exact FMA chains).
//   run-time mixed-radix kernel: its levels may be direct R-term chains: R per level on top.
//   generic path: radix-2 levels (4 each) for powers of two, an N-term direct sum (N + 4) otherwise.
// tests/test_rd_bound_cases_host.py restates these counts; tests/test_gpu_rd_error_bound.py asserts the inequality per family.
int mmw::rd_error_ulps(int S, int C) {
    auto factors = [](int n) {
        int u = 0;
        for (int p = 2; n > 1; ++p)
            while (n % p == 0) {
                u += 4 + (p == 2 ? 0 : (p == 127 ? 88 : (p + 7) / 2 + 1));       // (127: the bfloat16 x 3 MFMA form, mmw_fft_mixed_ct.h)
                n /= p;
            }
        return u;
    };
    const int structured = 8 + factors(S) + factors(C);
    const bool no_fused = env_int("MMW_NO_FUSED_RD", 0), no_mixed = env_int("MMW_NO_MIXED_RD", 0);
    if (!no_fused && (fused_rd_ok(S, C) || rd_lds_supported(S, C))) return structured;
    if (!no_mixed && rd_mixed_ct_supported(S, C)) return structured;
    RdMixedPlan mp;
    if (!no_mixed && rd_mixed_plan(S, C, sizeof(cplx<float>), &mp))
        return structured + mp.s1 + mp.s2 + mp.c1 + mp.c2 + 2 * (mp.rad_s[0] + mp.rad_s[1] + mp.rad_c[0] + mp.rad_c[1]);
    if (rd_split_ct_supported(S, C) && !env_int("MMW_NO_SPLIT_RD", 0)) return structured;
    int ulps = 8;
    for (int axis = 0; axis < 2; ++axis) {
        const int n = axis ? C : S;
        if (is_pow2(n)) ulps += 4 * ilog2(n);
        else ulps += n + 4;
    }
    return ulps;
}

// Does the float64 CFAR plane of an S x C shape go through the LDS-resident single-pass kernel?  Every plane that fits in
// float64 except small power-of-two ones, where the two-kernel register-FFT path is as fast (64 x 64, 512 x 8: equal;
// 128 x 64, 256 x 32: single pass +18 %).  One predicate for range_doppler_mag64_impl and mmw_diag_rd_plan.
static bool rd64_takes_mixed(int S, int C, RdMixedPlan *out) {
    RdMixedPlan mp;
    if (is_pow2(S) && is_pow2(C) && (long)S * C < 8192) return false;
    if (env_int("MMW_NO_MIXED_RD", 0) || !rd_mixed_plan(S, C, sizeof(cplx<double>), &mp)) return false;
    if (out) *out = mp;
    return true;
}

// Bytes of ctx->scratch range_doppler_mag64_impl below touches for n_frames planes of S x C (its three routes, restated): a caller
// that keeps data of its own behind them sizes the scratch once, before the first launch (mmw_tu_integrated.hip).
size_t mmw::rd_mag64_scratch_bytes(mmw_ctx *ctx, int n_frames, int S, int C) {
    const size_t plane_bytes = (size_t)S * C * sizeof(cplx<double>);
    if (rd_mag64_fused_ok(S, C) && n_frames >= 8 && opt_int(ctx, "MMW_RD64_FUSED", 1))
        return (size_t)std::min(n_frames, ctx->num_cu) * plane_bytes;
    if (rd64_takes_mixed(S, C, nullptr)) return 0;
    const size_t chunk = std::max<size_t>(1, ((size_t)128 << 20) / plane_bytes);
    return std::min<size_t>(chunk, (size_t)std::max(n_frames, 1)) * plane_bytes;
}

int mmw::range_doppler_mag64_impl(mmw_ctx *ctx, const void *d_cubes, double *d_mag, int n_frames, int V, int S, int C,
                                  int rx_idx) {
    MMW_REQUIRE(ctx && d_cubes && d_mag, "null argument");
    MMW_REQUIRE(n_frames >= 0 && V > 0 && S > 0 && C > 0 && rx_idx >= 0 && rx_idx < V, "bad shape / rx_idx");
    if (n_frames == 0) return MMW_OK;
    ProfScope ps(ctx, "rd64");
    // batches only (a single frame is spread over the chip by the two generic launches)
    if (rd_mag64_fused_ok(S, C) && n_frames >= 8 && opt_int(ctx, "MMW_RD64_FUSED", 1))
        return launch_rd_mag64_fused(ctx, d_cubes, d_mag, n_frames, V, rx_idx);
    if (rd64_takes_mixed(S, C, nullptr))
        return launch_rd_mixed<double, true>(ctx, (const cplx<float> *)d_cubes + (long)rx_idx * S * C,
                                             (long)V * S * C, d_mag, n_frames, S, C);
    // two passes with a complex128 intermediate: chunks of frames small enough for the intermediate to stay in the
    // Infinity Cache between them (128 MB; it also bounds the scratch: all 1250 frames of the bench at once were 640 MB)
    const size_t plane_bytes = (size_t)S * C * sizeof(cplx<double>);
    long chunk = (long)(((size_t)128 << 20) / plane_bytes);
    if (chunk < 1) chunk = 1;
    if (chunk > n_frames) chunk = n_frames;
    MMW_TRY(ensure_scratch(ctx, (size_t)chunk * plane_bytes));
    FftArgs a{};
    a.out = ctx->scratch;
    a.inner = C;
    a.n_in = S;
    a.in_outer_stride = (long)V * S * C;
    a.out_outer_stride = (long)S * C;
    a.in_axis_stride = a.out_axis_stride = C;
    a.in_inner_stride = a.out_inner_stride = 1;
    MMW_TRY(get_table<double>(ctx, TAB_HANN, S, &a.win_axis));
    MMW_TRY(get_table<double>(ctx, TAB_HANN, C, &a.win_inner));
    a.scale = 1.0;
    FftArgs b{};
    b.in = ctx->scratch;
    b.inner = 1;
    b.n_in = C;
    b.in_outer_stride = b.out_outer_stride = C;
    b.in_axis_stride = b.out_axis_stride = 1;
    b.scale = 1.0;
    b.shift = 1;
    b.magnitude = 1;
    for (long f0 = 0; f0 < n_frames; f0 += chunk) {
        const int nf = (int)std::min<long>(chunk, n_frames - f0);
        a.in = (const cplx<float> *)d_cubes + (f0 * V + rx_idx) * (long)S * C;
        a.outer = nf;
        MMW_TRY((launch_fft_axis<double, float>(ctx, a, S, false)));
        b.out = d_mag + f0 * (long)S * C;
        b.outer = nf * S;
        MMW_TRY((launch_fft_axis<double, double>(ctx, b, C, true)));
    }
    return MMW_OK;
}

extern "C" {

// ------------------------------------------------------------------ input staging
int mmw_synth_cubes(mmw_ctx *ctx, void *d_cubes, int n_frames, int V, int S, int C, uint64_t seed0,
                    int num_targets, float noise_sigma) {
    MMW_REQUIRE(ctx && d_cubes, "null argument");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_frames >= 0 && V > 0 && S > 0 && C > 0, "bad shape");
    MMW_REQUIRE(num_targets >= 0 && num_targets <= SYNTH_MAX_TARGETS, "num_targets must be 0..%d", SYNTH_MAX_TARGETS);
    const long total = (long)n_frames * V * S * C;
    if (!total) return MMW_OK;
    hipLaunchKernelGGL(k_synth, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream,
                       (float2 *)d_cubes, total, V, S, C, (unsigned long long)seed0, num_targets, noise_sigma);
    return check_launch("synth");
}

int mmw_virtual_array_reformat(mmw_ctx *ctx, const void *d_raw, void *d_virt, int n_frames, int num_rx,
                               int num_tx, int S, int loops) {
    MMW_REQUIRE(ctx && d_raw && d_virt, "null argument");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_frames >= 0 && num_rx > 0 && num_tx > 0 && S > 0 && loops > 0, "bad shape");
    const long total = (long)n_frames * num_rx * num_tx * S * loops;
    if (!total) return MMW_OK;
    hipLaunchKernelGGL(k_reformat, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream,
                       (const float2 *)d_raw, (float2 *)d_virt, total, num_rx, num_tx, S, loops);
    return check_launch("reformat");
}

int mmw_virtual_array_reformat_i16(mmw_ctx *ctx, const void *d_raw_i16, void *d_virt, int n_frames, int num_rx,
                                   int num_tx, int S, int loops) {
    MMW_REQUIRE(ctx && d_raw_i16 && d_virt, "null argument");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_frames >= 0 && num_rx > 0 && num_tx > 0 && S > 0 && loops > 0, "bad shape");
    const long total = (long)n_frames * num_rx * num_tx * S * loops;
    if (!total) return MMW_OK;
    hipLaunchKernelGGL(k_reformat_i16, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream,
                       (const short2 *)d_raw_i16, (float2 *)d_virt, total, num_rx, num_tx, S, loops);
    return check_launch("reformat_i16");
}

int mmw_range_doppler(mmw_ctx *ctx, const void *d_cubes, void *d_out, void *d_mag_f32, int n_frames, int V,
                      int S, int C) {
    MMW_REQUIRE(ctx, "ctx is null");
    MMW_JOIN(ctx);
    return range_doppler_impl(ctx, d_cubes, d_out, d_mag_f32, n_frames, V, S, C);
}

int mmw_range_doppler_mag64(mmw_ctx *ctx, const void *d_cubes, double *d_mag, int n_frames, int V, int S,
                            int C, int rx_idx) {
    MMW_REQUIRE(ctx, "ctx is null");
    MMW_JOIN(ctx);
    return range_doppler_mag64_impl(ctx, d_cubes, d_mag, n_frames, V, S, C, rx_idx);
}

int mmw_range_profile(mmw_ctx *ctx, const void *d_cubes, float *d_out, int n_frames, int V, int S, int C,
                      int chirp_idx) {
    return range_profile_impl<float>(ctx, d_cubes, d_out, n_frames, V, S, C, chirp_idx);
}

int mmw_range_profile_f64(mmw_ctx *ctx, const void *d_cubes, double *d_out, int n_frames, int V, int S, int C,
                          int chirp_idx) {
    return range_profile_impl<double>(ctx, d_cubes, d_out, n_frames, V, S, C, chirp_idx);
}

int mmw_plane_l1(mmw_ctx *ctx, const void *d_cubes, float *d_l1, int n_frames, int V, int S, int C) {
    MMW_REQUIRE(ctx && d_cubes && d_l1, "null argument");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_frames >= 0 && V > 0 && S > 0 && C > 0 && (long)n_frames * V < (1L << 31), "bad shape");
    return plane_l1_impl(ctx, d_cubes, d_l1, n_frames, V, S, C);
}

int mmw_abs_c64(mmw_ctx *ctx, const void *d_in, float *d_out, size_t n) {
    MMW_REQUIRE(ctx && (n == 0 || (d_in && d_out)), "null argument");
    MMW_JOIN(ctx);
    return abs_c64(ctx, d_in, d_out, n);
}

int mmw_widen_f32_f64(mmw_ctx *ctx, const float *d_in, double *d_out, size_t n) {
    MMW_REQUIRE(ctx && (n == 0 || (d_in && d_out)), "null argument");
    MMW_JOIN(ctx);
    if (n == 0) return MMW_OK;
    const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, (size_t)ctx->num_cu * 16);
    hipLaunchKernelGGL(k_widen_f32_f64, dim3(grid), dim3(256), 0, ctx->stream, d_in, d_out, n);
    return check_launch("widen_f32_f64");
}

int mmw_diag_rd_plan(int S, int C, int float64, int plan[8]) {
    MMW_REQUIRE(plan && S > 0 && C > 0, "bad argument");
    for (int i = 0; i < 8; ++i) plan[i] = 0;
    RdMixedPlan pl{};
    if (float64)
        plan[0] = rd64_takes_mixed(S, C, &pl) ? 2 : 3;       // (the entry's own test: MMW_NO_MIXED_RD included)
    else if (fused_rd_ok(S, C))
        plan[0] = 0;
    else if (rd_lds_supported(S, C))
        plan[0] = 1;
    else
        plan[0] = rd_mixed_plan(S, C, sizeof(cplx<float>), &pl) ? 2 : (rd_split_ct_supported(S, C) ? 4 : 3);
    if (plan[0] == 2) {
        plan[1] = pl.cls;
        plan[2] = pl.big;
        plan[3] = pl.s1;
        plan[4] = pl.s2;
        plan[5] = pl.c1;
        plan[6] = pl.c2;
        plan[7] = (int)pl.lds_bytes;
    }
    return MMW_OK;
}

int mmw_diag_membw(mmw_ctx *ctx, const void *d_src, void *d_dst, size_t bytes, int mode, int blocks) {
    MMW_REQUIRE(ctx && d_src && d_dst && bytes % 16 == 0 && mode >= 0 && mode <= 7, "bad argument");
    MMW_JOIN(ctx);
    if (blocks <= 0) blocks = ctx->num_cu * 8;
    hipLaunchKernelGGL(k_diag_membw, dim3(blocks), dim3(256), 0, ctx->stream, (const diag_f4 *)d_src,
                       (diag_f4 *)d_dst, bytes / 16, mode);
    return check_launch("diag_membw");
}

}  // extern "C"
