// Translation unit of the range, DBS and Doppler-azimuth maps with their zoom / chirp-z variants (kernels: mmw_maps.h, mmw_dbs.h,
// mmw_czt.h; the range-Doppler and angle stages in front of them are other units' launchers).
#include "mmw_entry.h"
#include "mmw_launch.h"
#include "mmw_maps.h"
#include "mmw_dbs.h"
#include "mmw_czt.h"

#include <algorithm>
#include <climits>

using namespace mmw;

// Frames per launch pair (range-Doppler, k_dbs_sharpen) when the range-Doppler cubes go to the library's scratch: as many as keep
// the intermediate within MMW_DBS_CHUNK_MB.  The default of 1024 bounds the scratch at 1 GB, as mmw_doppler_azimuth does; measured
// on 1250 frames of 12 x 256 x 128 (tools/dbs_batch.py) larger chunks are faster all the way: 32 MB 3.82 ms, 128 MB
// 2.46 ms, 1024 MB 2.07 ms, one chunk 2.04 ms -- keeping the chunk inside the Infinity Cache buys nothing against fewer launches.
static long dbs_chunk_frames(const mmw_ctx *ctx, size_t cube_bytes, int n_frames) {
    const size_t budget = (size_t)std::max(1, opt_int(ctx, "MMW_DBS_CHUNK_MB", 1024)) << 20;
    return std::max<long>(1, std::min<long>({(long)(budget / cube_bytes), 65535L, (long)n_frames}));
}

// |angle FFT| averaged over the range rows [s_lo, s_hi): d_rd [nf][V][S][C] c64 -> d_out [nf][C][A] float32.
// Fused single pass (k_angle64_rmean) when the angle fast path applies, else |angle FFT| cube + k_mean_over_range.
// d_work: scratch of angle_mean_work_bytes(...) bytes.
static bool angle_mean_fused(int V, int A) { return A == 64 && (V == 4 || V == 8 || V == 12 || V == 16) && !env_int("MMW_NO_FUSED_ANGLE", 0); }
static size_t angle_mean_work_bytes(int nf, int V, int S, int C, int A, int rows) {
    if (angle_mean_fused(V, A)) return (size_t)nf * rmean_partitions(nf, S, C, rows) * RMEAN_RL * 64 * C * sizeof(float);
    return (size_t)nf * A * S * C * sizeof(float);
}

static int angle_mean_impl(mmw_ctx *ctx, const void *d_rd, void *d_work, size_t work_bytes, float *d_out, int nf, int V,
                           int S, int C, int A, int s_lo, int s_hi, int flags) {
    const bool window = !(flags & MMW_ANGLE_NO_WINDOW), shift = !(flags & MMW_ANGLE_NO_SHIFT);
    if (angle_mean_fused(V, A)) {
        ProfScope ps(ctx, "angle_rmean");
        float h[16];
        for (int i = 0; i < V; ++i) h[i] = window ? (float)np_window(TAB_HANN, i, V) : 1.f;
        switch (V) {
            case 4: return launch_angle64_rmean<4>(ctx, d_rd, (float *)d_work, work_bytes, d_out, nf, S, C, s_lo, s_hi, h, shift);
            case 8: return launch_angle64_rmean<8>(ctx, d_rd, (float *)d_work, work_bytes, d_out, nf, S, C, s_lo, s_hi, h, shift);
            case 12: return launch_angle64_rmean<12>(ctx, d_rd, (float *)d_work, work_bytes, d_out, nf, S, C, s_lo, s_hi, h, shift);
            default: return launch_angle64_rmean<16>(ctx, d_rd, (float *)d_work, work_bytes, d_out, nf, S, C, s_lo, s_hi, h, shift);
        }
    }
    MMW_TRY(angle_fft_impl(ctx, d_rd, d_work, nf, V, S, C, A, (flags & (MMW_ANGLE_NO_WINDOW | MMW_ANGLE_NO_SHIFT)) | MMW_ANGLE_MAGNITUDE));
    const long total = (long)nf * A * C;
    hipLaunchKernelGGL(k_mean_over_range, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream,
                       (const float *)d_work, d_out, nf, A, S, C, s_lo, s_hi);
    return check_launch("mean_over_range");
}

extern "C" {

int mmw_range_zoom(mmw_ctx *ctx, const void *d_cubes, float *d_out, int n_frames, int V, int S, int C, int chirp_idx,
                   int m, double f0_cycles_per_sample, double df_cycles_per_sample) {
    MMW_REQUIRE(ctx && d_cubes && d_out, "null argument");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_frames >= 0 && V > 0 && S > 0 && C > 0 && m > 0, "bad shape");
    MMW_REQUIRE(chirp_idx >= -C && chirp_idx < C, "chirp_idx %d out of range", chirp_idx);
    MMW_REQUIRE((size_t)S * sizeof(float2) <= 64 * 1024, "too many samples for the zoom DFT row buffer");
    if (chirp_idx < 0) chirp_idx += C;
    if (n_frames == 0) return MMW_OK;
    const void *hann;
    MMW_TRY(get_table<float>(ctx, TAB_HANN, S, &hann));
    MMW_TRY(ensure_scratch(ctx, (size_t)n_frames * V * m * sizeof(float2)));
    // rows = (frame, antenna): x[row][i] = cube[frame][v][i][chirp]
    if (czt_length(S) > 0 && !env_int("MMW_ZOOM_DIRECT", 0)) {
        std::vector<double> freq(m);
        for (int k = 0; k < m; ++k) freq[k] = f0_cycles_per_sample + (double)k * df_cycles_per_sample;
        const CztPlan *plan = nullptr;
        MMW_TRY(czt_plan(ctx, freq.data(), m, S, &plan));
        CztArgs z{};
        z.x = (const float2 *)d_cubes + chirp_idx;
        z.outer_stride = (long)S * C;
        z.inner_stride = 0;
        z.elem_stride = C;
        z.s_lo = 0;
        z.s_keep = 1;
        z.win = (const float *)hann;
        z.M = m;
        z.rows = (long)n_frames * V;
        z.out = (float2 *)ctx->scratch;
        MMW_TRY(launch_czt_rows(ctx, *plan, z));
    } else {
        hipLaunchKernelGGL(k_zoom_dft, dim3(n_frames * V), dim3(256), (size_t)S * sizeof(float2), ctx->stream,
                           (const float2 *)d_cubes + chirp_idx, (long)S * C, (long)C, (const float *)hann,
                           (float2 *)ctx->scratch, S, m, f0_cycles_per_sample, df_cycles_per_sample);
        MMW_TRY(check_launch("zoom_dft"));
    }
    return mean_abs_over_v_impl<float>(ctx, ctx->scratch, d_out, n_frames, V, m);
}

int mmw_range_angle(mmw_ctx *ctx, const void *d_cubes, float *d_out, int n_frames, int V, int S, int C, int A,
                    int chirp_idx, const int *h_rx, int n_rx, int perform_windowing) {
    MMW_REQUIRE(ctx && d_cubes && d_out, "null argument");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_frames >= 0 && V > 0 && S > 0 && C > 0 && A > 0, "bad shape");
    MMW_REQUIRE(chirp_idx >= -C && chirp_idx < C, "chirp_idx %d out of range", chirp_idx);
    MMW_REQUIRE(n_rx >= 0 && (n_rx == 0 || h_rx), "bad rx list");
    if (chirp_idx < 0) chirp_idx += C;
    std::vector<int> rx;
    if (n_rx == 0)
        for (int v = 0; v < V; ++v) rx.push_back(v);
    else
        for (int i = 0; i < n_rx; ++i) {
            int r = h_rx[i];
            if (r < 0) r += V;
            MMW_REQUIRE(r >= 0 && r < V, "rx index %d out of range", h_rx[i]);
            rx.push_back(r);
        }
    const int n_sel = (int)rx.size();
    MMW_REQUIRE(n_sel <= A, "more antennas (%d) than angle bins (%d)", n_sel, A);
    if (n_frames == 0) return MMW_OK;
    MMW_TRY(ensure_scratch(ctx, (size_t)n_frames * n_sel * S * sizeof(cplx<float>)));
    for (int i = 0; i < n_sel; ++i) {
        FftArgs a{};
        a.in = (const cplx<float> *)d_cubes + (long)rx[i] * S * C + chirp_idx;
        a.out = (cplx<float> *)ctx->scratch + (long)i * S;
        a.outer = n_frames;
        a.inner = 1;
        a.n_in = S;
        a.in_outer_stride = (long)V * S * C;
        a.in_axis_stride = C;
        a.in_inner_stride = 1;
        a.out_outer_stride = (long)n_sel * S;
        a.out_axis_stride = 1;
        a.out_inner_stride = 1;
        a.scale = 1.0;
        if (perform_windowing) {
            MMW_TRY(get_table<float>(ctx, TAB_HANN, S, &a.win_axis));
            a.scale = np_window(TAB_HANN, rx[i], V);   // hann over ALL V antennas, then the subset
        }
        MMW_TRY((launch_fft_axis<float, float>(ctx, a, S, false)));
    }
    FftArgs b{};
    b.in = ctx->scratch;
    b.out = d_out;
    b.outer = n_frames;
    b.inner = S;
    b.n_in = n_sel;
    b.in_outer_stride = (long)n_sel * S;
    b.in_axis_stride = S;
    b.in_inner_stride = 1;
    b.out_outer_stride = (long)S * A;
    b.out_axis_stride = 1;
    b.out_inner_stride = A;
    b.scale = 1.0;
    b.shift = 1;
    b.magnitude = 1;
    return launch_fft_axis<float, float>(ctx, b, A, false);
}

int mmw_dbs_gather(mmw_ctx *ctx, const float *d_mag, const int *h_ang_idx, const int *h_vel_idx, float *d_out,
                   int n_frames, int A, int S, int C, int n_out) {
    MMW_REQUIRE(ctx && d_mag && h_ang_idx && h_vel_idx && d_out, "null argument");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_frames >= 0 && A > 0 && S > 0 && C > 0 && n_out > 0, "bad shape");
    for (int i = 0; i < n_out; ++i)
        MMW_REQUIRE(h_ang_idx[i] >= 0 && h_ang_idx[i] < A && h_vel_idx[i] >= 0 && h_vel_idx[i] < C,
                    "gather index %d out of range", i);
    if (n_frames == 0) return MMW_OK;
    MMW_TRY(ensure_scratch(ctx, (size_t)2 * n_out * sizeof(int)));
    int *d_idx = (int *)ctx->scratch;
    MMW_HIP(hipMemcpyAsync(d_idx, h_ang_idx, (size_t)n_out * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    MMW_HIP(hipMemcpyAsync(d_idx + n_out, h_vel_idx, (size_t)n_out * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    MMW_HIP(hipStreamSynchronize(ctx->stream));     // the index arrays are caller-owned host memory
    const long total = (long)n_frames * S * n_out;
    hipLaunchKernelGGL(k_dbs_gather, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, d_mag, d_idx,
                       d_idx + n_out, d_out, n_frames, A, S, C, n_out);
    return check_launch("dbs_gather");
}

int mmw_dbs_sharpen(mmw_ctx *ctx, const void *d_cubes, void *d_rd, const int32_t *h_ang_idx, const int32_t *h_vel_idx,
                    float *d_out, int n_frames, int V, int S, int C, int A, const int *h_rx, int n_rx, int n_out) {
    MMW_REQUIRE(ctx, "ctx is null");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_frames >= 0 && V > 0 && S > 0 && C > 0 && A > 0 && n_out >= 0, "bad shape");
    MMW_REQUIRE(n_rx >= 0 && (n_rx == 0 || h_rx), "bad rx list");
    const int n = n_rx ? n_rx : V;
    MMW_REQUIRE(n <= MAX_ANT, "antenna list of %d entries: at most %d", n, MAX_ANT);
    MMW_REQUIRE(A >= n, "more antennas (%d) than angle bins (%d)", n, A);
    for (int j = 0; j < n_rx; ++j)
        MMW_REQUIRE(h_rx[j] >= 0 && h_rx[j] < V, "rx entry %d is %d: not an antenna of [0, %d)", j, h_rx[j], V);
    if (n_frames == 0 || n_out == 0) return MMW_OK;
    MMW_REQUIRE(d_cubes && h_ang_idx && h_vel_idx && d_out, "null argument");
    MMW_REQUIRE((long)n_frames * S * n_out <= (long)INT_MAX, "%d frames of %d x %d pixels do not fit the kernel's 32-bit pixel index",
                n_frames, S, n_out);
    // (b_i, k_i) per frame and output: the FFT bin behind the fftshifted angle index, and the Doppler index as the cube stores it
    std::vector<int2> tab((size_t)n_frames * n_out);
    for (int f = 0; f < n_frames; ++f)
        for (int i = 0; i < n_out; ++i) {
            const size_t e = (size_t)f * n_out + i;
            const int a = h_ang_idx[e], k = h_vel_idx[e];
            MMW_REQUIRE(a >= 0 && a < A, "frame %d, entry %d: angle index %d is not in [0, %d)", f, i, a, A);
            MMW_REQUIRE(k >= 0 && k < C, "frame %d, entry %d: Doppler index %d is not in [0, %d)", f, i, k, C);
            tab[e] = make_int2(((a - A / 2) % A + A) % A, k);
        }
    DbsArgs da{};
    da.V = V, da.S = S, da.C = C, da.A = A, da.n_out = n_out;
    for (int j = 0; j < n; ++j) {       // np.hanning(n) over the SUBSET (process_dbs_enhanced :290-295); zero only at its two ends
        const float w = (float)np_window(TAB_HANN, j, n);
        if (w == 0.f) continue;
        if (da.n_eff == 0) da.j0 = j;
        da.ant[da.n_eff] = n_rx ? h_rx[j] : j;
        da.w[da.n_eff++] = w;
    }
    MMW_TRY(get_table<float>(ctx, TAB_TWIDDLE, A, (const void **)&da.tw));
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t cube_bytes = (size_t)V * S * C * sizeof(float2), tab_bytes = up(tab.size() * sizeof(int2));
    const long chunk = d_rd ? std::min(n_frames, 65535) : dbs_chunk_frames(ctx, cube_bytes, n_frames);
    MMW_TRY(ensure_scratch(ctx, tab_bytes + (d_rd ? 0 : (size_t)chunk * cube_bytes)));
    int2 *d_tab = (int2 *)ctx->scratch;
    MMW_HIP(hipMemcpyAsync(d_tab, tab.data(), tab.size() * sizeof(int2), hipMemcpyHostToDevice, ctx->stream));
    MMW_HIP(hipStreamSynchronize(ctx->stream));     // the table is host memory of this call
    const bool tw_lds = (size_t)A * sizeof(float2) <= 32768;
    const size_t lds = tw_lds ? (size_t)A * sizeof(float2) : 0;
    const dim3 block(256);
    for (long f0 = 0; f0 < n_frames; f0 += chunk) {
        const int nf = (int)std::min<long>(chunk, n_frames - f0);
        char *rd = d_rd ? (char *)d_rd + (size_t)f0 * cube_bytes : (char *)ctx->scratch + tab_bytes;
        MMW_TRY(range_doppler_impl(ctx, (const char *)d_cubes + (size_t)f0 * cube_bytes, rd, nullptr, nf, V, S, C));
        ProfScope ps(ctx, "dbs_sharpen");
        da.rd = (const float2 *)rd;
        da.tab = d_tab + (size_t)f0 * n_out;
        da.out = d_out + (size_t)f0 * S * n_out;
        const dim3 grid((unsigned)(((long)S * n_out + 255) / 256), (unsigned)nf);
        if (tw_lds) hipLaunchKernelGGL(k_dbs_sharpen<true>, grid, block, lds, ctx->stream, da);
        else hipLaunchKernelGGL(k_dbs_sharpen<false>, grid, block, 0, ctx->stream, da);
        MMW_TRY(check_launch("dbs_sharpen"));
    }
    return MMW_OK;
}

int mmw_mean_over_range(mmw_ctx *ctx, const float *d_mag, float *d_out, int n_frames, int A, int S, int C,
                        int s_lo, int s_hi) {
    MMW_REQUIRE(ctx && d_mag && d_out, "null argument");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_frames >= 0 && A > 0 && S > 0 && C > 0, "bad shape");
    MMW_REQUIRE(0 <= s_lo && s_lo < s_hi && s_hi <= S, "empty or out-of-range row interval [%d, %d)", s_lo, s_hi);
    const long total = (long)n_frames * A * C;
    if (!total) return MMW_OK;
    hipLaunchKernelGGL(k_mean_over_range, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, d_mag, d_out,
                       n_frames, A, S, C, s_lo, s_hi);
    return check_launch("mean_over_range");
}

int mmw_doppler_azimuth(mmw_ctx *ctx, const void *d_cubes, float *d_out, int n_frames, int V, int S, int C, int A,
                        int s_lo, int s_hi, int flags) {
    MMW_REQUIRE(ctx && d_cubes && d_out, "null argument");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_frames >= 0 && V > 0 && S > 0 && C > 0 && A >= V, "bad shape (need A >= V)");
    MMW_REQUIRE(0 <= s_lo && s_lo < s_hi && s_hi <= S, "empty or out-of-range row interval [%d, %d)", s_lo, s_hi);
    MMW_REQUIRE((flags & ~(MMW_ANGLE_NO_WINDOW | MMW_ANGLE_NO_SHIFT)) == 0, "unknown flag bits %d", flags);
    if (n_frames == 0) return MMW_OK;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t cube_bytes = (size_t)V * S * C * sizeof(float2);
    long chunk = std::min<long>(n_frames, 65535);
    while (chunk > 1 && up(chunk * cube_bytes) + angle_mean_work_bytes((int)chunk, V, S, C, A, s_hi - s_lo) > ((size_t)1 << 30))
        chunk = (chunk + 1) / 2;
    const size_t work_bytes = angle_mean_work_bytes((int)chunk, V, S, C, A, s_hi - s_lo);
    MMW_TRY(ensure_scratch(ctx, up(chunk * cube_bytes) + work_bytes));
    char *d_rd = (char *)ctx->scratch, *d_work = d_rd + up(chunk * cube_bytes);
    for (long f0 = 0; f0 < n_frames; f0 += chunk) {
        const int nf = (int)std::min<long>(chunk, n_frames - f0);
        MMW_TRY(range_doppler_impl(ctx, (const char *)d_cubes + (size_t)f0 * cube_bytes, d_rd, nullptr, nf, V, S, C));
        MMW_TRY(angle_mean_impl(ctx, d_rd, d_work, work_bytes, d_out + (size_t)f0 * C * A, nf, V, S, C, A, s_lo, s_hi, flags));
    }
    return MMW_OK;
}

int mmw_doppler_azimuth_zoom(mmw_ctx *ctx, const void *d_cubes, float *d_out, int n_frames, int V, int S, int C, int A,
                             int s_lo, int s_hi, int n_used, const double *h_freq, int M, int flags) {
    MMW_REQUIRE(ctx && d_cubes && d_out && h_freq, "null argument");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_frames >= 0 && V > 0 && S > 0 && C > 0 && A >= V && M > 0, "bad shape (need A >= V, M > 0)");
    MMW_REQUIRE(0 <= s_lo && s_lo < s_hi && s_hi <= S, "empty or out-of-range row interval [%d, %d)", s_lo, s_hi);
    MMW_REQUIRE(n_used > 0 && n_used <= C, "zoom transform defined for %d chirps, the cube has %d", n_used, C);
    MMW_REQUIRE((flags & ~(MMW_ANGLE_NO_WINDOW | MMW_ANGLE_NO_SHIFT)) == 0, "unknown flag bits %d", flags);
    constexpr int RB = 16;
    MMW_REQUIRE((size_t)RB * n_used * sizeof(float2) <= 64 * 1024, "too many chirps for the zoom row buffer");
    if (n_frames == 0) return MMW_OK;
    ProfScope ps(ctx, "dopaz_zoom");
    const int Sk = s_hi - s_lo;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_freq = up((size_t)M * sizeof(double)), b_tab = up((size_t)n_used * M * sizeof(float2));
    const size_t f_rng = (size_t)V * S * C * sizeof(float2), f_zoom = (size_t)V * Sk * M * sizeof(float2);
    long chunk = std::min<long>(n_frames, 65535);
    auto need = [&](long c) { return up(c * f_rng) + up(c * f_zoom) + up(angle_mean_work_bytes((int)c, V, Sk, M, A, Sk)); };
    while (chunk > 1 && need(chunk) > ((size_t)1 << 30)) chunk = (chunk + 1) / 2;    // <= 1 GiB of intermediates per pass
    MMW_TRY(ensure_scratch(ctx, b_freq + b_tab + need(chunk)));
    char *base = (char *)ctx->scratch;
    double *d_freq = (double *)base;
    float2 *d_tab = (float2 *)(base + b_freq);
    char *d_rng = base + b_freq + b_tab;
    char *d_zoom = d_rng + up((size_t)chunk * f_rng);
    char *d_mag = d_zoom + up((size_t)chunk * f_zoom);
    // chirp-z form (mmw_czt.h) unless the list has no usable plan; MMW_ZOOM_DIRECT=1 keeps the direct n_used x M table
    const CztPlan *plan = nullptr;
    if (czt_length(n_used) > 0 && !env_int("MMW_ZOOM_DIRECT", 0)) MMW_TRY(czt_plan(ctx, h_freq, M, n_used, &plan));
    if (!plan) {
        MMW_HIP(hipMemcpyAsync(d_freq, h_freq, (size_t)M * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        MMW_HIP(hipStreamSynchronize(ctx->stream));     // h_freq is caller-owned host memory
        const long tab_n = (long)n_used * M;
        hipLaunchKernelGGL(k_zoom_table, dim3((unsigned)((tab_n + 255) / 256)), dim3(256), 0, ctx->stream, d_freq, d_tab,
                           n_used, M);
        MMW_TRY(check_launch("zoom_table"));
    }
    for (long f0 = 0; f0 < n_frames; f0 += chunk) {
        const int nf = (int)((n_frames - f0 < chunk) ? n_frames - f0 : chunk);
        FftArgs a{};                                 // range FFT, Hann(S) x Hann(C) folded into the load
        a.in = (const char *)d_cubes + (size_t)f0 * f_rng;
        a.out = d_rng;
        a.outer = nf * V;
        a.inner = C;
        a.n_in = S;
        a.in_outer_stride = a.out_outer_stride = (long)S * C;
        a.in_axis_stride = a.out_axis_stride = C;
        a.in_inner_stride = a.out_inner_stride = 1;
        MMW_TRY(get_table<float>(ctx, TAB_HANN, S, &a.win_axis));
        MMW_TRY(get_table<float>(ctx, TAB_HANN, C, &a.win_inner));
        a.scale = 1.0;
        MMW_TRY((launch_fft_axis<float, float>(ctx, a, S, false)));
        const long rows = (long)nf * V * Sk;
        if (plan) {
            CztArgs z{};
            z.x = (const float2 *)d_rng;
            z.outer_stride = (long)S * C;
            z.inner_stride = C;
            z.elem_stride = 1;
            z.s_lo = s_lo;
            z.s_keep = Sk;
            z.M = M;
            z.rows = rows;
            z.out = (float2 *)d_zoom;
            MMW_TRY(launch_czt_rows(ctx, *plan, z));
        } else {
            hipLaunchKernelGGL((k_zoom_rows<RB>), dim3((unsigned)((rows + RB - 1) / RB), (unsigned)((M + 255) / 256)), dim3(256),
                               (size_t)RB * n_used * sizeof(float2), ctx->stream, (const float2 *)d_rng, d_tab,
                               (float2 *)d_zoom, S, C, s_lo, Sk, n_used, M, rows);
            MMW_TRY(check_launch("zoom_rows"));
        }
        // antenna window + zero-padded angle FFT + |.| on [nf][V][Sk][M] and the mean over the kept range bins
        MMW_TRY(angle_mean_impl(ctx, d_zoom, d_mag, up(angle_mean_work_bytes((int)chunk, V, Sk, M, A, Sk)), d_out + (size_t)f0 * M * A, nf, V, Sk, M,
                                A, 0, Sk, flags));
    }
    return MMW_OK;
}

int mmw_diag_czt_runs(const double *h_freq, int M, int n_used, int *h_runs, int cap, int *n_runs) {
    MMW_REQUIRE(h_freq && n_runs && M > 0 && n_used > 0 && cap >= 0 && (cap == 0 || h_runs), "bad argument");
    const int L = czt_length(n_used);
    *n_runs = 0;
    if (L <= 0) return MMW_OK;              // no chirp-z length for this many input points
    const auto runs = czt_runs(h_freq, M, L - n_used + 1);
    *n_runs = (int)runs.size();
    for (int i = 0; i < *n_runs && i < cap; ++i) {          // (offset, length, filled with zeros) per run
        h_runs[3 * i] = std::get<0>(runs[i]);
        h_runs[3 * i + 1] = std::get<1>(runs[i]);
        h_runs[3 * i + 2] = std::get<2>(runs[i]) ? 1 : 0;
    }
    return MMW_OK;
}

}  // extern "C"
