// Translation unit of the CFAR entry points (mmw_cfar.h), the batched ground detector (mmw_ground.h), the batched sequential
// detector (mmw_seq.h) and the batched range detector (mmw_range_detect.h).
#include "mmw_entry.h"
#include "mmw_cfar.h"
#include "mmw_ground.h"
#include "mmw_seq.h"
#include "mmw_range_detect.h"

#include <algorithm>

using namespace mmw;

// ------------------------------------------------------------------ CFAR
int mmw::cfar2d_impl(mmw_ctx *ctx, const double *d_X, double *d_thr, double *d_noise, uint8_t *d_mask, int n_frames,
                     int R, int D, int kind, int train_r, int train_d, int guard_r, int guard_d, double scale,
                     int k_rank) {
    MMW_REQUIRE(ctx && d_X, "null argument");
    MMW_REQUIRE(n_frames >= 0 && R > 0 && D > 0, "bad shape");
    MMW_REQUIRE(train_r >= 0 && train_d >= 0 && guard_r >= 0 && guard_d >= 0, "negative window size");
    MMW_REQUIRE(kind == MMW_CFAR_CA || kind == MMW_CFAR_OS, "2-D CFAR kind must be CA or OS");
    MMW_REQUIRE(n_frames <= 65535, "at most 65535 frames per call");
    const int hr = train_r + guard_r, hd = train_d + guard_d;
    const long ntrain = (long)(2 * hr + 1) * (2 * hd + 1) - (long)(2 * guard_r + 1) * (2 * guard_d + 1);
    if (kind == MMW_CFAR_OS) MMW_REQUIRE(k_rank >= 1 && k_rank <= ntrain, "k_rank must be between 1 and %ld, got %d", ntrain, k_rank);
    if (kind == MMW_CFAR_OS && !d_thr && !d_noise && d_mask && scale > 0.0) {
        // mask only: one count per cell under test instead of an order-statistic selection (k_cfar2d_os_mask)
        // the GUI's window (gui_configs/processor_params.yaml: [5,5] / [3,2]) and the (4,4)/(2,2) of the tests: four cells per thread
        if (n_frames > 0 && opt_int(ctx, "MMW_OS_MASK_FORM", 1) == 1) {
            Cfar2dArgs a{d_X, nullptr, nullptr, d_mask, R, D, kind, train_r, train_d, guard_r, guard_d, scale, k_rank, 0};
            const dim3 grid((D + OSV_T - 1) / OSV_T, (R + OSV_T - 1) / OSV_T, n_frames);
#define MMW_OSV(tr, td, gr, gd) \
    if (train_r == tr && train_d == td && guard_r == gr && guard_d == gd) { \
        ProfScope ps(ctx, "cfar"); \
        hipLaunchKernelGGL((k_cfar2d_os_mask_v<tr, td, gr, gd>), grid, dim3(256), 0, ctx->stream, a); \
        return check_launch("cfar2d_os_mask_v"); \
    }
            MMW_OSV(5, 5, 3, 2)
            MMW_OSV(4, 4, 2, 2)
#undef MMW_OSV
        }
        const int TW = OSM_TC + 2 * hd, TH = OSM_TR + 2 * hr, TWp = ((TW + 15) / 32) * 32 + 16;
        const size_t lds_m = (size_t)TH * TWp * sizeof(double);
        if (lds_m <= 64 * 1024) {
            if (n_frames == 0) return MMW_OK;
            ProfScope ps(ctx, "cfar");
            Cfar2dArgs a{d_X, nullptr, nullptr, d_mask, R, D, kind, train_r, train_d, guard_r, guard_d, scale, k_rank, 0};
            dim3 grid((D + OSM_TC - 1) / OSM_TC, (R + OSM_TR - 1) / OSM_TR, n_frames);
            hipLaunchKernelGGL(k_cfar2d_os_mask, grid, dim3(OSM_TR * OSM_TC), lds_m, ctx->stream, a);
            return check_launch("cfar2d_os_mask");
        }
    }
    MMW_REQUIRE(2 * hd + 1 <= 512, "Doppler window too wide for the exact summation order");
    if (kind == MMW_CFAR_CA && D == 2 * hd + 1 && R >= 2 * hr + 1) {
        // one valid column: NumPy sums each window as one run (k_cfar2d_ca_1col)
        MMW_REQUIRE((long)(2 * hr + 1) * (2 * hd + 1) <= 0x7fffffffL, "CFAR window too large");
        if (n_frames == 0) return MMW_OK;
        ProfScope ps(ctx, "cfar");
        Cfar2dArgs a{d_X, d_thr, d_noise, d_mask, R, D, kind, train_r, train_d, guard_r, guard_d, scale, k_rank, 0};
        hipLaunchKernelGGL(k_cfar2d_ca_1col, dim3((unsigned)(((long)R * D + 255) / 256), n_frames), dim3(256), 0, ctx->stream, a);
        return check_launch("cfar2d_ca_1col");
    }
    if (kind == MMW_CFAR_CA) {
        // 32 x 32 tile (k_cfar2d_ca) while tile + halo + row-sum tables fit the default LDS limit
        const size_t th = CA_TR + 2 * hr, tw = CA_TC + 2 * hd;
        const size_t lds_ca = (th * tw + 2 * th * CA_TC) * sizeof(double);
        if (lds_ca <= 64 * 1024) {
            if (n_frames == 0) return MMW_OK;
            ProfScope ps(ctx, "cfar");
            Cfar2dArgs a{d_X, d_thr, d_noise, d_mask, R, D, kind, train_r, train_d, guard_r, guard_d, scale, k_rank, 0};
            dim3 grid((D + CA_TC - 1) / CA_TC, (R + CA_TR - 1) / CA_TR, n_frames);
            hipLaunchKernelGGL(k_cfar2d_ca, grid, dim3(256), lds_ca, ctx->stream, a);
            return check_launch("cfar2d_ca");
        }
    }
    const size_t n_tile = (size_t)(CFAR_TR + 2 * hr) * (CFAR_TC + 2 * hd);
    size_t npad = 1;
    while (npad < n_tile) npad <<= 1;
    const size_t aux_ca = 2 * (size_t)(CFAR_TR + 2 * hr) * CFAR_TC * sizeof(double);     // row-sum tables
    size_t aux_os = npad * 8 + npad * 2 + ((n_tile + 1) & ~(size_t)1) * 2 + 16;         // keys, positions, ranks
    const size_t integ = (size_t)(OS_COARSE - 1) * (CFAR_TR + 2 * hr + 1) * (CFAR_TC + 2 * hd + 1) * 2;
    const bool os_fast = kind == MMW_CFAR_OS && npad <= 1024 && n_tile * sizeof(double) + aux_os + integ <= 64 * 1024;
    if (os_fast) aux_os += integ;
    const size_t lds = n_tile * sizeof(double) + (kind == MMW_CFAR_OS ? aux_os : aux_ca);
    MMW_REQUIRE(kind != MMW_CFAR_OS || npad <= 32768, "OS-CFAR window too large");
    if (lds > 64 * 1024) return set_error(MMW_ERR_UNSUPPORTED, "CFAR window %dx%d too large for the LDS tile", 2 * hr + 1, 2 * hd + 1);
    if (n_frames == 0) return MMW_OK;
    ProfScope ps(ctx, "cfar");
    Cfar2dArgs a{d_X, d_thr, d_noise, d_mask, R, D, kind, train_r, train_d, guard_r, guard_d, scale, k_rank, os_fast ? 1 : 0};
    dim3 grid((D + CFAR_TC - 1) / CFAR_TC, (R + CFAR_TR - 1) / CFAR_TR, n_frames);
    hipLaunchKernelGGL(k_cfar2d, grid, dim3(CFAR_TR * CFAR_TC), lds, ctx->stream, a);
    return check_launch("cfar2d");
}

int mmw::compact2d_impl(mmw_ctx *ctx, const uint8_t *d_mask, int32_t *d_dets, int32_t *d_counts, int n_frames,
                        int R, int D, int cap) {
    MMW_REQUIRE(ctx && d_mask && d_dets && d_counts, "null argument");
    MMW_REQUIRE(n_frames >= 0 && R > 0 && D > 0 && cap >= 0, "bad shape");
    if (n_frames == 0) return MMW_OK;
    ProfScope ps(ctx, "compact");
    hipLaunchKernelGGL(k_compact2d, dim3(n_frames), dim3(1024), 0, ctx->stream, d_mask, d_dets, d_counts, R, D, cap);
    return check_launch("compact2d");
}

static int ground_flag_all(const mmw_ctx *ctx) { return opt_int(ctx, "MMW_GROUND_FLAG_ALL", 0) != 0 ? 1 : 0; }

static int cfar1d_args_ok(int kind, int num_train, int num_guard, int k_rank) {
    MMW_REQUIRE(num_train >= 0 && num_guard >= 0, "bad CFAR window");
    MMW_REQUIRE(kind >= MMW_CFAR_CA && kind <= MMW_CFAR_SO, "unknown CFAR kind %d", kind);
    MMW_REQUIRE(num_train <= 512, "num_train too large for the exact summation order");
    if (kind == MMW_CFAR_OS)
        MMW_REQUIRE(k_rank >= 1 && k_rank <= 2 * num_train, "k_rank must be between 1 and %d, got %d", 2 * num_train, k_rank);
    return MMW_OK;
}

// k_cfar1d_gated on the listed rows of every frame's plane[F][R][D], then the ordered compaction (arguments judged by the caller)
static int cfar1d_rows_impl(mmw_ctx *ctx, const double *d_mag64, const int32_t *d_rows, const int32_t *d_nrows, uint8_t *d_mask,
                            int32_t *d_dets, int32_t *d_counts, int n_frames, int R, int D, int kind, int num_train,
                            int num_guard, double scale, int k_rank, int cap) {
    Cfar1dArgs a{d_mag64, nullptr, nullptr, nullptr, 0, D, kind, num_train, num_guard, scale, k_rank};
    {
        ProfScope ps(ctx, "cfar");
        hipLaunchKernelGGL(k_cfar1d_gated, dim3((unsigned)(((long)R * D + 255) / 256), n_frames), dim3(256), 0, ctx->stream, a,
                           (const int32_t *)nullptr, d_rows, d_nrows, d_mask, R);
        MMW_TRY(check_launch("cfar1d_rows"));
    }
    return compact2d_impl(ctx, d_mask, d_dets, d_counts, n_frames, R, D, cap);
}

// Every argument of mmw_range_detect is judged here, before the context is touched: the function is not given the context, so a
// refused call cannot enqueue anything and needs no device (tests/cpp/sar_range_sanitize.cpp relies on it).
static int range_detect_validate(bool have_ctx, const void *d_cubes, int n_frames, int V, int S, int C, int chirp_idx, int kind,
                                 int num_train, int num_guard, int k_rank, const void *d_dets, const void *d_counts, int cap) {
    MMW_REQUIRE(have_ctx && d_cubes && d_dets && d_counts, "null argument (ctx %d, d_cubes %d, d_dets %d, d_counts %d)", (int)have_ctx,
                d_cubes != nullptr, d_dets != nullptr, d_counts != nullptr);
    MMW_REQUIRE(n_frames >= 0 && n_frames <= 65535, "n_frames is %d (0 to 65535 per call)", n_frames);
    MMW_REQUIRE(V > 0 && S > 0 && C > 0, "bad shape: V %d, S %d, C %d must all be positive", V, S, C);
    MMW_REQUIRE(chirp_idx >= -C && chirp_idx < C, "chirp_idx %d is not a chirp of [-%d, %d)", chirp_idx, C, C);
    MMW_REQUIRE(cap >= 0, "cap is %d", cap);
    return cfar1d_args_ok(kind, num_train, num_guard, k_rank);
}

extern "C" {

int mmw_range_detect(mmw_ctx *ctx, const void *d_cubes, int n_frames, int V, int S, int C, int chirp_idx, int kind, int num_train,
                     int num_guard, double scale, int k_rank, double *d_profile, double *d_thr, int32_t *d_dets, int32_t *d_counts,
                     int cap) {
    MMW_TRY(range_detect_validate(ctx != nullptr, d_cubes, n_frames, V, S, C, chirp_idx, kind, num_train, num_guard, k_rank, d_dets,
                                  d_counts, cap));
    if (S > RANGE_DETECT_MAX_S)
        return set_error(MMW_ERR_UNSUPPORTED, "range detector: %d range cells, at most %d (one flag byte per cell in the LDS)", S,
                         RANGE_DETECT_MAX_S);
    if (n_frames == 0) return MMW_OK;
    // the profile pass works in the head of the scratch; a profile nobody asked for goes behind it
    const size_t head = ((size_t)n_frames * V * S * 2 * sizeof(double) + 255) & ~(size_t)255;
    if (!d_profile) {
        MMW_JOIN(ctx);
        MMW_TRY(ensure_scratch(ctx, head + (size_t)n_frames * S * sizeof(double)));
        d_profile = (double *)((char *)ctx->scratch + head);
    }
    MMW_TRY(range_profile_impl<double>(ctx, d_cubes, d_profile, n_frames, V, S, C, chirp_idx));
    Cfar1dArgs a{d_profile, d_thr, nullptr, nullptr, n_frames, S, kind, num_train, num_guard, scale, k_rank};
    ProfScope ps(ctx, "range_detect");
    hipLaunchKernelGGL(k_range_detect, dim3(n_frames), dim3(256), (size_t)S, ctx->stream, a, d_dets, d_counts, cap);
    return check_launch("range_detect");
}

int mmw_cfar2d(mmw_ctx *ctx, const double *d_X, double *d_thr, double *d_noise, uint8_t *d_mask, int n_frames,
               int R, int D, int kind, int train_r, int train_d, int guard_r, int guard_d, double scale,
               int k_rank) {
    MMW_REQUIRE(ctx, "ctx is null");
    MMW_JOIN(ctx);
    return cfar2d_impl(ctx, d_X, d_thr, d_noise, d_mask, n_frames, R, D, kind, train_r, train_d, guard_r, guard_d, scale,
                       k_rank);
}

int mmw_cfar1d(mmw_ctx *ctx, const double *d_x, double *d_thr, double *d_noise, uint8_t *d_mask, int n_rows,
               int L, int kind, int num_train, int num_guard, double scale, int k_rank) {
    MMW_REQUIRE(ctx && d_x, "null argument");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_rows >= 0 && L > 0 && num_train >= 0 && num_guard >= 0, "bad shape");
    MMW_REQUIRE(kind >= MMW_CFAR_CA && kind <= MMW_CFAR_SO, "unknown CFAR kind %d", kind);
    MMW_REQUIRE(num_train <= 512, "num_train too large for the exact summation order");
    if (kind == MMW_CFAR_OS)
        MMW_REQUIRE(k_rank >= 1 && k_rank <= 2 * num_train, "k_rank must be between 1 and %d, got %d", 2 * num_train, k_rank);
    if (n_rows == 0) return MMW_OK;
    Cfar1dArgs a{d_x, d_thr, d_noise, d_mask, n_rows, L, kind, num_train, num_guard, scale, k_rank};
    const long total = (long)n_rows * L;
    hipLaunchKernelGGL(k_cfar1d, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, a);
    return check_launch("cfar1d");
}

int mmw_compact2d(mmw_ctx *ctx, const uint8_t *d_mask, int32_t *d_dets, int32_t *d_counts, int n_frames,
                  int R, int D, int cap) {
    MMW_REQUIRE(ctx, "ctx is null");
    MMW_JOIN(ctx);
    return compact2d_impl(ctx, d_mask, d_dets, d_counts, n_frames, R, D, cap);
}

// One call for the per-frame detection pipeline of RangeDopplerDetector2D over a batch: RD cube (fp32, all
// antennas), float64 |RD| of antenna 0, 2-D CFAR, ordered compaction.  The stages run back to back on the context
// stream: running the RD kernel beside the detection kernels on CU-masked queues was measured 2x SLOWER, because the
// float64 FFT and CFAR kernels are latency/ALU bound and scale with the CUs they get (unlike the angle kernel).
int mmw_detect_batch(mmw_ctx *ctx, const void *d_cubes, void *d_rd, double *d_mag64, uint8_t *d_mask,
                     int32_t *d_dets, int32_t *d_counts, float *d_l1, int n_frames, int V, int S, int C, int cfar_kind,
                     int train_r, int train_d, int guard_r, int guard_d, double scale, int k_rank, int cap) {
    MMW_REQUIRE(ctx && d_cubes && d_rd && d_mag64 && d_mask && d_dets && d_counts, "null argument");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_frames >= 0 && n_frames <= 65535 && V > 0 && S > 0 && C > 0 && cap >= 0, "bad shape");
    if (n_frames == 0) return MMW_OK;
    MMW_TRY(range_doppler_impl(ctx, d_cubes, d_rd, nullptr, n_frames, V, S, C, RawView{1, 0}, d_l1));
    MMW_TRY(range_doppler_mag64_impl(ctx, d_cubes, d_mag64, n_frames, V, S, C, 0));
    MMW_TRY(cfar2d_impl(ctx, d_mag64, nullptr, nullptr, d_mask, n_frames, S, C, cfar_kind, train_r, train_d, guard_r,
                        guard_d, scale, k_rank));
    return compact2d_impl(ctx, d_mask, d_dets, d_counts, n_frames, S, C, cap);
}

// ------------------------------------------------------------------ batched ground detector (mmw_ground.h)
int mmw_ground_candidates(mmw_ctx *ctx, const void *d_cubes, const double *d_bins, double *d_profile, double *d_cand,
                          int32_t *d_counts, int n_frames, int V, int S, int C) {
    MMW_REQUIRE(ctx && d_cubes && d_bins && d_profile && d_cand && d_counts, "null argument");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_frames >= 0 && n_frames <= 65535 && V > 0 && S >= 3 && C > 0, "bad shape");
    MMW_REQUIRE((size_t)S * 2 * sizeof(double) <= 48 * 1024, "range profile of %d samples does not fit the picker's LDS", S);
    if (n_frames == 0) return MMW_OK;
    MMW_TRY(range_profile_impl<double>(ctx, d_cubes, d_profile, n_frames, V, S, C, 0));
    ProfScope ps(ctx, "ground");
    hipLaunchKernelGGL(k_ground_peaks, dim3(n_frames), dim3(256), (size_t)S * 2 * sizeof(double), ctx->stream, d_profile, d_bins,
                       d_cand, d_counts, S, GROUND_COARSE, ground_flag_all(ctx));
    return check_launch("ground_peaks");
}

// k_ground_peaks on a caller's profiles (tests/test_gpu_ground_pick.py): the picker alone, at either max_peaks the detector uses
int mmw_diag_ground_pick(mmw_ctx *ctx, const double *d_profile, const double *d_bins, double *d_cand, int32_t *d_counts, int n_rows,
                         int S, int max_peaks) {
    MMW_REQUIRE(ctx && d_profile && d_bins && d_cand && d_counts, "null argument");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_rows >= 0 && n_rows <= 65535 && S >= 3, "bad shape");
    MMW_REQUIRE(max_peaks == GROUND_FINE || max_peaks == GROUND_COARSE, "max_peaks is %d (%d or %d)", max_peaks, GROUND_FINE,
                GROUND_COARSE);
    MMW_REQUIRE((size_t)S * 2 * sizeof(double) <= 48 * 1024, "range profile of %d samples does not fit the picker's LDS", S);
    if (n_rows == 0) return MMW_OK;
    ProfScope ps(ctx, "ground");
    hipLaunchKernelGGL(k_ground_peaks, dim3(n_rows), dim3(256), (size_t)S * 2 * sizeof(double), ctx->stream, d_profile, d_bins,
                       d_cand, d_counts, S, max_peaks, ground_flag_all(ctx));
    return check_launch("ground_peaks");
}

int mmw_ground_zoom_candidates(mmw_ctx *ctx, const void *d_cubes, const double *d_cand, const int32_t *d_counts, double *d_spec,
                               double *d_zcand, int32_t *d_zcounts, int n_frames, int V, int S, int C, double half_width_m,
                               double hi_cap_m, double fs, double range_max_m) {
    MMW_REQUIRE(ctx && d_cubes && d_cand && d_counts && d_spec && d_zcand && d_zcounts, "null argument");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_frames >= 0 && n_frames <= 65535 && V > 0 && S >= 3 && C > 0, "bad shape");
    MMW_REQUIRE(S <= 256 * ZOOM_BINS_PER_THREAD, "zoom window of %d bins: at most %d", S, 256 * ZOOM_BINS_PER_THREAD);
    MMW_REQUIRE(half_width_m > 0.0 && fs > 0.0 && range_max_m > 0.0, "bad zoom window parameters");
    if (n_frames == 0) return MMW_OK;
    const void *hann;
    MMW_TRY(get_table<double>(ctx, TAB_HANN, S, &hann));
    const int vb = std::max(1, std::min(std::min(V, ZOOM_VB), (int)((48 * 1024) / ((size_t)S * sizeof(double2)))));
    const size_t lds = std::max((size_t)vb * S * sizeof(double2), (size_t)S * 2 * sizeof(double));
    ZoomArgs a{(const float2 *)d_cubes, (const double *)hann, d_cand, d_counts, d_spec, d_zcand, d_zcounts, V, S, C, vb,
               half_width_m, hi_cap_m, fs, range_max_m, ground_flag_all(ctx)};
    ProfScope ps(ctx, "ground");
    hipLaunchKernelGGL(k_ground_zoom, dim3(GROUND_COARSE, n_frames), dim3(256), lds, ctx->stream, a);
    return check_launch("ground_zoom");
}

int mmw_cfar1d_gated(mmw_ctx *ctx, const double *d_mag64, const int32_t *d_gate, uint8_t *d_mask, int32_t *d_dets,
                     int32_t *d_counts, int n_frames, int R, int D, int kind, int num_train, int num_guard, double scale,
                     int k_rank, int cap) {
    MMW_REQUIRE(ctx && d_mag64 && d_gate && d_mask && d_dets && d_counts, "null argument");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_frames >= 0 && n_frames <= 65535 && R > 0 && D > 0 && cap >= 0 && num_train >= 0 && num_guard >= 0,
                "bad shape");
    MMW_REQUIRE(kind >= MMW_CFAR_CA && kind <= MMW_CFAR_SO, "unknown CFAR kind %d", kind);
    MMW_REQUIRE(num_train <= 512, "num_train too large for the exact summation order");
    if (kind == MMW_CFAR_OS)
        MMW_REQUIRE(k_rank >= 1 && k_rank <= 2 * num_train, "k_rank must be between 1 and %d, got %d", 2 * num_train, k_rank);
    if (n_frames == 0) return MMW_OK;
    Cfar1dArgs a{d_mag64, nullptr, nullptr, nullptr, 0, D, kind, num_train, num_guard, scale, k_rank};
    {
        ProfScope ps(ctx, "cfar");
        hipLaunchKernelGGL(k_cfar1d_gated, dim3((unsigned)(((long)R * D + 255) / 256), n_frames), dim3(256), 0, ctx->stream, a,
                           d_gate, (const int32_t *)nullptr, (const int32_t *)nullptr, d_mask, R);
        MMW_TRY(check_launch("cfar1d_gated"));
    }
    return compact2d_impl(ctx, d_mask, d_dets, d_counts, n_frames, R, D, cap);
}

// mmw_cfar1d_gated with the rows of each frame named by a list (the second half of mmw_seq_detect_plane on a caller's plane)
int mmw_cfar1d_rows(mmw_ctx *ctx, const double *d_mag64, const int32_t *d_rows, const int32_t *d_nrows, uint8_t *d_mask,
                    int32_t *d_dets, int32_t *d_counts, int n_frames, int R, int D, int kind, int num_train, int num_guard,
                    double scale, int k_rank, int cap) {
    MMW_REQUIRE(ctx && d_mag64 && d_rows && d_nrows && d_mask && d_dets && d_counts, "null argument");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_frames >= 0 && n_frames <= 65535 && R > 0 && D > 0 && cap >= 0, "bad shape");
    MMW_TRY(cfar1d_args_ok(kind, num_train, num_guard, k_rank));
    if (n_frames == 0) return MMW_OK;
    return cfar1d_rows_impl(ctx, d_mag64, d_rows, d_nrows, d_mask, d_dets, d_counts, n_frames, R, D, kind, num_train, num_guard,
                            scale, k_rank, cap);
}

// ------------------------------------------------------------------ batched sequential detector (mmw_seq.h)
int mmw_seq_route(mmw_ctx *ctx, int S, int C) {
    if (opt_int(ctx, "MMW_SEQ_FULL_PLANE", SEQ_FULL_PLANE_DEFAULT) != 0) return 1;
    return (S > 0 && C > 0 && seq_lds_bytes(S, C) <= SEQ_LDS_MAX) ? 0 : 1;
}

int mmw_seq_rows(mmw_ctx *ctx, const double *d_profile, int32_t *d_rows, int32_t *d_nrows, int n_frames, int S, int kind,
                 int num_train, int num_guard, double scale, int k_rank) {
    MMW_REQUIRE(ctx && d_profile && d_rows && d_nrows, "null argument");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_frames >= 0 && n_frames <= 65535 && S > 0, "bad shape");
    MMW_REQUIRE((size_t)S * 2 * sizeof(double) <= 48 * 1024, "range profile of %d samples does not fit the row picker's LDS", S);
    MMW_TRY(cfar1d_args_ok(kind, num_train, num_guard, k_rank));
    if (n_frames == 0) return MMW_OK;
    Cfar1dArgs a{d_profile, nullptr, nullptr, nullptr, n_frames, S, kind, num_train, num_guard, scale, k_rank};
    ProfScope ps(ctx, "seq");
    hipLaunchKernelGGL(k_seq_rows, dim3(n_frames), dim3(256), (size_t)S * (sizeof(double) + 1), ctx->stream, a, d_rows, d_nrows);
    return check_launch("seq_rows");
}

int mmw_seq_detect(mmw_ctx *ctx, const void *d_cubes, const int32_t *d_rows, const int32_t *d_nrows, int32_t *d_dets,
                   int32_t *d_counts, int n_frames, int V, int S, int C, int kind, int num_train, int num_guard, double scale,
                   int k_rank, int cap, double *d_rowmag) {
    MMW_REQUIRE(ctx && d_cubes && d_rows && d_nrows && d_dets && d_counts, "null argument");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_frames >= 0 && n_frames <= 65535 && V > 0 && S > 0 && C > 0 && cap >= 0, "bad shape");
    MMW_TRY(cfar1d_args_ok(kind, num_train, num_guard, k_rank));
    const size_t lds = seq_lds_bytes(S, C);
    if (lds > SEQ_LDS_MAX)
        return set_error(MMW_ERR_UNSUPPORTED, "sequential row kernel: %d x %d needs %zu bytes of LDS (mmw_seq_route says so): "
                         "use mmw_seq_detect_plane", S, C, lds);
    if (n_frames == 0) return MMW_OK;
    SeqArgs a{};
    a.cubes = (const float2 *)d_cubes;
    const void *t;
    MMW_TRY(get_table<double>(ctx, TAB_HANN, S, &t));
    a.hann_s = (const double *)t;
    MMW_TRY(get_table<double>(ctx, TAB_HANN, C, &t));
    a.hann_c = (const double *)t;
    MMW_TRY(get_table<double>(ctx, TAB_TWIDDLE, S, &t));
    a.tw_s = (const double2 *)t;
    MMW_TRY(get_table<double>(ctx, TAB_TWIDDLE, C, &t));
    a.tw_c = (const double2 *)t;
    a.rows = d_rows;
    a.nrows = d_nrows;
    a.dets = d_dets;
    a.counts = d_counts;
    a.rowmag = d_rowmag;
    a.V = V;
    a.S = S;
    a.C = C;
    a.cap = cap;
    a.cfar = Cfar1dArgs{nullptr, nullptr, nullptr, nullptr, 0, C, kind, num_train, num_guard, scale, k_rank};
    if (lds > 64 * 1024)
        MMW_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_seq_detect), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds));         // per device, so on every call
    ProfScope ps(ctx, "seq");
    hipLaunchKernelGGL(k_seq_detect, dim3(n_frames), dim3(256), lds, ctx->stream, a);
    return check_launch("seq_detect");
}

int mmw_seq_detect_plane(mmw_ctx *ctx, const void *d_cubes, const int32_t *d_rows, const int32_t *d_nrows, double *d_mag64,
                         uint8_t *d_mask, int32_t *d_dets, int32_t *d_counts, int n_frames, int V, int S, int C, int kind,
                         int num_train, int num_guard, double scale, int k_rank, int cap) {
    MMW_REQUIRE(ctx && d_cubes && d_rows && d_nrows && d_mag64 && d_mask && d_dets && d_counts, "null argument");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_frames >= 0 && n_frames <= 65535 && V > 0 && S > 0 && C > 0 && cap >= 0, "bad shape");
    MMW_TRY(cfar1d_args_ok(kind, num_train, num_guard, k_rank));
    if (n_frames == 0) return MMW_OK;
    MMW_TRY(range_doppler_mag64_impl(ctx, d_cubes, d_mag64, n_frames, V, S, C, 0));
    return cfar1d_rows_impl(ctx, d_mag64, d_rows, d_nrows, d_mask, d_dets, d_counts, n_frames, S, C, kind, num_train, num_guard,
                            scale, k_rank, cap);
}

}  // extern "C"
