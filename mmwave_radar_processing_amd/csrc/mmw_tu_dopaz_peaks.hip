// Translation unit of the Doppler-azimuth peak pickers (mmw_dopaz_peaks.h).
#include <algorithm>
#include <climits>

#include "mmw_ctx.h"
#include "mmw_dopaz_peaks.h"

using namespace mmw;

namespace {

struct DzpCall {
    std::vector<int2> groups;
    int max_m = 0;
    double floor_ratio = 1.0;
    DzpRule rule{};
};

// Every argument is judged here, before the context is touched: the function is not given the context, so a refused call cannot
// enqueue anything and needs no device (tests/cpp/doppler_azimuth_peaks_sanitize.cpp relies on it).
int dzp_validate(bool need_ctx, bool have_ctx, const float *maps, int n_sets, int F, int n_rows, int A, const int32_t *h_groups, int G,
                 const int32_t *h_m, int a_lo, int a_hi, int a_zero, double min_threshold_dB, double prominence_dB,
                 const int32_t *row_peak, const int32_t *zero, DzpCall *call) {
    MMW_REQUIRE((have_ctx || !need_ctx) && maps && h_groups && row_peak && zero,
                "null argument (ctx %d, maps %d, h_groups %d, row_peak %d, zero %d)", (int)(have_ctx || !need_ctx), maps != nullptr,
                h_groups != nullptr, row_peak != nullptr, zero != nullptr);
    MMW_REQUIRE(n_sets >= 0 && F >= 0 && n_rows >= 0 && G >= 0, "negative count: n_sets %d, F %d, n_rows %d, G %d", n_sets, F, n_rows, G);
    MMW_REQUIRE(A >= 1, "A is %d angle bins", A);
    MMW_REQUIRE(0 <= a_lo && a_lo < a_hi && a_hi <= A, "column interval [%d, %d) is not inside 0 <= a_lo < a_hi <= %d", a_lo, a_hi, A);
    MMW_REQUIRE(a_lo <= a_zero && a_zero < a_hi, "a_zero %d is not a column of [%d, %d)", a_zero, a_lo, a_hi);
    MMW_REQUIRE(std::isfinite(min_threshold_dB) && min_threshold_dB >= 0.0, "min_threshold_dB %g is not a finite, non-negative number",
                min_threshold_dB);
    MMW_REQUIRE(std::isfinite(prominence_dB) && prominence_dB >= 0.0, "prominence_dB %g is not a finite, non-negative number",
                prominence_dB);
    call->groups.resize((size_t)G);
    for (int g = 0; g < G; ++g) {
        const int s1 = h_groups[2 * (size_t)g], s2 = h_groups[2 * (size_t)g + 1];
        MMW_REQUIRE(s1 >= 0 && s1 < n_sets && (s2 == -1 || (s2 >= 0 && s2 < n_sets)),
                    "group %d: (%d, %d) does not name sets of [0, %d) (second -1: a single set)", g, s1, s2, n_sets);
        MMW_REQUIRE(s1 != s2, "group %d names set %d twice", g, s1);
        call->groups[g] = make_int2(s1, s2);
    }
    call->max_m = h_m ? 0 : n_rows;
    for (int f = 0; h_m && f < F; ++f) {
        MMW_REQUIRE(h_m[f] >= 0 && h_m[f] <= n_rows, "frame %d: m is %d rows of %d", f, h_m[f], n_rows);
        call->max_m = std::max(call->max_m, (int)h_m[f]);
    }
    MMW_REQUIRE((double)n_sets * F * n_rows * A <= (double)INT_MAX && (double)G * F * std::max(n_rows, 1) <= (double)INT_MAX,
                "%d sets / %d groups x %d frames x %d rows x %d angle bins do not fit a 32-bit element index", n_sets, G, F, n_rows, A);
    if (A != 64) return set_error(MMW_ERR_UNSUPPORTED, "the Doppler-azimuth peak pickers are built for 64 angle bins, not %d", A);
    call->floor_ratio = std::pow(10.0, -min_threshold_dB / 20.0);
    call->rule.prom = std::pow(10.0, prominence_dB / 20.0);
    call->rule.fl_exact = call->floor_ratio == 1.0;
    call->rule.prom_exact = call->rule.prom == 1.0;
    return MMW_OK;
}

size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

extern "C" {

int mmw_doppler_azimuth_peaks(mmw_ctx *ctx, const float *d_maps, int n_sets, int F, int n_rows, int A, const int32_t *h_groups, int G,
                              const int32_t *h_m, int a_lo, int a_hi, int a_zero, double min_threshold_dB, double prominence_dB,
                              int32_t *d_row_peak, int32_t *d_zero) {
    DzpCall call;
    MMW_TRY(dzp_validate(true, ctx != nullptr, d_maps, n_sets, F, n_rows, A, h_groups, G, h_m, a_lo, a_hi, a_zero, min_threshold_dB,
                         prominence_dB, d_row_peak, d_zero, &call));
    if (F == 0 || G == 0) return MMW_OK;
    MMW_JOIN(ctx);
    ProfScope ps(ctx, "dopaz_peaks");
    // the two host tables of this call -> the head of the scratch
    const size_t g_bytes = (size_t)G * sizeof(int2), m_bytes = h_m ? (size_t)F * sizeof(int) : 0;
    MMW_TRY(ensure_scratch(ctx, up256(g_bytes) + up256(m_bytes)));
    char *d_tab = (char *)ctx->scratch;
    MMW_HIP(hipMemcpyAsync(d_tab, call.groups.data(), g_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (h_m) MMW_HIP(hipMemcpyAsync(d_tab + up256(g_bytes), h_m, m_bytes, hipMemcpyHostToDevice, ctx->stream));
    MMW_HIP(hipStreamSynchronize(ctx->stream));     // the tables are host memory of this call
    DzpArgs a{};
    a.maps = d_maps;
    a.set_stride = (long)F * n_rows * 64;
    a.groups = (const int2 *)d_tab;
    a.m = h_m ? (const int *)(d_tab + up256(g_bytes)) : nullptr;
    a.F = F, a.n_rows = n_rows, a.a_lo = a_lo, a.a_hi = a_hi, a.a_zero = a_zero;
    a.floor_ratio = call.floor_ratio;
    a.rule = call.rule;
    a.row_peak = d_row_peak;
    a.zero = d_zero;
    const size_t lds = dopaz_peaks_lds(call.max_m);
    const dim3 grid((unsigned)(G * F));
    if (lds <= DZP_LDS_MAX) {
        if (lds > 64 * 1024)
            MMW_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_dopaz_peaks<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)lds));
        hipLaunchKernelGGL(k_dopaz_peaks<true>, grid, dim3(256), lds, ctx->stream, a);
    } else {
        hipLaunchKernelGGL(k_dopaz_peaks<false>, grid, dim3(256), DZP_LDS_HEAD, ctx->stream, a);
    }
    return check_launch("dopaz_peaks");
}

int mmw_diag_doppler_azimuth_peaks_host(const float *h_maps, int n_sets, int F, int n_rows, int A, const int32_t *h_groups, int G,
                                        const int32_t *h_m, int a_lo, int a_hi, int a_zero, double min_threshold_dB,
                                        double prominence_dB, int32_t *h_row_peak, int32_t *h_zero) {
    DzpCall call;
    MMW_TRY(dzp_validate(false, false, h_maps, n_sets, F, n_rows, A, h_groups, G, h_m, a_lo, a_hi, a_zero, min_threshold_dB,
                         prominence_dB, h_row_peak, h_zero, &call));
    const int nc = a_hi - a_lo;
    const long set_stride = (long)F * n_rows * 64;
    std::vector<double> y((size_t)std::max(call.max_m, 1) * nc);
    for (int g = 0; g < G; ++g)
        for (int f = 0; f < F; ++f) {
            const int m = h_m ? h_m[f] : n_rows;
            const long frame = (long)f * n_rows * 64;
            const float *m1 = h_maps + call.groups[g].x * set_stride + frame;
            const float *m2 = call.groups[g].y >= 0 ? h_maps + call.groups[g].y * set_stride + frame : nullptr;
            double mx = 0.0;
            bool bad = false;
            for (int r = 0; r < m; ++r)
                for (int c = 0; c < nc; ++c) {
                    const double v = dzp_value(m1, m2, (long)r * 64 + a_lo + c);
                    bad |= !(v <= DBL_MAX);
                    mx = fmax(mx, v);
                    y[(size_t)r * nc + c] = v;
                }
            DzpRule R = call.rule;
            R.fl = mx * call.floor_ratio;
            int32_t *rp = h_row_peak + ((long)g * F + f) * n_rows;
            for (int r = 0; r < n_rows; ++r)
                rp[r] = r >= m ? DZP_NONE : (bad ? DZP_UNDECIDED : dzp_pick(DzpLine{y.data() + (size_t)r * nc, 1}, nc, R, true));
            h_zero[(long)g * F + f] = bad ? DZP_UNDECIDED : dzp_pick(DzpLine{y.data() + (a_zero - a_lo), nc}, m, R, false);
        }
    return MMW_OK;
}

}  // extern "C"
