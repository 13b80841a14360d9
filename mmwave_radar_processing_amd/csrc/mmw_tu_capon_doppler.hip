// Translation unit of the MVDR-beamformed Doppler of Capon detections (mmw_capon_doppler.h).  Built with -ffp-contract=off
// (Makefile): the kernel and the host-only entry round every operation alike.
#include <algorithm>
#include <climits>

#include "mmw_ctx.h"
#include "mmw_capon_doppler.h"

using namespace mmw;

namespace {

// Every argument is judged here, before the context is touched: the function is not given the context, so a refused call cannot
// enqueue anything and needs no device (tests/cpp/capon_doppler_sanitize.cpp relies on it).
int cd_validate(bool have_ctx, const void *X, const int32_t *dets, const int32_t *counts, const double *h_thetas, const int32_t *dop,
                const double *peak, const double *points, const double *range, const double *vel, int n_frames, int n, int R, int K,
                int T, int cap, double delta) {
    MMW_REQUIRE(have_ctx && X && dets && counts && h_thetas && dop && peak,
                "null argument (ctx %d, X %d, dets %d, counts %d, h_thetas %d, dop %d, peak %d)", (int)have_ctx, X != nullptr,
                dets != nullptr, counts != nullptr, h_thetas != nullptr, dop != nullptr, peak != nullptr);
    MMW_REQUIRE(!points || (range && vel), "points without the range and velocity tables (range %d, vel %d)", range != nullptr,
                vel != nullptr);
    MMW_REQUIRE(n_frames >= 0, "n_frames is %d", n_frames);
    MMW_REQUIRE(n >= 1 && n <= CD_MAX_N, "n is %d antennas (1 .. %d)", n, CD_MAX_N);
    MMW_REQUIRE(K >= 1 && K <= CD_MAX_K, "K is %d chirps (1 .. %d)", K, CD_MAX_K);
    MMW_REQUIRE(R >= 1 && T >= 1 && cap >= 1, "bad shape: R %d, T %d, cap %d must all be positive", R, T, cap);
    MMW_REQUIRE(delta >= 0.0 && std::isfinite(delta), "diagonal loading %g is not a finite number >= 0", delta);
    for (int t = 0; t < T; ++t) MMW_REQUIRE(std::isfinite(h_thetas[t]), "h_thetas[%d] = %g is not finite", t, h_thetas[t]);
    if ((double)n_frames * R > (double)INT_MAX || (double)n_frames * cap > (double)INT_MAX)
        return set_error(MMW_ERR_UNSUPPORTED, "capon_doppler: %d frames x %d rows / %d slots exceed one launch grid: split the frames",
                         n_frames, R, cap);
    return MMW_OK;
}

// [T][n] steering vectors a_i = exp(-j pi i sin(theta)) (the phase rounded as NumPy rounds -1j * pi * i * sin(theta)), then cos and
// sin of the T angles
std::vector<double> cd_angle_tables(const double *h_thetas, int T, int n) {
    std::vector<double> tab((size_t)T * n * 2 + 2 * (size_t)T);
    for (int t = 0; t < T; ++t) {
        const double s = std::sin(h_thetas[t]);
        for (int i = 0; i < n; ++i) {
            const double ph = (-M_PI * (double)i) * s;
            tab[2 * ((size_t)t * n + i)] = std::cos(ph);
            tab[2 * ((size_t)t * n + i) + 1] = std::sin(ph);
        }
        tab[(size_t)T * n * 2 + t] = std::cos(h_thetas[t]);
        tab[(size_t)T * n * 2 + T + t] = s;
    }
    return tab;
}

void cd_set_angle_tables(CdArgs &a, const double *tab, int T, int n) {
    a.steer = reinterpret_cast<const CdC *>(tab);
    a.cos_t = tab + (size_t)T * n * 2;
    a.sin_t = a.cos_t + T;
}

}  // namespace

extern "C" {

int mmw_capon_doppler(mmw_ctx *ctx, const void *d_X, const int32_t *d_dets, const int32_t *d_counts, const double *h_thetas,
                      int32_t *d_dop, double *d_peak, double *d_spec, double *d_points, const double *d_range, const double *d_vel,
                      int n_frames, int n, int R, int K, int T, int cap, double delta, int doppler_window) {
    MMW_TRY(cd_validate(ctx != nullptr, d_X, d_dets, d_counts, h_thetas, d_dop, d_peak, d_points, d_range, d_vel, n_frames, n, R, K, T,
                        cap, delta));
    if (n_frames == 0) return MMW_OK;
    MMW_JOIN(ctx);
    // the angle tables stay on the device while the caller keeps its grid and antenna count (as mmw_capon's)
    std::vector<double> key(h_thetas, h_thetas + T);
    key.push_back((double)n);
    if (ctx->capon_dop_key != key) {
        const std::vector<double> tab = cd_angle_tables(h_thetas, T, n);
        MMW_HIP(hipStreamSynchronize(ctx->stream));                     // a launch in flight may still read the old tables
        if (ctx->capon_dop_tab) (void)hipFree(ctx->capon_dop_tab);
        ctx->capon_dop_tab = nullptr;
        ctx->capon_dop_key.clear();
        MMW_HIP(hipMalloc(&ctx->capon_dop_tab, tab.size() * sizeof(double)));
        MMW_HIP(hipMemcpy(ctx->capon_dop_tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
        ctx->capon_dop_key = key;
    }
    CdArgs a{};
    a.X = (const float2 *)d_X;
    a.dets = d_dets, a.counts = d_counts;
    cd_set_angle_tables(a, (const double *)ctx->capon_dop_tab, T, n);
    MMW_TRY(get_table<double>(ctx, TAB_TWIDDLE, K, (const void **)&a.tw));
    if (doppler_window) MMW_TRY(get_table<double>(ctx, TAB_HANN, K, (const void **)&a.hann));
    a.range = d_range, a.vel = d_vel;
    a.dop = d_dop, a.peak = d_peak, a.spec = d_spec, a.points = d_points;
    a.n = n, a.R = R, a.K = K, a.T = T, a.cap = cap, a.ch = cd_chunk(K);
    a.delta = delta;
    const size_t lds = cd_lds(n, K, a.ch).total;
    if (lds > 64 * 1024)
        MMW_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_capon_doppler), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds));         // per device, so on every call
    ProfScope ps(ctx, "capon_doppler");
    const long n_slots = (long)n_frames * cap;
    if (d_spec) MMW_HIP(hipMemsetAsync(d_spec, 0, (size_t)n_slots * K * sizeof(double), ctx->stream));
    hipLaunchKernelGGL(k_cd_fill, dim3((unsigned)((n_slots + 255) / 256)), dim3(256), 0, ctx->stream, a, n_slots);
    MMW_TRY(check_launch("capon_doppler_fill"));
    hipLaunchKernelGGL(k_capon_doppler, dim3((unsigned)((long)n_frames * R)), dim3(CD_THREADS), lds, ctx->stream, a);
    return check_launch("capon_doppler");
}

int mmw_diag_capon_doppler_host(const void *h_X, const int32_t *h_dets, const int32_t *h_counts, const double *h_thetas, int32_t *h_dop,
                                double *h_peak, double *h_spec, double *h_points, const double *h_range, const double *h_vel,
                                int n_frames, int n, int R, int K, int T, int cap, double delta, int doppler_window) {
    MMW_TRY(cd_validate(true, h_X, h_dets, h_counts, h_thetas, h_dop, h_peak, h_points, h_range, h_vel, n_frames, n, R, K, T, cap,
                        delta));
    if (n_frames == 0) return MMW_OK;
    const std::vector<double> tab = cd_angle_tables(h_thetas, T, n);
    const std::vector<double> tw = make_table<double>(TAB_TWIDDLE, K), hann = make_table<double>(TAB_HANN, K);
    CdArgs a{};
    a.X = (const float2 *)h_X;
    cd_set_angle_tables(a, tab.data(), T, n);
    a.tw = reinterpret_cast<const CdC *>(tw.data());
    a.hann = doppler_window ? hann.data() : nullptr;
    a.range = h_range, a.vel = h_vel;
    a.n = n, a.R = R, a.K = K, a.T = T, a.cap = cap;
    std::vector<CdC> A((size_t)CD_MAX_N * CD_MP), L((size_t)CD_MAX_N * CD_MP), u(CD_MP), y((size_t)K);
    std::vector<double> mag((size_t)K);
    for (long f = 0; f < n_frames; ++f) {
        const int nf = cd_clamp_count(h_counts[f], cap);
        int factored = -1;              // the row whose inverse A holds
        bool degenerate = false;        // ... and whether its covariance is not positive definite
        for (int j = 0; j < cap; ++j) {
            const long slot = f * cap + j;
            double *spec = h_spec ? h_spec + slot * K : nullptr, *pt = h_points ? h_points + slot * 4 : nullptr;
            const int q = j < nf ? h_dets[2 * slot] : 0, t = j < nf ? h_dets[2 * slot + 1] : 0;
            const bool past = j >= nf, inside = !past && (unsigned)q < (unsigned)R && (unsigned)t < (unsigned)T;
            if (!inside) {
                const double v = past ? 0.0 : cd_nan();
                h_dop[slot] = past ? 0 : -1;
                h_peak[slot] = v;
                if (pt) pt[0] = v, pt[1] = v, pt[2] = 0.0, pt[3] = v;
                for (int m = 0; spec && m < K; ++m) spec[m] = v;
                continue;
            }
            const CdSnap X{a.X + (f * n * (long)R + q) * (long)K, (long)R * K};
            if (factored != q) {
                for (int i = 0; i < n; ++i)
                    for (int c = 0; c <= i; ++c) A[i * CD_MP + c] = cd_cov_entry(X, i, c, K);
                cd_load_diagonal(A.data(), n, delta);
                bool bad = false;
                for (int c = 0; c < n; ++c)
                    for (int i = c; i < n; ++i) {
                        double pivot;
                        L[i * CD_MP + c] = cd_chol_entry(A.data(), L.data(), i, c, &pivot);
                        bad |= i == c && !cd_pivot_ok(pivot);
                    }
                for (int c = 0; c < n; ++c) cd_inverse_column(L.data(), A.data(), n, c);
                degenerate = bad;
                factored = q;
            }
            int dop = -1;
            double best = -1.0;
            if (!degenerate) {
                const CdC *st = a.steer + (size_t)t * n;
                for (int i = 0; i < n; ++i) u[i] = cd_solve_entry(A.data(), st, n, i);
                const double den = cd_denominator(st, u.data(), n);
                for (int i = 0; i < n; ++i) u[i] = CdC{u[i].re / den, u[i].im / den};
                for (int k = 0; k < K; ++k) y[k] = cd_beamform(X, u.data(), n, k, a.hann);
                int bi = INT_MAX;
                for (int m = 0; m < K; ++m) {
                    mag[m] = cd_spectrum(y.data(), a.tw, K, m);
                    if (cd_better(mag[m], m, best, bi)) best = mag[m], bi = m;
                }
                dop = bi == INT_MAX ? -1 : bi;
            }
            h_dop[slot] = dop;
            h_peak[slot] = dop < 0 ? cd_nan() : best;
            if (pt) cd_point(a, slot, q, t, dop, pt);
            for (int m = 0; spec && m < K; ++m) spec[m] = degenerate ? cd_nan() : mag[m];
        }
    }
    return MMW_OK;
}

}  // extern "C"
