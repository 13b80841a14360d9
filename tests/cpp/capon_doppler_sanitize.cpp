// mmw_capon_doppler's host code under AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own: the translation unit
// mmw_tu_capon_doppler.hip compiled host-only (kernels become launch stubs that are never reached here) and linked with this driver.
// It runs the host twin mmw_diag_capon_doppler_host on buffers of exactly the sizes the entry documents -- every shape extreme, a
// degenerate row, detections outside the map, counts above cap and below zero -- and every class of refused argument of the device
// entry, which judges its arguments before it touches its context: a context that is never dereferenced stands in for a real one.
// mmw_last_error and the one function of the main unit the context plumbing refers to are supplied here.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/mmwgpu.h"
#include "../../mmwave_radar_processing_amd/csrc/mmw_ctx.h"

namespace mmw {
int chain_settle(mmw_ctx *) { return MMW_OK; }      // mmw_tu_chain.hip's; only reached through a context with chain work pending
}  // namespace mmw

static int fails = 0, calls = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        ++calls;                                                             \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++fails;                                                         \
        }                                                                    \
    } while (0)

static bool refused(int rc) {
    const bool ok = rc == MMW_ERR_INVALID && !mmw::g_last_error.empty();
    mmw::g_last_error.clear();
    return ok;
}

// the host twin on heap buffers of exactly the documented sizes (ASan sees any access past them)
static void run_host(int F, int n, int R, int K, int T, int cap, int window, bool with_spec, bool with_points) {
    std::vector<float> X((size_t)F * n * R * K * 2);
    unsigned s = 12345u + (unsigned)(n * 131 + R * 17 + K);
    for (float &v : X) {
        s = s * 1664525u + 1013904223u;
        v = (float)((int)(s >> 20) % 200 - 100);
    }
    if (F > 1 && R > 1)
        for (int i = 0; i < n; ++i) std::memset(&X[(((size_t)1 * n + i) * R + 1) * K * 2], 0, (size_t)K * 2 * sizeof(float));
    std::vector<int32_t> dets((size_t)F * cap * 2), counts((size_t)F);
    for (int f = 0; f < F; ++f) {
        counts[f] = f == 0 ? cap + 3 : (f == 2 ? -4 : cap - 1);
        for (int j = 0; j < cap; ++j) {
            dets[((size_t)f * cap + j) * 2] = (j * 7 + f) % R;
            dets[((size_t)f * cap + j) * 2 + 1] = (j * 5 + 2 * f) % T;
        }
        if (cap > 3) {
            dets[((size_t)f * cap + 1) * 2] = R;            // outside the map, either index
            dets[((size_t)f * cap + 2) * 2 + 1] = -1;
            dets[((size_t)f * cap + 3) * 2] = INT_MIN;
        }
    }
    std::vector<double> th((size_t)T), range((size_t)R), vel((size_t)K);
    for (int t = 0; t < T; ++t) th[t] = -1.0 + 2.0 * t / (T > 1 ? T - 1 : 1);
    for (int r = 0; r < R; ++r) range[r] = 0.5 * r;
    for (int k = 0; k < K; ++k) vel[k] = k - K / 2;
    std::vector<int32_t> dop((size_t)F * cap, 77);
    std::vector<double> peak((size_t)F * cap, 7.0), spec(with_spec ? (size_t)F * cap * K : 0, 7.0),
        points(with_points ? (size_t)F * cap * 4 : 0, 7.0);
    const int rc = mmw_diag_capon_doppler_host(X.data(), dets.data(), counts.data(), th.data(), dop.data(), peak.data(),
                                               with_spec ? spec.data() : nullptr, with_points ? points.data() : nullptr,
                                               with_points ? range.data() : nullptr, with_points ? vel.data() : nullptr, F, n, R, K, T,
                                               cap, 1e-3, window);
    CHECK(rc == MMW_OK);
    for (int f = 0; f < F; ++f) {
        const int nf = counts[f] < 0 ? 0 : (counts[f] > cap ? cap : counts[f]);
        for (int j = 0; j < cap; ++j) {
            const size_t slot = (size_t)f * cap + j;
            const int q = dets[slot * 2], t = dets[slot * 2 + 1];
            if (j >= nf) {
                CHECK(dop[slot] == 0 && peak[slot] == 0.0);
            } else if (q < 0 || q >= R || t < 0 || t >= T || (f == 1 && q == 1 && R > 1)) {
                CHECK(dop[slot] == -1 && std::isnan(peak[slot]));
            } else {
                CHECK(dop[slot] >= 0 && dop[slot] < K && std::isfinite(peak[slot]));
            }
        }
    }
}

int main() {
    const int shapes[][6] = {{2, 8, 6, 16, 33, 12}, {3, 12, 5, 10, 7, 9},  {3, 1, 3, 7, 4, 6},   {2, 16, 2, 1, 5, 5},
                             {2, 4, 3, 2, 3, 4},    {1, 16, 1, 512, 2, 2}, {3, 3, 9, 33, 1, 40}, {1, 1, 1, 1, 1, 1}};
    for (const auto &sh : shapes)
        for (int window = 0; window < 2; ++window) {
            run_host(sh[0], sh[1], sh[2], sh[3], sh[4], sh[5], window, true, true);
            run_host(sh[0], sh[1], sh[2], sh[3], sh[4], sh[5], window, false, false);
        }

    // the refusals of the device entry: never dereferenced context, outputs untouched
    alignas(64) static unsigned char ctx_bytes[64];
    mmw_ctx *ctx = reinterpret_cast<mmw_ctx *>(ctx_bytes);
    const int n = 2, R = 3, K = 4, T = 2, cap = 2;
    static float X[2 * 3 * 4 * 2];
    static int32_t dets[2 * 2] = {0, 0, 1, 1}, counts[1] = {2}, dop[2] = {5, 5};
    static double th[2] = {0.1, 0.2}, peak[2] = {5, 5}, spec[2 * 4], pts[2 * 4], rng[3], vel[4];
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    auto call = [&](mmw_ctx *c, const void *x, const int32_t *d, const int32_t *cn, const double *t, int32_t *dp, double *pk, double *pt,
                    const double *rg, const double *vl, int F, int nn, int RR, int KK, int TT, int cp, double delta) {
        return mmw_capon_doppler(c, x, d, cn, t, dp, pk, spec, pt, rg, vl, F, nn, RR, KK, TT, cp, delta, 1);
    };
    CHECK(refused(call(nullptr, X, dets, counts, th, dop, peak, pts, rng, vel, 1, n, R, K, T, cap, 1e-3)));
    CHECK(refused(call(ctx, nullptr, dets, counts, th, dop, peak, pts, rng, vel, 1, n, R, K, T, cap, 1e-3)));
    CHECK(refused(call(ctx, X, nullptr, counts, th, dop, peak, pts, rng, vel, 1, n, R, K, T, cap, 1e-3)));
    CHECK(refused(call(ctx, X, dets, nullptr, th, dop, peak, pts, rng, vel, 1, n, R, K, T, cap, 1e-3)));
    CHECK(refused(call(ctx, X, dets, counts, nullptr, dop, peak, pts, rng, vel, 1, n, R, K, T, cap, 1e-3)));
    CHECK(refused(call(ctx, X, dets, counts, th, nullptr, peak, pts, rng, vel, 1, n, R, K, T, cap, 1e-3)));
    CHECK(refused(call(ctx, X, dets, counts, th, dop, nullptr, pts, rng, vel, 1, n, R, K, T, cap, 1e-3)));
    CHECK(refused(call(ctx, X, dets, counts, th, dop, peak, pts, nullptr, vel, 1, n, R, K, T, cap, 1e-3)));
    CHECK(refused(call(ctx, X, dets, counts, th, dop, peak, pts, rng, nullptr, 1, n, R, K, T, cap, 1e-3)));
    for (int bad : {-1, INT_MIN}) CHECK(refused(call(ctx, X, dets, counts, th, dop, peak, pts, rng, vel, bad, n, R, K, T, cap, 1e-3)));
    for (int bad : {0, 17, -1, INT_MAX, INT_MIN}) CHECK(refused(call(ctx, X, dets, counts, th, dop, peak, pts, rng, vel, 1, bad, R, K, T, cap, 1e-3)));
    for (int bad : {0, 513, -1, INT_MAX, INT_MIN}) CHECK(refused(call(ctx, X, dets, counts, th, dop, peak, pts, rng, vel, 1, n, R, bad, T, cap, 1e-3)));
    for (int which = 0; which < 3; ++which)
        for (int bad : {0, -2, INT_MIN})
            CHECK(refused(call(ctx, X, dets, counts, th, dop, peak, pts, rng, vel, 1, n, which == 0 ? bad : R, K, which == 1 ? bad : T,
                               which == 2 ? bad : cap, 1e-3)));
    for (double bad : {-1e-3, nan, inf, -inf}) CHECK(refused(call(ctx, X, dets, counts, th, dop, peak, pts, rng, vel, 1, n, R, K, T, cap, bad)));
    for (double bad : {nan, inf, -inf}) {
        double t2[2] = {0.1, bad};
        CHECK(refused(call(ctx, X, dets, counts, t2, dop, peak, pts, rng, vel, 1, n, R, K, T, cap, 1e-3)));
    }
    // a refused call names what it refused
    CHECK(call(ctx, X, dets, counts, th, dop, peak, pts, rng, vel, 1, 17, R, K, T, cap, 1e-3) == MMW_ERR_INVALID);
    CHECK(std::strstr(mmw::g_last_error.c_str(), "n is 17") != nullptr);
    // more rows or slots than a launch grid: unsupported, nothing launched
    CHECK(call(ctx, X, dets, counts, th, dop, peak, pts, rng, vel, INT_MAX, n, R, K, T, cap, 1e-3) == MMW_ERR_UNSUPPORTED);
    // no frames: a successful no-op (points without tables stays refused)
    CHECK(call(ctx, X, dets, counts, th, dop, peak, pts, rng, vel, 0, n, R, K, T, cap, 1e-3) == MMW_OK);
    CHECK(call(ctx, X, dets, counts, th, dop, peak, nullptr, nullptr, nullptr, 0, 16, 1, 512, T, 1, 0.0) == MMW_OK);
    CHECK(refused(call(ctx, X, dets, counts, th, dop, peak, pts, nullptr, nullptr, 0, n, R, K, T, cap, 1e-3)));
    // the host twin refuses the same classes
    CHECK(refused(mmw_diag_capon_doppler_host(X, dets, counts, th, dop, peak, spec, pts, rng, vel, 1, 0, R, K, T, cap, 1e-3, 1)));
    CHECK(refused(mmw_diag_capon_doppler_host(X, dets, counts, th, dop, peak, spec, pts, nullptr, vel, 1, n, R, K, T, cap, 1e-3, 1)));
    CHECK(refused(mmw_diag_capon_doppler_host(X, dets, counts, th, dop, peak, spec, pts, rng, vel, 1, n, R, K, T, cap, nan, 1)));
    CHECK(dop[0] == 5 && dop[1] == 5 && peak[0] == 5 && peak[1] == 5);          // nothing was written
    for (double v : spec) CHECK(v == 0.0);
    for (double v : pts) CHECK(v == 0.0);
    std::printf("capon_doppler_sanitize: %d checks, %d failures\n", calls, fails);
    return fails ? 1 : 0;
}
