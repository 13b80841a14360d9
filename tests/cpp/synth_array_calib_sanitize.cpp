// The host code of mmw_synth_array_calibrate / mmw_diag_synth_array_calib_host under AddressSanitizer + UndefinedBehaviorSanitizer,
// as a program of its own: mmw_tu_synth_calib.hip compiled host-only (the kernels become launch stubs that are never reached) and
// linked with this driver.  The device entry judges every argument before it touches its context, so a context that is never
// dereferenced stands in for a real one: each refused argument must come back as MMW_ERR_INVALID (S > 3584: MMW_ERR_UNSUPPORTED)
// with the sentinel-filled outputs untouched, n_out == 0 as MMW_OK.  The host arrays are exactly as long as the entry is told.
// Then the host twin runs the decision and solve code over a sweep of shapes on scenes with three reflectors, and on degenerate
// inputs.  The functions of other units that the plumbing refers to are supplied here.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/mmwgpu.h"
#include "../../mmwave_radar_processing_amd/csrc/mmw_ctx.h"

namespace mmw {
int chain_settle(mmw_ctx *) { return MMW_OK; }      // mmw_tu_chain.hip's; only reached through a context with chain work pending
int synth_array_contract(mmw_ctx *, const char *, const void *, int, int, int, int, int, int, const int *, int, const double *, const double *,
                         int, double, void *, size_t) {
    std::fprintf(stderr, "FAILED: the contraction was reached\n");
    return MMW_ERR_HIP;
}
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

static bool refused(int rc, int code = MMW_ERR_INVALID) {
    const bool ok = rc == code && !mmw::g_last_error.empty();
    if (!ok) std::fprintf(stderr, "  rc %d, text '%s'\n", rc, mmw::g_last_error.c_str());
    mmw::g_last_error.clear();
    return ok;
}

struct Args {
    mmw_ctx *ctx;
    int n_res = 6, V = 3, S = 16, C = 8, v = 1, k = 2, H = 2, n_out = 2, n_az = 5, n_el = 2, n_iters = 1;
    double lambda_m = 0.005;
    std::vector<int32_t> frames{2, 5};
    std::vector<double> P = std::vector<double>((size_t)2 * 3 * 8, 0.0), dirs = std::vector<double>((size_t)3 * 10, 0.5);
    char cubes[16], out[16], Pcal[16], status[16], targets[16];        // stand-ins for device memory: never dereferenced
    bool no_cubes = false, no_frames = false, no_P = false, no_dirs = false, no_out = false, no_Pcal = false, no_status = false,
         no_targets = false;
    Args(mmw_ctx *c) : ctx(c) { std::memset(out, 0x5a, 16), std::memset(Pcal, 0x5a, 16), std::memset(status, 0x5a, 16), std::memset(targets, 0x5a, 16); }
};

static int run(Args &a) {
    return mmw_synth_array_calibrate(a.ctx, a.no_cubes ? nullptr : a.cubes, a.n_res, a.V, a.S, a.C, a.v, a.k, a.H,
                                     a.no_frames ? nullptr : a.frames.data(), a.n_out, a.no_P ? nullptr : a.P.data(),
                                     a.no_dirs ? nullptr : a.dirs.data(), a.n_az, a.n_el, a.lambda_m, a.n_iters, a.no_out ? nullptr : a.out,
                                     a.no_Pcal ? nullptr : (double *)a.Pcal, a.no_status ? nullptr : (int32_t *)a.status,
                                     a.no_targets ? nullptr : (int32_t *)a.targets);
}

static bool untouched(const Args &a) {
    for (int i = 0; i < 16; ++i)
        if (a.out[i] != 0x5a || a.Pcal[i] != 0x5a || a.status[i] != 0x5a || a.targets[i] != 0x5a) return false;
    return true;
}

template <class F> static void expect_refused(mmw_ctx *ctx, F change, int code = MMW_ERR_INVALID) {
    Args a(ctx);
    change(a);
    CHECK(refused(run(a), code));
    CHECK(untouched(a));
}

static void twin_sweep() {
    const double lam = 0.005;
    for (int S : {8, 16, 63, 64})
        for (int E : {1, 2, 17, 102})
            for (int n_az : {2, 3, 13}) {
                const int n_el = 2, T = n_az * n_el;
                std::vector<double> dirs((size_t)3 * T), P((size_t)3 * E), avg((size_t)S), mag((size_t)S * n_az), l1((size_t)E, 100.0 * S);
                std::vector<std::complex<double>> Fq((size_t)S * E);
                for (int a = 0; a < n_az; ++a)
                    for (int el = 0; el < n_el; ++el) {
                        const double th = 0.1 + 0.08 * a, ph = 0.1 * el;
                        dirs[(size_t)a * n_el + el] = std::cos(th) * std::cos(ph);
                        dirs[(size_t)T + a * n_el + el] = std::sin(th) * std::cos(ph);
                        dirs[(size_t)2 * T + a * n_el + el] = std::sin(ph);
                    }
                for (int e = 0; e < E; ++e) P[e] = -1e-3 * (E - 1 - e), P[(size_t)E + e] = 1e-5 * e, P[(size_t)2 * E + e] = 0.0;
                const int rows[3] = {1, S / 2, S - 2};
                for (int r = 0; r < S; ++r) {
                    avg[r] = 5.0 + 0.01 * ((r * 7) % 5);
                    for (int a = 0; a < n_az; ++a) mag[(size_t)r * n_az + a] = 3.0 + 0.1 * ((a * 5 + r) % 3);
                    for (int e = 0; e < E; ++e) Fq[(size_t)r * E + e] = std::polar(1.0 + 0.1 * ((r + e) % 3), 0.07 * e * ((r % 3) + 1));
                }
                for (int t = 0; t < 3; ++t) {
                    avg[rows[t]] = 60.0 - 7.0 * t;
                    if (n_az >= 3) mag[(size_t)rows[t] * n_az + 1 + (t % (n_az - 2))] = 50.0 + t;
                }
                std::vector<double> Pcal((size_t)3 * E, -1.0);
                int32_t tg[6], info[4];
                for (int with_bounds = 0; with_bounds < 2; ++with_bounds) {
                    std::vector<double> err((size_t)S, 1e-9);
                    CHECK(mmw_diag_synth_array_calib_host(avg.data(), with_bounds ? err.data() : nullptr, S, mag.data(), with_bounds ? 1e-6 : 0.0,
                                                          n_az, n_el, (const double *)Fq.data(), with_bounds ? l1.data() : nullptr, E, P.data(),
                                                          dirs.data(), lam, Pcal.data(), tg, info) == MMW_OK);
                    CHECK(info[0] == (n_az >= 3 ? (info[3] ? -1 : 1) : 0));
                    for (int e = 0; e < E; ++e) CHECK(Pcal[(size_t)2 * E + e] == 0.0 && std::isfinite(Pcal[e]) && std::isfinite(Pcal[(size_t)E + e]));
                    CHECK(Pcal[0] == P[0]);
                }
            }
    // degenerate inputs: S = 1, all-equal avg, NaN, zero magnitudes
    double avg1[3] = {1.0, 1.0, 1.0}, mag1[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, P1[6] = {0, 0, 0, 0, 0, 0}, d1[9] = {1, 1, 1, 0, 0, 0, 0, 0, 0}, Pc[6];
    std::complex<double> F1[6];
    int32_t tg[6], info[4];
    CHECK(mmw_diag_synth_array_calib_host(avg1, nullptr, 3, mag1, 0.0, 3, 1, (const double *)F1, nullptr, 2, P1, d1, 0.005, Pc, tg, info) == MMW_OK && info[0] == 0);
    avg1[1] = NAN;
    CHECK(mmw_diag_synth_array_calib_host(avg1, nullptr, 3, mag1, 0.0, 3, 1, (const double *)F1, nullptr, 2, P1, d1, 0.005, Pc, tg, info) == MMW_OK && info[0] == 0);
    CHECK(mmw_diag_synth_array_calib_host(avg1, nullptr, 1, mag1, 0.0, 3, 1, (const double *)F1, nullptr, 1, P1, d1, 0.005, Pc, tg, info) == MMW_OK && info[0] == 0);
    CHECK(refused(mmw_diag_synth_array_calib_host(nullptr, nullptr, 3, mag1, 0.0, 3, 1, (const double *)F1, nullptr, 2, P1, d1, 0.005, Pc, tg, info)));
    CHECK(refused(mmw_diag_synth_array_calib_host(avg1, nullptr, 0, mag1, 0.0, 3, 1, (const double *)F1, nullptr, 2, P1, d1, 0.005, Pc, tg, info)));
    CHECK(refused(mmw_diag_synth_array_calib_host(avg1, nullptr, 3, mag1, -1.0, 3, 1, (const double *)F1, nullptr, 2, P1, d1, 0.005, Pc, tg, info)));
    CHECK(refused(mmw_diag_synth_array_calib_host(avg1, nullptr, 3, mag1, 0.0, 3, 1, (const double *)F1, nullptr, 2, P1, d1, 0.0, Pc, tg, info)));
}

int main() {
    alignas(64) static char fake[sizeof(mmw_ctx)];       // never dereferenced: every call below is refused or empty
    mmw_ctx *ctx = reinterpret_cast<mmw_ctx *>(fake);
    expect_refused(nullptr, [](Args &) {});
    expect_refused(ctx, [](Args &a) { a.no_cubes = true; });
    expect_refused(ctx, [](Args &a) { a.no_frames = true; });
    expect_refused(ctx, [](Args &a) { a.no_P = true; });
    expect_refused(ctx, [](Args &a) { a.no_dirs = true; });
    expect_refused(ctx, [](Args &a) { a.no_out = true; });
    expect_refused(ctx, [](Args &a) { a.no_Pcal = true; });
    expect_refused(ctx, [](Args &a) { a.no_status = true; });
    expect_refused(ctx, [](Args &a) { a.no_targets = true; });
    expect_refused(ctx, [](Args &a) { a.v = 3; });
    expect_refused(ctx, [](Args &a) { a.v = -1; });
    expect_refused(ctx, [](Args &a) { a.k = 0; });
    expect_refused(ctx, [](Args &a) { a.H = 0; });
    expect_refused(ctx, [](Args &a) { a.S = 0; });
    expect_refused(ctx, [](Args &a) { a.lambda_m = 0.0; });
    expect_refused(ctx, [](Args &a) { a.lambda_m = NAN; });
    expect_refused(ctx, [](Args &a) { a.n_out = -1; });
    expect_refused(ctx, [](Args &a) { a.frames = {5, 2}; });
    expect_refused(ctx, [](Args &a) { a.frames = {2, 2}; });
    expect_refused(ctx, [](Args &a) { a.frames = {2, 6}; });
    expect_refused(ctx, [](Args &a) { a.frames = {-1, 2}; });
    expect_refused(ctx, [](Args &a) { a.n_iters = 0; });
    expect_refused(ctx, [](Args &a) { a.n_iters = 9; });
    expect_refused(ctx, [](Args &a) { a.n_az = 0; });
    expect_refused(ctx, [](Args &a) { a.n_el = 0; });
    expect_refused(ctx, [](Args &a) { a.n_az = 1 << 16, a.n_el = 1 << 16; });
    expect_refused(ctx, [](Args &a) { a.S = 3585; }, MMW_ERR_UNSUPPORTED);
    {
        Args a(ctx);
        a.n_out = 0;
        a.frames.clear(), a.P.clear();
        CHECK(run(a) == MMW_OK && untouched(a));
    }
    {
        Args a(ctx);        // the largest S is judged like any other: refused here only for what else is wrong with the call
        a.S = 3584, a.v = 3;
        CHECK(refused(run(a)) && untouched(a));
    }
    twin_sweep();
    std::printf("synth_array_calib_sanitize: %d checks, %d failures\n", calls, fails);
    return fails ? 1 : 0;
}
