// mmw_vehicle_velocity_ransac's host code under AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own: the
// translation unit mmw_tu_vehicle_vel.hip compiled host-only (the kernel becomes a launch stub that is never reached here) and
// linked with this driver.  The entry judges every argument before it touches its context, so a context that is never
// dereferenced stands in for a real one: each class of refused argument must come back as MMW_ERR_INVALID with an error text, an
// LDS demand beyond 160 KiB as MMW_ERR_UNSUPPORTED, and n_frames == 0 as MMW_OK, without a device.  A sweep walks the integer
// arguments over values at and beyond both ends of int.  mmw_last_error and the functions of other units that the unit refers to
// are supplied here; none of them is reached.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../../include/mmwgpu.h"
#include "../../mmwave_radar_processing_amd/csrc/mmw_entry.h"

namespace mmw {
int chain_settle(mmw_ctx *) { return MMW_OK; }      // mmw_tu_chain.hip's; only reached through a context with chain work pending
int env_int(const char *, int dflt) { return dflt; }
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

struct Call {
    mmw_ctx *ctx;
    const double *points;
    const int32_t *counts;
    int F = 0, cap = 16, dim = 2, ppf = 7, iters = 100;
    double fit = 0.05;
    int ncp = 10;
    double stat = 0.2;
    const double *init = nullptr;
    const int32_t *draws;
    int n_tab = 1, chain = 0;
    double *out;
    int32_t *status, *flags;
    int run() const {
        return mmw_vehicle_velocity_ransac(ctx, points, counts, F, cap, dim, ppf, iters, fit, ncp, stat, init, draws, n_tab, chain, out,
                                           status, flags);
    }
};

int main() {
    // never dereferenced: the entry hands its checks to a function that is not given the context, and every call below ends in
    // that function, at the LDS limit or at the n_frames == 0 return behind them
    alignas(64) static unsigned char ctx_bytes[64];
    static double points[16 * 4], init[3], out[5];
    static int32_t counts[1], draws[7 * 100], status[1], flags[1];
    Call good;
    good.ctx = reinterpret_cast<mmw_ctx *>(ctx_bytes);
    good.points = points, good.counts = counts, good.draws = draws, good.out = out, good.status = status, good.flags = flags;
    const int lo = std::numeric_limits<int>::min(), hi = std::numeric_limits<int>::max();

    CHECK(good.run() == MMW_OK);                    // no frames: a successful no-op, with or without the optional table
    for (int chain : {0, 1})
        for (int dim : {2, 3}) {
            Call c = good;
            c.chain = chain, c.dim = dim, c.init = init;
            CHECK(c.run() == MMW_OK);
        }
    // null pointers (d_init may be null)
    for (int which = 0; which < 7; ++which) {
        Call c = good;
        if (which == 0) c.ctx = nullptr;
        if (which == 1) c.points = nullptr;
        if (which == 2) c.counts = nullptr;
        if (which == 3) c.draws = nullptr;
        if (which == 4) c.out = nullptr;
        if (which == 5) c.status = nullptr;
        if (which == 6) c.flags = nullptr;
        CHECK(refused(c.run()));
        c.F = 1;
        CHECK(refused(c.run()));
    }
    // extents
    for (int v : {-1, lo}) {
        Call c = good;
        c.F = v;
        CHECK(refused(c.run()));
        c = good, c.n_tab = v;
        CHECK(refused(c.run()));
    }
    for (int v : {0, -1, lo}) {
        Call c = good;
        c.cap = v;
        CHECK(refused(c.run()));
        c = good, c.iters = v;
        CHECK(refused(c.run()));
    }
    // dim, points_per_fit below dim, num_close_pts below points_per_fit
    for (int v : {1, 4, 0, -2, lo, hi}) {
        Call c = good;
        c.dim = v;
        CHECK(refused(c.run()));
    }
    for (int dim : {2, 3})
        for (int v : {dim - 1, 0, -1, lo}) {
            Call c = good;
            c.dim = dim, c.ppf = v;
            CHECK(refused(c.run()));
        }
    for (int v : {6, 0, -1, lo}) {
        Call c = good;
        c.ncp = v;
        CHECK(refused(c.run()));
    }
    {
        Call c = good;
        c.ppf = hi, c.ncp = hi;                     // equal is allowed, whatever the size
        CHECK(c.run() == MMW_OK);
        c.ppf = 3, c.dim = 3, c.ncp = 3;
        CHECK(c.run() == MMW_OK);
    }
    // thresholds that are no numbers, the chain switch
    for (double v : {std::nan(""), HUGE_VAL, -HUGE_VAL}) {
        Call c = good;
        c.fit = v;
        CHECK(refused(c.run()));
        c = good, c.stat = v;
        CHECK(refused(c.run()));
    }
    for (int v : {2, -1, lo, hi}) {
        Call c = good;
        c.chain = v;
        CHECK(refused(c.run()));
    }
    // n_frames == 0 does not excuse a bad argument; a refused call names what it refused
    {
        Call c = good;
        c.ncp = 5;
        CHECK(c.run() == MMW_ERR_INVALID);
        CHECK(std::strstr(mmw::g_last_error.c_str(), "num_close_pts 5") != nullptr);
        mmw::g_last_error.clear();
    }
    // the LDS demand: 4 cap + 9 max_iters + 192 doubles against 160 KiB, also where the products leave int
    {
        Call c = good;
        c.cap = 4896;                               // (4 * 4896 + 900 + 192) * 8 = 165 408 > 163 840
        CHECK(c.run() == MMW_ERR_UNSUPPORTED);
        c.cap = 4847;                               // 163 840 exactly
        CHECK(c.run() == MMW_OK);
        c.cap = 4848;
        CHECK(c.run() == MMW_ERR_UNSUPPORTED);
        c = good, c.iters = 20449;                  // (64 + 9 * 20449 + 192) * 8 = 1 474 376
        CHECK(c.run() == MMW_ERR_UNSUPPORTED);
        for (int v : {hi, hi - 1, 1 << 30}) {
            c = good, c.cap = v;
            CHECK(c.run() == MMW_ERR_UNSUPPORTED);
            c = good, c.iters = v;
            CHECK(c.run() == MMW_ERR_UNSUPPORTED);
            c.cap = v;
            CHECK(c.run() == MMW_ERR_UNSUPPORTED);
        }
        mmw::g_last_error.clear();
    }
    std::printf("vehicle_vel_sanitize: %d checks, %d failures\n", calls, fails);
    return fails ? 1 : 0;
}
