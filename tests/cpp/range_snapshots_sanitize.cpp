// mmw_range_snapshots' host code under AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own: the translation
// unit mmw_tu_range_snapshots.hip compiled host-only (kernels become launch stubs that are never reached here) and linked with this
// driver.  The entry judges every argument before it touches its context, so a context that is never dereferenced stands in for a
// real one: each class of refused argument must come back as MMW_ERR_INVALID with an error text, S = 1025 as MMW_ERR_UNSUPPORTED
// and n_frames == 0 as MMW_OK, without a device.  mmw_last_error and the one function of the main unit the context plumbing
// refers to are supplied here.
#include <climits>
#include <cstdio>
#include <cstring>

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

int main() {
    // never dereferenced: the entry hands its checks to a function that is not given the context (rs_validate), and every call
    // below ends in that function or at the n_frames == 0 return right behind it
    alignas(64) static unsigned char ctx_bytes[64];
    mmw_ctx *ctx = reinterpret_cast<mmw_ctx *>(ctx_bytes);
    alignas(16) static float cube[2 * 4 * 8 * 2], out[2 * 4 * 8 * 2];
    const int V = 2, S = 4, C = 8;
    const int rx[3] = {1, 0, 1};            // a duplicate is allowed
    // null pointers
    CHECK(refused(mmw_range_snapshots(nullptr, cube, out, 1, V, S, C, rx, 3, 0, S, 1)));
    CHECK(refused(mmw_range_snapshots(ctx, nullptr, out, 1, V, S, C, rx, 3, 0, S, 1)));
    CHECK(refused(mmw_range_snapshots(ctx, cube, nullptr, 1, V, S, C, rx, 3, 0, S, 1)));
    CHECK(refused(mmw_range_snapshots(ctx, cube, out, 1, V, S, C, nullptr, 3, 0, S, 1)));
    CHECK(refused(mmw_range_snapshots(ctx, cube, out, 1, V, S, C, nullptr, INT_MAX, 0, S, 1)));
    // frame count, shape, list length
    for (int bad : {-1, INT_MIN}) CHECK(refused(mmw_range_snapshots(ctx, cube, out, bad, V, S, C, rx, 3, 0, S, 1)));
    for (int which = 0; which < 3; ++which)
        for (int bad : {0, -3, INT_MIN})
            CHECK(refused(mmw_range_snapshots(ctx, cube, out, 1, which == 0 ? bad : V, which == 1 ? bad : S, which == 2 ? bad : C, nullptr,
                                              0, 0, 1, 0)));
    for (int bad : {-1, INT_MIN}) CHECK(refused(mmw_range_snapshots(ctx, cube, out, 1, V, S, C, rx, bad, 0, S, 1)));
    // a listed antenna outside [0, V)
    for (int bad : {-1, V, V + 7, INT_MIN, INT_MAX}) {
        const int lst[3] = {0, bad, 1};
        CHECK(refused(mmw_range_snapshots(ctx, cube, out, 1, V, S, C, lst, 3, 0, S, 1)));
        CHECK(refused(mmw_range_snapshots(ctx, cube, out, 1, V, S, C, lst + 1, 1, 0, S, 1)));
    }
    // windows that are not 0 <= r_lo < r_hi <= S
    const int windows[][2] = {{2, 2}, {3, 2}, {-1, 2}, {0, S + 1}, {S, S + 1}, {S, S}, {INT_MIN, INT_MAX}, {INT_MAX, INT_MIN},
                              {0, INT_MAX}, {INT_MIN, 1}, {INT_MAX, INT_MAX}};
    for (const auto &w : windows) CHECK(refused(mmw_range_snapshots(ctx, cube, out, 1, V, S, C, rx, 3, w[0], w[1], 1)));
    // a refused call names what it refused
    const int lst5[2] = {0, 5};
    CHECK(mmw_range_snapshots(ctx, cube, out, 1, V, S, C, lst5, 2, 0, S, 1) == MMW_ERR_INVALID);
    CHECK(std::strstr(mmw::g_last_error.c_str(), "h_rx[1] = 5") != nullptr);
    CHECK(mmw_range_snapshots(ctx, cube, out, 1, V, 0, -3, rx, 3, 0, 1, 1) == MMW_ERR_INVALID);
    CHECK(std::strstr(mmw::g_last_error.c_str(), "S 0, C -3") != nullptr);
    CHECK(mmw_range_snapshots(ctx, cube, out, 1, V, S, C, rx, 3, 3, 2, 1) == MMW_ERR_INVALID);
    CHECK(std::strstr(mmw::g_last_error.c_str(), "[3, 2)") != nullptr);
    // more samples than a strip's LDS image holds: unsupported, nothing launched (with and without frames, any good window)
    mmw::g_last_error.clear();
    CHECK(mmw_range_snapshots(ctx, cube, out, 1, V, 1025, C, rx, 3, 0, 1025, 1) == MMW_ERR_UNSUPPORTED);
    CHECK(std::strstr(mmw::g_last_error.c_str(), "1025") != nullptr);
    CHECK(mmw_range_snapshots(ctx, cube, out, 1, V, INT_MAX, C, nullptr, 0, INT_MAX - 1, INT_MAX, 0) == MMW_ERR_UNSUPPORTED);
    CHECK(mmw_range_snapshots(ctx, cube, out, 0, V, 1025, C, rx, 3, 5, 6, 1) == MMW_ERR_UNSUPPORTED);
    // ... but a bad argument is named first
    CHECK(refused(mmw_range_snapshots(ctx, cube, out, 1, V, 1025, C, rx, 3, 0, 1026, 1)));
    // no frames: a successful no-op, for every window and list a caller may hold, the largest shapes included
    for (int lo = 0; lo < S; ++lo)
        for (int hi = lo + 1; hi <= S; ++hi) {
            CHECK(mmw_range_snapshots(ctx, cube, out, 0, V, S, C, rx, 3, lo, hi, 1) == MMW_OK);
            CHECK(mmw_range_snapshots(ctx, cube, out, 0, V, S, C, nullptr, 0, lo, hi, 0) == MMW_OK);
        }
    CHECK(mmw_range_snapshots(ctx, cube, out, 0, INT_MAX, 1024, INT_MAX, nullptr, 0, 0, 1024, 1) == MMW_OK);
    // n_frames == 0 does not excuse a bad argument
    CHECK(refused(mmw_range_snapshots(ctx, cube, out, 0, V, S, C, lst5, 2, 0, S, 1)));
    CHECK(refused(mmw_range_snapshots(ctx, cube, out, 0, V, S, C, rx, 3, 0, S + 1, 1)));
    for (float v : out) CHECK(v == 0.f);            // nothing was written
    std::printf("range_snapshots_sanitize: %d checks, %d failures\n", calls, fails);
    return fails ? 1 : 0;
}
