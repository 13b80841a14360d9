// mmw_micro_doppler's host code under AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own: the translation
// unit mmw_tu_micro_doppler.hip compiled host-only (kernels become launch stubs that are never reached here) and linked with this
// driver.  The entry judges every argument before it touches its context, so a context that is never dereferenced stands in for a
// real one: each class of refused argument must come back as MMW_ERR_INVALID with an error text, and n_frames == 0 as MMW_OK,
// without a device.  mmw_last_error and the one function of the main unit the context plumbing refers to are supplied here.
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
    // never dereferenced: the entry hands its checks to a function that is not given the context (md_validate), and every call below
    // ends in that function or at the n_frames == 0 return right behind it
    alignas(64) static unsigned char ctx_bytes[64];
    mmw_ctx *ctx = reinterpret_cast<mmw_ctx *>(ctx_bytes);
    alignas(16) static float cube[2 * 4 * 8 * 2], out[8];
    const int V = 2, S = 4, C = 8;
    // null pointers
    CHECK(refused(mmw_micro_doppler(nullptr, cube, out, 1, V, S, C, 0, 0, 1)));
    CHECK(refused(mmw_micro_doppler(ctx, nullptr, out, 1, V, S, C, 0, 0, 1)));
    CHECK(refused(mmw_micro_doppler(ctx, cube, nullptr, 1, V, S, C, 0, 0, 1)));
    // frame count and shape
    CHECK(refused(mmw_micro_doppler(ctx, cube, out, -1, V, S, C, 0, 0, 1)));
    for (int bad = 0; bad < 3; ++bad)
        CHECK(refused(mmw_micro_doppler(ctx, cube, out, 1, bad == 0 ? 0 : V, bad == 1 ? 0 : S, bad == 2 ? -3 : C, 0, 0, 0)));
    // antenna outside [0, V)
    for (int rx : {-1, V, V + 7, -2147483647 - 1, 2147483647})
        CHECK(refused(mmw_micro_doppler(ctx, cube, out, 1, V, S, C, rx, 0, 1)));
    // empty window, rows outside [0, S)
    CHECK(refused(mmw_micro_doppler(ctx, cube, out, 1, V, S, C, 0, 2, 1)));
    CHECK(refused(mmw_micro_doppler(ctx, cube, out, 1, V, S, C, 0, -1, 1)));
    CHECK(refused(mmw_micro_doppler(ctx, cube, out, 1, V, S, C, 0, 0, S)));
    CHECK(refused(mmw_micro_doppler(ctx, cube, out, 1, V, S, C, 0, S, S)));
    CHECK(refused(mmw_micro_doppler(ctx, cube, out, 1, V, S, C, 0, -2147483647 - 1, 2147483647)));
    CHECK(refused(mmw_micro_doppler(ctx, cube, out, 1, V, S, C, 0, 2147483647, -2147483647 - 1)));
    // a refused call names what it refused
    CHECK(mmw_micro_doppler(ctx, cube, out, 1, V, S, C, 5, 0, 1) == MMW_ERR_INVALID);
    CHECK(std::strstr(mmw::g_last_error.c_str(), "rx_idx 5") != nullptr);
    CHECK(mmw_micro_doppler(ctx, cube, out, 1, V, 0, -3, 0, 0, 0) == MMW_ERR_INVALID);
    CHECK(std::strstr(mmw::g_last_error.c_str(), "S 0, C -3") != nullptr);
    // no frames: a successful no-op, for every window a caller may hold
    for (int hi = 0; hi < S; ++hi) CHECK(mmw_micro_doppler(ctx, cube, out, 0, V, S, C, V - 1, 0, hi) == MMW_OK);
    // n_frames == 0 does not excuse a bad argument
    CHECK(refused(mmw_micro_doppler(ctx, cube, out, 0, V, S, C, V, 0, 1)));
    std::printf("micro_doppler_sanitize: %d checks, %d failures\n", calls, fails);
    return fails ? 1 : 0;
}
