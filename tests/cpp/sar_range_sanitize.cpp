// mmw_sar_slices' and mmw_range_detect's host code under AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own:
// the translation units mmw_tu_sar.hip and mmw_tu_cfar.hip compiled host-only (kernels become launch stubs that are never reached
// here) and linked with this driver.  Both entries judge every argument before they touch their context, so a context that is
// never dereferenced stands in for a real one: each class of refused argument must come back as MMW_ERR_INVALID with an error
// text, and n_frames == 0 as MMW_OK, without a device.  A sweep walks the window and offset validation of mmw_sar_slices over
// every window of a small plane and over offsets that are wrong by one, negative or at the ends of int64.  mmw_last_error and the
// functions of other units that the two units refer to are supplied here; none of them is reached.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/mmwgpu.h"
#include "../../mmwave_radar_processing_amd/csrc/mmw_entry.h"

namespace mmw {
static int unreachable(const char *what) {
    std::fprintf(stderr, "FAILED: %s was reached\n", what);
    return MMW_ERR_INVALID;
}
int chain_settle(mmw_ctx *) { return MMW_OK; }      // mmw_tu_chain.hip's; only reached through a context with chain work pending
int env_int(const char *, int dflt) { return dflt; }
int range_doppler_impl(mmw_ctx *, const void *, void *, void *, int, int, int, int, RawView, float *) { return unreachable("range_doppler_impl"); }
int range_doppler_mag64_impl(mmw_ctx *, const void *, double *, int, int, int, int, int) { return unreachable("range_doppler_mag64_impl"); }
template <> int range_profile_impl<double>(mmw_ctx *, const void *, double *, int, int, int, int, int) { return unreachable("range_profile_impl"); }
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

static void sar_checks(mmw_ctx *ctx) {
    alignas(16) static float cube[2 * 4 * 8 * 2], out[4 * 8 * 2];
    const int V = 2, S = 4, C = 8;
    const int32_t win[4] = {1, 3, 2, 7};
    const int64_t off[2] = {0, 10};
    // the good call's tables are accepted as far as the checks go: with no frames it is a successful no-op
    CHECK(mmw_sar_slices(ctx, cube, 0, V, S, C, 0, win, off, out) == MMW_OK);
    // null pointers
    CHECK(refused(mmw_sar_slices(nullptr, cube, 1, V, S, C, 0, win, off, out)));
    CHECK(refused(mmw_sar_slices(ctx, nullptr, 1, V, S, C, 0, win, off, out)));
    CHECK(refused(mmw_sar_slices(ctx, cube, 1, V, S, C, 0, nullptr, off, out)));
    CHECK(refused(mmw_sar_slices(ctx, cube, 1, V, S, C, 0, win, nullptr, out)));
    CHECK(refused(mmw_sar_slices(ctx, cube, 1, V, S, C, 0, win, off, nullptr)));
    // frame count and shape
    CHECK(refused(mmw_sar_slices(ctx, cube, -1, V, S, C, 0, win, off, out)));
    for (int bad = 0; bad < 3; ++bad)
        CHECK(refused(mmw_sar_slices(ctx, cube, 1, bad == 0 ? 0 : V, bad == 1 ? 0 : S, bad == 2 ? -3 : C, 0, win, off, out)));
    // antenna outside [0, V)
    for (int rx : {-1, V, V + 7, -2147483647 - 1, 2147483647}) CHECK(refused(mmw_sar_slices(ctx, cube, 1, V, S, C, rx, win, off, out)));
    // the first block does not start at 0 (also with no frames: n_frames == 0 does not excuse a bad argument)
    const int64_t off1[2] = {1, 11};
    CHECK(refused(mmw_sar_slices(ctx, cube, 1, V, S, C, 0, win, off1, out)));
    CHECK(refused(mmw_sar_slices(ctx, cube, 0, V, S, C, 0, win, off1, out)));
    CHECK(refused(mmw_sar_slices(ctx, cube, 0, V, S, C, V, win, off, out)));
    // a refused call names what it refused
    CHECK(mmw_sar_slices(ctx, cube, 1, V, S, C, 5, win, off, out) == MMW_ERR_INVALID);
    CHECK(std::strstr(mmw::g_last_error.c_str(), "rx_idx 5") != nullptr);
    // sweep: every (lo, hi) pair a little beyond the plane on both axes; one frame whose offsets match the area exactly.  A window
    // inside [0, S] x [0, C] that is not reversed is the only kind that passes the window check -- and it then dies on the second
    // frame, whose window is always bad, so that nothing is ever launched
    const int lim[] = {-2147483647 - 1, -1, 0, 1, 3, 4, 5, 8, 9, 2147483647};
    int passed_first = 0;
    for (int r0 : lim)
        for (int r1 : lim)
            for (int c0 : lim)
                for (int c1 : lim) {
                    const bool good = r0 >= 0 && r0 <= r1 && r1 <= S && c0 >= 0 && c0 <= c1 && c1 <= C;
                    const int64_t area = good ? (int64_t)(r1 - r0) * (c1 - c0) : 0;
                    const int32_t w2[8] = {r0, r1, c0, c1, 0, S + 1, 0, 0};
                    const int64_t o2[3] = {0, area, area};
                    CHECK(mmw_sar_slices(ctx, cube, 2, V, S, C, 0, w2, o2, out) == MMW_ERR_INVALID);
                    const bool first_ok = std::strstr(mmw::g_last_error.c_str(), "frame 1:") != nullptr;
                    CHECK(first_ok == good);
                    passed_first += first_ok;
                    mmw::g_last_error.clear();
                }
    CHECK(passed_first > 0);
    // offsets: wrong by one either way, negative, overflowing
    for (int64_t bad : {(int64_t)9, (int64_t)11, (int64_t)0, (int64_t)-10, INT64_MAX, INT64_MIN}) {
        const int64_t o[2] = {0, bad};
        CHECK(refused(mmw_sar_slices(ctx, cube, 1, V, S, C, 0, win, o, out)));
    }
    // a later frame that steps wrongly, or from a hostile offset
    std::vector<int32_t> wins;
    std::vector<int64_t> offs{0};
    for (int f = 0; f < 5; ++f) {
        wins.insert(wins.end(), {0, f % 3, 1, 1 + f});
        offs.push_back(offs.back() + (int64_t)(f % 3) * f);
    }
    for (int f = 1; f <= 5; ++f)
        for (int64_t delta : {(int64_t)-1, (int64_t)1, INT64_MAX - offs[f] - 0, INT64_MIN + 1}) {
            std::vector<int64_t> o = offs;
            o[f] += delta;
            CHECK(refused(mmw_sar_slices(ctx, cube, 5, V, S, C, 1, wins.data(), o.data(), out)));
        }
    wins[4 * 4 + 1] = S + 1;            // the good tables, spoilt in their last frame
    CHECK(refused(mmw_sar_slices(ctx, cube, 5, V, S, C, 1, wins.data(), offs.data(), out)));
}

static void range_checks(mmw_ctx *ctx) {
    alignas(16) static float cube[2 * 16 * 3 * 2];
    static double prof[16], thr[16];
    static int32_t dets[16], counts[1];
    const int V = 2, S = 16, C = 3;
    auto call = [&](mmw_ctx *c, const void *cb, int F, int v, int s, int ch, int chirp, int kind, int T, int G, int k, int32_t *d, int32_t *n,
                    int cap) { return mmw_range_detect(c, cb, F, v, s, ch, chirp, kind, T, G, 2.0, k, prof, thr, d, n, cap); };
    CHECK(call(ctx, cube, 0, V, S, C, 0, MMW_CFAR_OS, 3, 1, 4, dets, counts, S) == MMW_OK);
    CHECK(mmw_range_detect(ctx, cube, 0, V, S, C, -C, MMW_CFAR_CA, 3, 1, 2.0, 0, nullptr, nullptr, dets, counts, 0) == MMW_OK);
    // null pointers (d_profile and d_thr may be null)
    CHECK(refused(call(nullptr, cube, 1, V, S, C, 0, MMW_CFAR_OS, 3, 1, 4, dets, counts, S)));
    CHECK(refused(call(ctx, nullptr, 1, V, S, C, 0, MMW_CFAR_OS, 3, 1, 4, dets, counts, S)));
    CHECK(refused(call(ctx, cube, 1, V, S, C, 0, MMW_CFAR_OS, 3, 1, 4, nullptr, counts, S)));
    CHECK(refused(call(ctx, cube, 1, V, S, C, 0, MMW_CFAR_OS, 3, 1, 4, dets, nullptr, S)));
    // frame count, shape, chirp, capacity
    for (int F : {-1, 65536, -2147483647 - 1, 2147483647}) CHECK(refused(call(ctx, cube, F, V, S, C, 0, MMW_CFAR_OS, 3, 1, 4, dets, counts, S)));
    for (int bad = 0; bad < 3; ++bad)
        CHECK(refused(call(ctx, cube, 1, bad == 0 ? 0 : V, bad == 1 ? -1 : S, bad == 2 ? 0 : C, 0, MMW_CFAR_OS, 3, 1, 4, dets, counts, S)));
    for (int chirp : {C, -C - 1, 2147483647, -2147483647 - 1}) CHECK(refused(call(ctx, cube, 1, V, S, C, chirp, MMW_CFAR_OS, 3, 1, 4, dets, counts, S)));
    CHECK(refused(call(ctx, cube, 1, V, S, C, 0, MMW_CFAR_OS, 3, 1, 4, dets, counts, -1)));
    // the CFAR arguments mmw_cfar1d refuses
    for (int kind : {-1, 4, 2147483647}) CHECK(refused(call(ctx, cube, 1, V, S, C, 0, kind, 3, 1, 4, dets, counts, S)));
    CHECK(refused(call(ctx, cube, 1, V, S, C, 0, MMW_CFAR_CA, -1, 1, 0, dets, counts, S)));
    CHECK(refused(call(ctx, cube, 1, V, S, C, 0, MMW_CFAR_CA, 3, -1, 0, dets, counts, S)));
    CHECK(refused(call(ctx, cube, 1, V, S, C, 0, MMW_CFAR_GO, 513, 0, 0, dets, counts, S)));
    for (int k : {0, 7, -1, 2147483647}) CHECK(refused(call(ctx, cube, 1, V, S, C, 0, MMW_CFAR_OS, 3, 1, k, dets, counts, S)));
    // n_frames == 0 does not excuse a bad argument; a refused call names what it refused
    CHECK(refused(call(ctx, cube, 0, V, S, C, C, MMW_CFAR_OS, 3, 1, 4, dets, counts, S)));
    CHECK(call(ctx, cube, 1, V, S, C, 9, MMW_CFAR_OS, 3, 1, 4, dets, counts, S) == MMW_ERR_INVALID);
    CHECK(std::strstr(mmw::g_last_error.c_str(), "chirp_idx 9") != nullptr);
    mmw::g_last_error.clear();
    // more cells than the kernel's flag table holds: refused as unsupported, before the context is used
    CHECK(call(ctx, cube, 1, V, 49153, C, 0, MMW_CFAR_OS, 3, 1, 4, dets, counts, S) == MMW_ERR_UNSUPPORTED);
}

int main() {
    // never dereferenced: both entries hand their checks to functions that are not given the context, and every call below ends in
    // those functions, at the n_frames == 0 return behind them or at the shape limit
    alignas(64) static unsigned char ctx_bytes[64];
    mmw_ctx *ctx = reinterpret_cast<mmw_ctx *>(ctx_bytes);
    sar_checks(ctx);
    range_checks(ctx);
    std::printf("sar_range_sanitize: %d checks, %d failures\n", calls, fails);
    return fails ? 1 : 0;
}
