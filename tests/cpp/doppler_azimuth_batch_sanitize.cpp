// The host code of mmw_doppler_azimuth_batch / mmw_doppler_azimuth_zoom_batch under AddressSanitizer + UndefinedBehaviorSanitizer,
// as a program of its own: the translation unit mmw_tu_dopaz_batch.hip compiled host-only (kernels become launch stubs that are
// never reached here) and linked with this driver.  Both entries judge every argument before they touch their context, so a
// context that is never dereferenced stands in for a real one: each class of refused argument must come back as MMW_ERR_INVALID
// (A != 64: MMW_ERR_UNSUPPORTED) with an error text that names what was refused, and n_frames == 0 as MMW_OK, without a device.
// The host arrays are exactly as long as the entries are told.  mmw_last_error's storage and the three functions of other units
// the plumbing refers to are supplied here.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/mmwgpu.h"
#include "../../mmwave_radar_processing_amd/csrc/mmw_ctx.h"
#include "../../mmwave_radar_processing_amd/csrc/mmw_fft_generic.h"

namespace mmw {
int chain_settle(mmw_ctx *) { return MMW_OK; }      // mmw_tu_chain.hip's; only reached through a context with chain work pending
template <> int launch_fft_axis<float, float>(mmw_ctx *, FftArgs, int, bool) { return MMW_ERR_HIP; }    // mmw_tu_generic.hip's; never reached
}  // namespace mmw
extern "C" int mmw_range_doppler(mmw_ctx *, const void *, void *, void *, int, int, int, int) { return MMW_ERR_HIP; }   // mmw_tu_input.hip's; never reached

static int fails = 0, calls = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        ++calls;                                                             \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++fails;                                                         \
        }                                                                    \
    } while (0)

static bool refused(int rc, const char *names = nullptr, int code = MMW_ERR_INVALID) {
    const bool ok = rc == code && !mmw::g_last_error.empty() && (!names || std::strstr(mmw::g_last_error.c_str(), names));
    if (!ok) std::fprintf(stderr, "  rc %d, text '%s'\n", rc, mmw::g_last_error.c_str());
    mmw::g_last_error.clear();
    return ok;
}

struct Args {
    mmw_ctx *ctx;
    const void *cubes;
    float *out;
    int F = 3, V = 12, S = 32, C = 16, A = 64;
    std::vector<int32_t> rx{0, 3, 4, 7, 1, 2, 5, 6}, set_flags{0, MMW_ANGLE_NO_SHIFT}, rows{0, 32, 4, 5, 7, 7};
    int n_sets = 2, n_rx = 4, flags = 0, n_used = 16, M = 5;
    std::vector<double> freq = std::vector<double>(15, 0.125);
    bool no_rx = false, no_set_flags = false, no_rows = false, no_freq = false;
};

// both entries with the same arguments; the refusal has to be the same
static int run(const Args &a, bool zoom) {
    const int32_t *rx = a.no_rx ? nullptr : a.rx.data(), *sf = a.no_set_flags ? nullptr : a.set_flags.data();
    const int32_t *rows = a.no_rows ? nullptr : a.rows.data();
    if (zoom)
        return mmw_doppler_azimuth_zoom_batch(a.ctx, a.cubes, a.out, a.F, a.V, a.S, a.C, a.A, rx, a.n_sets, a.n_rx, sf, rows, a.flags,
                                              a.n_used, a.no_freq ? nullptr : a.freq.data(), a.M);
    return mmw_doppler_azimuth_batch(a.ctx, a.cubes, a.out, a.F, a.V, a.S, a.C, a.A, rx, a.n_sets, a.n_rx, sf, rows, a.flags);
}

int main() {
    // never dereferenced: the entries hand their checks to a function that is not given the context (dz_validate), and every call
    // below ends in that function or at the n_frames == 0 return right behind it
    alignas(64) static unsigned char ctx_bytes[64];
    alignas(16) static float cube[8], out[8];           // never dereferenced either (device pointers to the entries)
    Args good;
    good.ctx = reinterpret_cast<mmw_ctx *>(ctx_bytes);
    good.cubes = cube;
    good.out = out;
    for (bool zoom : {false, true}) {
        Args a = good;
        // null pointers
        a.ctx = nullptr; CHECK(refused(run(a, zoom), "null")); a = good;
        a.cubes = nullptr; CHECK(refused(run(a, zoom), "null")); a = good;
        a.out = nullptr; CHECK(refused(run(a, zoom), "null")); a = good;
        a.no_rx = true; CHECK(refused(run(a, zoom), "h_rx")); a = good;
        a.no_set_flags = true; CHECK(refused(run(a, zoom), "null")); a = good;
        a.no_rows = true; CHECK(refused(run(a, zoom), "null")); a = good;
        if (zoom) { a.no_freq = true; CHECK(refused(run(a, zoom), "null")); a = good; }
        // counts
        for (int F : {-1, -2147483647 - 1}) { a.F = F; CHECK(refused(run(a, zoom), "n_frames")); a = good; }
        for (int n : {0, -1, -2147483647 - 1}) { a.n_sets = n; CHECK(refused(run(a, zoom), "n_sets")); a = good; }
        for (int n : {-1, 17, 2147483647, -2147483647 - 1}) { a.n_rx = n; CHECK(refused(run(a, zoom), "n_rx")); a = good; }
        a.n_rx = 0; CHECK(refused(run(a, zoom), "n_rx 0")); a = good;                  // all antennas is ONE set
        a.n_rx = 0, a.n_sets = 1, a.V = 17; CHECK(refused(run(a, zoom), "n_rx 0")); a = good;
        for (int v : {0, -3}) { a.V = v; CHECK(refused(run(a, zoom), "shape")); a = good; }
        // antennas: outside [0, V), repeated within a set -- the text names set and entry
        for (int v : {-1, 12, 2147483647, -2147483647 - 1}) { a.rx[6] = v; CHECK(refused(run(a, zoom), "set 1, entry 2")); a = good; }
        a.rx[3] = 3; CHECK(refused(run(a, zoom), "set 0: antenna 3 is repeated")); a = good;
        // row intervals -- the text names the frame
        const int bad_rows[][2] = {{-1, 4}, {5, 4}, {0, 33}, {33, 33}, {2147483647, -2147483647 - 1}};
        for (auto &r : bad_rows) { a.rows[4] = r[0], a.rows[5] = r[1]; CHECK(refused(run(a, zoom), "frame 2")); a = good; }
        // flag bits: the shift is per set, the window per call
        for (int fl : {1, 4, 8, -1}) { a.flags = fl; CHECK(refused(run(a, zoom), "flag")); a = good; }
        for (int fl : {1, 2, 8, -1}) { a.set_flags[1] = fl; CHECK(refused(run(a, zoom), "set 1")); a = good; }
        // the output index
        { Args b = good; b.F = 2100000; b.rows.assign((size_t)2 * b.F, 0); b.freq.assign((size_t)b.F * b.M, 0.0); CHECK(refused(run(b, zoom), "32-bit")); }
        if (zoom) {
            for (int n : {0, -1, 17, 2147483647}) { a.n_used = n; CHECK(refused(run(a, zoom), "n_used")); a = good; }
            for (int m : {0, -1}) { a.M = m; CHECK(refused(run(a, zoom), "M is")); a = good; }
        }
        // other angle sizes belong to the single-frame entries
        for (int A : {32, 128}) { a.A = A; CHECK(refused(run(a, zoom), "64 angle bins", MMW_ERR_UNSUPPORTED)); a = good; }
        a.A = 0; CHECK(refused(run(a, zoom), "shape")); a = good;
        // no frames: a successful no-op (the per-frame tables are then empty); it does not excuse a bad argument
        a.F = 0; a.rows.clear(); a.freq.clear(); a.rows.reserve(1); a.freq.reserve(1);
        CHECK(run(a, zoom) == MMW_OK && mmw::g_last_error.empty());
        a.n_sets = 0; CHECK(refused(run(a, zoom), "n_sets")); a.n_sets = 2;
        a.rx[0] = 12; CHECK(refused(run(a, zoom), "set 0, entry 0"));
        // NaN frequencies are data, not errors
        if (zoom) { Args b = good; b.F = 0; b.freq.assign(15, (double)NAN); CHECK(run(b, zoom) == MMW_OK); }
    }
    std::printf("doppler_azimuth_batch_sanitize: %d checks, %d failures\n", calls, fails);
    return fails ? 1 : 0;
}
