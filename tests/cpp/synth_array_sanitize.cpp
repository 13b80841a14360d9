// mmw_synth_array's host code under AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own: the translation unit
// mmw_tu_synth_array.hip compiled host-only (kernels become launch stubs that are never reached here) and linked with this
// driver.  The entry judges every argument before it touches its context, so a context that is never dereferenced stands in for a
// real one: each class of refused argument must come back as MMW_ERR_INVALID with an error text, and n_out == 0 as MMW_OK,
// without a device.  The window arithmetic (mmw_diag_synth_array_window) runs over a sweep of shapes with exactly sized arrays.
// mmw_last_error's storage and the two functions of other units the plumbing refers to are supplied here.
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
    // never dereferenced: the entry hands its checks to a function that is not given the context (sa_validate), and every call
    // below ends in that function or at the n_out == 0 return right behind it
    alignas(64) static unsigned char ctx_bytes[64];
    mmw_ctx *ctx = reinterpret_cast<mmw_ctx *>(ctx_bytes);
    const int N = 6, V = 2, S = 4, C = 8, T = 3, H = 2;
    alignas(16) static float cube[8], out[8];           // never dereferenced either (device pointers to the entry)
    std::vector<double> P((size_t)2 * 3 * H * C, 0.0), dirs((size_t)3 * T, 0.0);
    const int32_t good[2] = {1, 4};
    auto call = [&](mmw_ctx *c, const void *cb, int v, int k, int h, const int32_t *fr, int n_out, const double *p, const double *d,
                    int t, double lam, void *o) { return mmw_synth_array(c, cb, N, V, S, C, v, k, h, fr, n_out, p, d, t, lam, o); };
    // null pointers
    CHECK(refused(call(nullptr, cube, 0, 1, H, good, 2, P.data(), dirs.data(), T, 0.005, out)));
    CHECK(refused(call(ctx, nullptr, 0, 1, H, good, 2, P.data(), dirs.data(), T, 0.005, out)));
    CHECK(refused(call(ctx, cube, 0, 1, H, nullptr, 2, P.data(), dirs.data(), T, 0.005, out)));
    CHECK(refused(call(ctx, cube, 0, 1, H, good, 2, nullptr, dirs.data(), T, 0.005, out)));
    CHECK(refused(call(ctx, cube, 0, 1, H, good, 2, P.data(), nullptr, T, 0.005, out)));
    CHECK(refused(call(ctx, cube, 0, 1, H, good, 2, P.data(), dirs.data(), T, 0.005, nullptr)));
    // antenna, stride, window length, directions, wavelength
    for (int v : {-1, V, V + 7, -2147483647 - 1, 2147483647}) CHECK(refused(call(ctx, cube, v, 1, H, good, 2, P.data(), dirs.data(), T, 0.005, out)));
    for (int k : {0, -1, -2147483647 - 1}) CHECK(refused(call(ctx, cube, 0, k, H, good, 2, P.data(), dirs.data(), T, 0.005, out)));
    for (int h : {0, -1, -2147483647 - 1}) CHECK(refused(call(ctx, cube, 0, 1, h, good, 2, P.data(), dirs.data(), T, 0.005, out)));
    CHECK(refused(call(ctx, cube, 0, 1, 2147483647, good, 2, P.data(), dirs.data(), T, 0.005, out)));     // E beyond 2^24
    for (int t : {0, -1}) CHECK(refused(call(ctx, cube, 0, 1, H, good, 2, P.data(), dirs.data(), t, 0.005, out)));
    for (double lam : {0.0, -0.005, (double)NAN}) CHECK(refused(call(ctx, cube, 0, 1, H, good, 2, P.data(), dirs.data(), T, lam, out)));
    // the frame list: unsorted, repeated, out of range, a negative count
    const int32_t unsorted[2] = {4, 1}, repeated[2] = {3, 3}, past[2] = {1, N}, negative[2] = {-1, 2};
    for (const int32_t *fr : {unsorted, repeated, past, negative}) CHECK(refused(call(ctx, cube, 0, 1, H, fr, 2, P.data(), dirs.data(), T, 0.005, out)));
    CHECK(refused(call(ctx, cube, 0, 1, H, good, -1, P.data(), dirs.data(), T, 0.005, out)));
    CHECK(refused(call(ctx, cube, 0, 1, H, good, 65536, P.data(), dirs.data(), T, 0.005, out)));
    CHECK(refused(mmw_synth_array(ctx, cube, N, 0, S, C, 0, 1, H, good, 2, P.data(), dirs.data(), T, 0.005, out)));
    CHECK(refused(mmw_synth_array(ctx, cube, -1, V, S, C, 0, 1, H, good, 0, P.data(), dirs.data(), T, 0.005, out)));
    // a refused call names what it refused
    CHECK(call(ctx, cube, 5, 1, H, good, 2, P.data(), dirs.data(), T, 0.005, out) == MMW_ERR_INVALID);
    CHECK(std::strstr(mmw::g_last_error.c_str(), "v 5") != nullptr);
    CHECK(call(ctx, cube, 0, 1, H, repeated, 2, P.data(), dirs.data(), T, 0.005, out) == MMW_ERR_INVALID);
    CHECK(std::strstr(mmw::g_last_error.c_str(), "ascending") != nullptr);
    // no outputs: a successful no-op; it does not excuse a bad argument
    CHECK(call(ctx, cube, V - 1, 3, 7, good, 0, P.data(), dirs.data(), T, 0.005, out) == MMW_OK);
    CHECK(refused(call(ctx, cube, V, 1, H, good, 0, P.data(), dirs.data(), T, 0.005, out)));
    // the window arithmetic with arrays of exactly the size it is told: the segments of every run tile the run
    for (int c : {1, 7, 8, 16, 20, 21, 32, 34})
        for (int k : {1, 3})
            for (int h : {1, 2, 3, 4})
                for (int n : {8, 16, 32, 64}) {
                    const int Cv = (c + k - 1) / k, E = h * Cv;
                    for (int e0 = 0; e0 < E + n; e0 += n)
                        for (int cap : {1, 8}) {
                            std::vector<int32_t> segs((size_t)4 * cap);
                            int32_t info[4];
                            CHECK(mmw_diag_synth_array_window(c, k, h, h, e0, n, segs.data(), cap, info) == MMW_OK);
                            int covered = 0;
                            for (int i = 0; i < info[0] && i < cap; ++i) covered += segs[4 * i + 3];
                            const int want = e0 >= E ? 0 : (e0 + n <= E ? n : E - e0);
                            if (info[0] <= cap) CHECK(covered == want);
                        }
                }
    CHECK(refused(mmw_diag_synth_array_window(8, 1, 2, 0, 0, 8, nullptr, 4, nullptr)));
    std::printf("synth_array_sanitize: %d checks, %d failures\n", calls, fails);
    return fails ? 1 : 0;
}
