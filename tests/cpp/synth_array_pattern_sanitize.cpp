// mmw_synth_array_pattern's host code under AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own: the translation
// unit mmw_tu_synth_pattern.hip compiled host-only (kernels become launch stubs that are never reached here) and linked with this
// driver.  The entry judges every argument before it touches its context, so a context that is never dereferenced stands in for a
// real one: each class of refused argument must come back as MMW_ERR_INVALID with an error text, and n == 0 as MMW_OK, without a
// device.  The host-only twin runs over a sweep of (n, E, T) with arrays of exactly the size it is told -- a read or a write past
// either end is AddressSanitizer's to report -- on a zero geometry (every pattern value exactly 1, every array factor exactly E)
// and on a random one (finite, at most 1, one value of exactly 1 per frame, |AF| <= E).
#include <cmath>
#include <cstdio>
#include <cstring>
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

int main() {
    // never dereferenced: the entry hands its checks to a function that is not given the context (sap_validate), and every call
    // below ends in that function or at the n == 0 return right behind it
    alignas(64) static unsigned char ctx_bytes[64];
    mmw_ctx *ctx = reinterpret_cast<mmw_ctx *>(ctx_bytes);
    const int n = 2, E = 5, T = 3;
    alignas(16) static double dP[8];                    // never dereferenced either (device pointers to the entry)
    alignas(16) static float dpat[8];
    std::vector<double> dirs((size_t)3 * T, 0.0);
    const double inf = HUGE_VAL;
    // null pointers
    CHECK(refused(mmw_synth_array_pattern(nullptr, dP, n, E, dirs.data(), T, 0.004, dpat, nullptr)));
    CHECK(refused(mmw_synth_array_pattern(ctx, nullptr, n, E, dirs.data(), T, 0.004, dpat, nullptr)));
    CHECK(refused(mmw_synth_array_pattern(ctx, dP, n, E, nullptr, T, 0.004, dpat, nullptr)));
    CHECK(refused(mmw_synth_array_pattern(ctx, dP, n, E, dirs.data(), T, 0.004, nullptr, nullptr)));
    // counts
    for (int bad : {-1, -2147483647 - 1}) CHECK(refused(mmw_synth_array_pattern(ctx, dP, bad, E, dirs.data(), T, 0.004, dpat, nullptr)));
    for (int bad : {0, -1, -2147483647 - 1}) {
        CHECK(refused(mmw_synth_array_pattern(ctx, dP, n, bad, dirs.data(), T, 0.004, dpat, nullptr)));
        CHECK(refused(mmw_synth_array_pattern(ctx, dP, n, E, dirs.data(), bad, 0.004, dpat, nullptr)));
    }
    // the wavelength
    for (double lam : {0.0, -0.004, (double)NAN, inf, -inf}) CHECK(refused(mmw_synth_array_pattern(ctx, dP, n, E, dirs.data(), T, lam, dpat, nullptr)));
    // tables beyond int32 entries
    CHECK(refused(mmw_synth_array_pattern(ctx, dP, 65536, E, dirs.data(), 32768, 0.004, dpat, nullptr)));           // n T = 2^31
    CHECK(refused(mmw_synth_array_pattern(ctx, dP, 2147483647, E, dirs.data(), 2147483647, 0.004, dpat, nullptr)));
    CHECK(refused(mmw_synth_array_pattern(ctx, dP, 3, 238609295, dirs.data(), T, 0.004, dpat, nullptr)));           // 3 n E = 2^31 + 7
    CHECK(refused(mmw_synth_array_pattern(ctx, dP, 2147483647, 2147483647, dirs.data(), 1, 0.004, dpat, nullptr)));
    // a refused call names what it refused
    CHECK(mmw_synth_array_pattern(ctx, dP, n, E, dirs.data(), T, -1.5, dpat, nullptr) == MMW_ERR_INVALID);
    CHECK(std::strstr(mmw::g_last_error.c_str(), "lambda_m") != nullptr);
    // no frames: a successful no-op; it does not excuse a bad argument
    CHECK(mmw_synth_array_pattern(ctx, dP, 0, E, dirs.data(), T, 0.004, dpat, nullptr) == MMW_OK);
    CHECK(mmw_synth_array_pattern(ctx, dP, 0, 2147483647, dirs.data(), 2147483647, 0.004, dpat, dP) == MMW_OK);
    CHECK(refused(mmw_synth_array_pattern(ctx, dP, 0, 0, dirs.data(), T, 0.004, dpat, nullptr)));
    CHECK(refused(mmw_synth_array_pattern(ctx, dP, 0, E, dirs.data(), T, 0.0, dpat, nullptr)));
    // the host-only twin refuses the same
    CHECK(refused(mmw_diag_synth_array_pattern_host(nullptr, n, E, dirs.data(), T, 0.004, dpat, nullptr)));
    CHECK(refused(mmw_diag_synth_array_pattern_host(dP, n, E, nullptr, T, 0.004, dpat, nullptr)));
    CHECK(refused(mmw_diag_synth_array_pattern_host(dP, n, E, dirs.data(), T, 0.004, nullptr, nullptr)));
    CHECK(refused(mmw_diag_synth_array_pattern_host(dP, n, 0, dirs.data(), T, 0.004, dpat, nullptr)));
    CHECK(refused(mmw_diag_synth_array_pattern_host(dP, n, E, dirs.data(), 0, 0.004, dpat, nullptr)));
    CHECK(refused(mmw_diag_synth_array_pattern_host(dP, -1, E, dirs.data(), T, 0.004, dpat, nullptr)));
    CHECK(refused(mmw_diag_synth_array_pattern_host(dP, n, E, dirs.data(), T, inf, dpat, nullptr)));
    CHECK(mmw_diag_synth_array_pattern_host(dP, 0, E, dirs.data(), T, 0.004, dpat, nullptr) == MMW_OK);
    // the sweep: exactly sized arrays
    unsigned long long seed = 88172645463325252ULL;
    auto uniform = [&]() {          // xorshift64: [0, 1)
        seed ^= seed << 13, seed ^= seed >> 7, seed ^= seed << 17;
        return (double)(seed >> 11) / 9007199254740992.0;
    };
    for (int nn : {1, 3})
        for (int e : {1, 63, 64, 65, 257})
            for (int t : {1, 63, 64, 65, 257})
                for (int random : {0, 1})
                    for (int with_af : {0, 1}) {
                        std::vector<double> P((size_t)nn * 3 * e, 0.0), d((size_t)3 * t), af((size_t)(with_af ? 2 * nn * t : 0));
                        std::vector<float> pat((size_t)nn * t, -7.0f);
                        for (double &x : d) x = 2.0 * uniform() - 1.0;
                        if (random)
                            for (double &x : P) x = 10.0 * uniform() - 5.0;
                        CHECK(mmw_diag_synth_array_pattern_host(P.data(), nn, e, d.data(), t, 0.0039, pat.data(), with_af ? af.data() : nullptr) == MMW_OK);
                        bool ok = true;
                        for (int i = 0; i < nn; ++i) {
                            int ones = 0;
                            for (int q = 0; q < t; ++q) {
                                const float v = pat[(size_t)i * t + q];
                                ok = ok && v >= 0.0f && v <= 1.0f && (random || v == 1.0f);
                                ones += v == 1.0f;
                                if (with_af) {
                                    const double re = af[2 * ((size_t)i * t + q)], im = af[2 * ((size_t)i * t + q) + 1];
                                    ok = ok && std::hypot(re, im) <= e * (1.0 + 1e-12) && (random || (re == (double)e && im == 0.0));
                                }
                            }
                            ok = ok && ones >= 1;
                        }
                        CHECK(ok);
                    }
    std::printf("synth_array_pattern_sanitize: %d checks, %d failures\n", calls, fails);
    return fails ? 1 : 0;
}
