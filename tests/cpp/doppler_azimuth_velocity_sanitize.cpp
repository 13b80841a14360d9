// The host code of mmw_doppler_azimuth_ransac / mmw_diag_doppler_azimuth_ransac_host under AddressSanitizer +
// UndefinedBehaviorSanitizer, as a program of its own: the translation unit mmw_tu_dopaz_velocity.hip compiled host-only (the
// kernel becomes a launch stub that is never reached here) and linked with this driver.  Both entries judge every argument before
// the device entry touches its context, so a context that is never dereferenced stands in for a real one: each class of refused
// argument must come back as MMW_ERR_INVALID (n_rows beyond the limit: MMW_ERR_UNSUPPORTED) with an error text that names what
// was refused and with the sentinel-filled outputs untouched, and F == 0 / G == 0 as MMW_OK, without a device.  Every array is
// exactly as long as the entries are told.  The host-only entry then runs the shared rule on the boundary sizes (0, 9, 10, 11,
// 63, 64, 65 and 512 rows, short frames, -2 entries) with made-up subset tables.  mmw_last_error's storage and the one function
// of another unit the plumbing refers to are supplied here.
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

static bool refused(int rc, const char *names = nullptr, int code = MMW_ERR_INVALID) {
    const bool ok = rc == code && !mmw::g_last_error.empty() && (!names || std::strstr(mmw::g_last_error.c_str(), names));
    if (!ok) std::fprintf(stderr, "  rc %d, text '%s'\n", rc, mmw::g_last_error.c_str());
    mmw::g_last_error.clear();
    return ok;
}

constexpr double SENTINEL = -77.0;

static long trials_len(int n_tab) { return ((long)(10 + n_tab) * (11 + n_tab) - 110) / 2; }

struct Args {
    mmw_ctx *ctx = nullptr;
    int G, F, n_rows, n_cols = 7, n_tab, g_az = 0, g_el = -1, mode = 0, vel_per_frame = 0, vel_len;
    int tab_told, trials_told;
    std::vector<int32_t> row, zero, m, subsets, trials;
    std::vector<double> vel, cos_t, sin_t, theta, out;
    std::vector<int32_t> flags;
    double thr[4] = {0.15, 0.20, 0.6, 0.75};
    const char *null_one = "";
    bool no_m = true;

    Args(int G_, int F_, int n_rows_) : G(G_), F(F_), n_rows(n_rows_) {
        n_tab = n_rows >= 10 ? n_rows - 9 : 0;
        tab_told = n_tab, trials_told = (int)trials_len(n_tab), vel_len = n_rows;
        row.assign((size_t)G * F * n_rows, -1);
        zero.assign((size_t)G * F, -1);
        m.assign((size_t)F, n_rows);
        vel.resize((size_t)n_rows);
        for (int r = 0; r < n_rows; ++r) vel[r] = -2.0 + 4.0 * r / (n_rows > 0 ? n_rows : 1);
        for (int c = 0; c < n_cols; ++c) {
            theta.push_back(-0.9 + 0.3 * c);
            cos_t.push_back(std::cos(theta[c]));
            sin_t.push_back(std::sin(theta[c]));
        }
        // made-up subsets: trial t of N points takes the points (7 t + 3 k) mod N -- valid indices, which is all the rule needs
        subsets.assign((size_t)(n_tab > 0 ? n_tab : 1) * 200, 0);
        for (int i = 0; i < n_tab; ++i)
            for (int t = 0; t < 20; ++t)
                for (int k = 0; k < 10; ++k) subsets[((size_t)i * 20 + t) * 10 + k] = (7 * t + 3 * k) % (10 + i);
        trials.assign((size_t)(trials_told > 0 ? trials_told : 1), 20);
        out.assign((size_t)G * F * 4, SENTINEL);
        flags.assign((size_t)G * F, (int32_t)SENTINEL);
    }
    bool untouched() const {
        for (double v : out) if (v != SENTINEL) return false;
        for (int32_t v : flags) if (v != (int32_t)SENTINEL) return false;
        return true;
    }
    template <class T> T *p(std::vector<T> &v, const char *name) { return std::strcmp(null_one, name) ? v.data() : nullptr; }
    int run(bool device) {
        const int32_t *hm = no_m ? nullptr : m.data();
        if (device)
            return mmw_doppler_azimuth_ransac(ctx, p(row, "row"), p(zero, "zero"), G, F, n_rows, hm, p(vel, "vel"), vel_len, vel_per_frame,
                                              p(cos_t, "cos"), p(sin_t, "sin"), p(theta, "theta"), n_cols, p(subsets, "subsets"),
                                              p(trials, "trials"), tab_told, trials_told, g_az, g_el, mode, thr[0], thr[1], thr[2], thr[3],
                                              p(out, "out"), p(flags, "flags"));
        return mmw_diag_doppler_azimuth_ransac_host(p(row, "row"), p(zero, "zero"), G, F, n_rows, hm, p(vel, "vel"), vel_len,
                                                    vel_per_frame, p(cos_t, "cos"), p(sin_t, "sin"), p(theta, "theta"), n_cols,
                                                    p(subsets, "subsets"), p(trials, "trials"), tab_told, trials_told, g_az, g_el, mode,
                                                    thr[0], thr[1], thr[2], thr[3], p(out, "out"), p(flags, "flags"));
    }
};

#define REFUSED(a, ...) CHECK(refused((a).run(device), __VA_ARGS__) && (a).untouched())

int main() {
    // never dereferenced: every call of the device entry below ends in dzv_validate, which is not given the context, or at the
    // F == 0 / G == 0 return right behind it
    alignas(64) static unsigned char ctx_bytes[64];
    for (bool device : {true, false}) {
        auto fresh = [&]() {
            Args a(2, 3, 12);
            a.ctx = reinterpret_cast<mmw_ctx *>(ctx_bytes);
            a.g_el = 1;
            return a;
        };
        if (device) { Args a = fresh(); a.ctx = nullptr; REFUSED(a, "null"); }
        for (const char *name : {"row", "zero", "vel", "cos", "sin", "theta", "subsets", "trials", "out", "flags"}) {
            Args a = fresh(); a.null_one = name; REFUSED(a, "null");
        }
        for (int n : {-1, -2147483647 - 1}) {
            { Args a = fresh(); a.G = n; REFUSED(a, "negative count"); }
            { Args a = fresh(); a.F = n; REFUSED(a, "negative count"); }
            { Args a = fresh(); a.n_rows = n; REFUSED(a, "negative count"); }
            { Args a = fresh(); a.vel_len = n; REFUSED(a, "negative count"); }
            { Args a = fresh(); a.tab_told = n; REFUSED(a, "negative count"); }
            { Args a = fresh(); a.trials_told = n; REFUSED(a, "negative count"); }
        }
        for (int n : {0, -1}) { Args a = fresh(); a.n_cols = n; REFUSED(a, "n_cols"); }
        for (int g : {-1, 2, 2147483647, -2147483647 - 1}) { Args a = fresh(); a.g_az = g; REFUSED(a, "g_az"); }
        for (int g : {-2, 2, 2147483647, -2147483647 - 1}) { Args a = fresh(); a.g_el = g; REFUSED(a, "g_el"); }
        for (int mf : {-1, 13, 2147483647, -2147483647 - 1}) { Args a = fresh(); a.no_m = false; a.m[2] = mf; REFUSED(a, "frame 2"); }
        { Args a = fresh(); a.vel_len = 11; REFUSED(a, "velocity table"); }
        { Args a = fresh(); a.tab_told = 2; REFUSED(a, "subset tables"); }
        { Args a = fresh(); a.trials_told -= 1; REFUSED(a, "trial table"); }
        { Args a = fresh(); a.mode = 4; REFUSED(a, "mode"); }
        { Args a = fresh(); a.vel_per_frame = 3; REFUSED(a, "vel_per_frame"); }
        for (int k = 0; k < 4; ++k)
            for (double v : {(double)NAN, (double)INFINITY, -(double)INFINITY}) { Args a = fresh(); a.thr[k] = v; REFUSED(a, "not finite"); }
        { Args a = fresh(); a.F = 100000000; REFUSED(a, "32-bit"); }
        { Args a = fresh(); a.n_rows = 513; a.vel_len = 513; a.tab_told = 504; a.trials_told = (int)trials_len(504);
          REFUSED(a, "513", MMW_ERR_UNSUPPORTED); }
        if (device) {
            { Args a = fresh(); a.F = 0; CHECK(a.run(device) == MMW_OK && mmw::g_last_error.empty() && a.untouched()); }
            { Args a = fresh(); a.F = 0; a.n_cols = 0; REFUSED(a, "n_cols"); }
            { Args a = fresh(); a.G = 0; a.g_az = 5; CHECK(a.run(device) == MMW_OK && mmw::g_last_error.empty() && a.untouched()); }
        }
    }
    // the shared rule on the host at the boundary sizes: every row of every frame with a peak near a line, then variations
    for (int n_rows : {0, 1, 9, 10, 11, 63, 64, 65, 512}) {
        Args a(2, 4, n_rows);
        a.g_el = 1;
        a.no_m = false;
        a.vel_per_frame = 1;
        a.vel.resize((size_t)a.F * n_rows);
        for (int f = 0; f < a.F; ++f)
            for (int r = 0; r < n_rows; ++r) a.vel[(size_t)f * n_rows + r] = -2.0 + 4.0 * r / n_rows + 0.01 * f;
        for (size_t i = 0; i < a.row.size(); ++i) a.row[i] = (int32_t)((i * 5) % 7);
        for (int f = 0; f < a.F; ++f) a.zero[f] = n_rows > 0 ? (f % 2 ? n_rows / 4 : -1) : -1, a.zero[a.F + f] = n_rows > 2 ? 1 : -1;
        if (n_rows > 0) a.m[1] = n_rows / 2, a.m[3] = 0, a.zero[3] = a.zero[a.F + 3] = -1, a.zero[1] = a.zero[a.F + 1] = 0;
        if (n_rows > 2) a.row[2] = -2, a.row[(size_t)n_rows * 2 + 1] = -1;
        if (n_rows == 0) a.zero.assign(a.zero.size(), -1), a.row.reserve(1), a.vel.reserve(1);   // no rows: non-null, never read
        const int rc = a.run(false);
        if (rc != MMW_OK) std::fprintf(stderr, "  n_rows %d: rc %d, text '%s'\n", n_rows, rc, mmw::g_last_error.c_str());
        CHECK(rc == MMW_OK && mmw::g_last_error.empty());
        for (int g = 0; g < 2; ++g)
            for (int f = 0; f < a.F; ++f) {
                const int32_t w = a.flags[(size_t)g * a.F + f];
                const int status = (w >> MMW_DOPAZ_STATUS_SHIFT) & MMW_DOPAZ_STATUS_MASK;
                CHECK(w >= 0 && (w >> MMW_DOPAZ_INLIERS_SHIFT) <= n_rows);
                if (n_rows > 2 && g == 0 && f == 0) CHECK((w & MMW_DOPAZ_FLAG_MASK) == MMW_DOPAZ_FLAG_UNDECIDED);
                if (f == 3 || n_rows == 0) CHECK(status == MMW_DOPAZ_STATUS_EMPTY && (w & MMW_DOPAZ_FLAG_MASK) == 0);
                else if (n_rows < 10 && !(w & MMW_DOPAZ_FLAG_MASK)) CHECK(status == MMW_DOPAZ_STATUS_FAILED);
                for (int k = 0; k < 4; ++k) CHECK(std::isfinite(a.out[((size_t)g * a.F + f) * 4 + k]));
            }
        a.mode = MMW_DOPAZ_RANSAC_VX_ONLY;
        CHECK(a.run(false) == MMW_OK);
    }
    std::printf("%d checks, %d failures\n", calls, fails);
    return fails ? 1 : 0;
}
