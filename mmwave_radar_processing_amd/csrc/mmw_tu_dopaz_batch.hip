// Translation unit of the batched Doppler-azimuth maps (mmw_dopaz_batch.h).
#include <algorithm>
#include <climits>

#include "mmw_ctx.h"
#include "mmw_fft_generic.h"
namespace mmw {
extern template int launch_fft_axis<float, float>(mmw_ctx *, FftArgs, int, bool);      // mmw_tu_generic.hip
}
#include "mmw_dopaz_batch.h"

using namespace mmw;

namespace {

// what both entries share once their arguments have been judged
struct DopazCall {
    int n = 0, U = 0, max_rows = 0, pmax = 1;
    std::vector<int> sets, sets_u, ants;        // per set: antennas (+ shift offset); the same through the union; the union
    std::vector<int2> rows, rows0;              // [lo, hi) per frame; [0, hi - lo) per frame
};

// Every argument is judged here, before the context is touched: the function is not given the context, so a refused call cannot
// enqueue anything and needs no device (tests/cpp/doppler_azimuth_batch_sanitize.cpp relies on it).  M == 0: the coarse entry.
int dz_validate(bool have_ctx, const void *d_cubes, const float *d_out, int n_frames, int V, int S, int C, int A, const int32_t *h_rx,
                int n_sets, int n_rx, const int32_t *h_set_flags, const int32_t *h_rows, int flags, bool zoom, int n_used,
                const double *h_freq, int M, DopazCall *call) {
    MMW_REQUIRE(have_ctx && d_cubes && d_out && h_set_flags && h_rows && (!zoom || h_freq),
                "null argument (ctx %d, d_cubes %d, d_out %d, h_set_flags %d, h_rows %d, h_freq %d)", (int)have_ctx, d_cubes != nullptr,
                d_out != nullptr, h_set_flags != nullptr, h_rows != nullptr, !zoom || h_freq != nullptr);
    MMW_REQUIRE(n_frames >= 0, "n_frames is %d", n_frames);
    MMW_REQUIRE(V > 0 && S > 0 && C > 0 && A > 0, "bad shape: V %d, S %d, C %d, A %d must all be positive", V, S, C, A);
    MMW_REQUIRE(n_sets >= 1, "n_sets is %d: at least one antenna set", n_sets);
    MMW_REQUIRE(n_rx >= 0 && n_rx <= DOPAZ_MAX_N, "n_rx %d is not in [0, %d]", n_rx, DOPAZ_MAX_N);
    MMW_REQUIRE(n_rx == 0 || h_rx, "null argument (h_rx with n_rx %d)", n_rx);
    MMW_REQUIRE(n_rx > 0 || (n_sets == 1 && V <= DOPAZ_MAX_N), "n_rx 0 is ONE set of all V antennas, at most %d: n_sets %d, V %d",
                DOPAZ_MAX_N, n_sets, V);
    MMW_REQUIRE((flags & ~MMW_ANGLE_NO_WINDOW) == 0, "unknown flag bits %d (MMW_ANGLE_NO_WINDOW only; the shift is per set)", flags);
    if (zoom) {
        MMW_REQUIRE(M >= 1, "M is %d zoom bins", M);
        MMW_REQUIRE(n_used >= 1 && n_used <= C, "n_used %d is not in [1, %d]: the zoom transform is defined on the cube's chirps", n_used, C);
    }
    const int n = n_rx ? n_rx : V;
    call->n = n;
    call->sets.assign((size_t)n_sets * DOPAZ_SET_WORDS, 0);
    std::vector<char> used((size_t)V, 0);
    for (int k = 0; k < n_sets; ++k) {
        MMW_REQUIRE((h_set_flags[k] & ~MMW_ANGLE_NO_SHIFT) == 0, "set %d: unknown flag bits %d (MMW_ANGLE_NO_SHIFT only)", k, h_set_flags[k]);
        int *set = call->sets.data() + (size_t)k * DOPAZ_SET_WORDS;
        for (int j = 0; j < n; ++j) {
            const int v = n_rx ? h_rx[(size_t)k * n_rx + j] : j;
            MMW_REQUIRE(v >= 0 && v < V, "set %d, entry %d: %d is not an antenna of [0, %d)", k, j, v, V);
            for (int i = 0; i < j; ++i) MMW_REQUIRE(set[i] != v, "set %d: antenna %d is repeated (entries %d and %d)", k, v, i, j);
            set[j] = v;
            used[v] = 1;
        }
        set[DOPAZ_MAX_N] = (h_set_flags[k] & MMW_ANGLE_NO_SHIFT) ? 0 : 32;
    }
    call->rows.resize((size_t)n_frames);
    call->rows0.resize((size_t)n_frames);
    for (int f = 0; f < n_frames; ++f) {
        const int lo = h_rows[2 * (size_t)f], hi = h_rows[2 * (size_t)f + 1];
        MMW_REQUIRE(0 <= lo && lo <= hi && hi <= S, "frame %d: row interval [%d, %d) is not inside 0 <= lo <= hi <= %d", f, lo, hi, S);
        call->rows[f] = make_int2(lo, hi);
        call->rows0[f] = make_int2(0, hi - lo);
        call->max_rows = std::max(call->max_rows, hi - lo);
    }
    call->pmax = dopaz_parts(call->max_rows);
    MMW_REQUIRE((double)n_sets * n_frames * std::max(C, zoom ? M : 0) * A <= (double)INT_MAX,
                "%d sets x %d frames x %d rows x %d angle bins do not fit a 32-bit element index", n_sets, n_frames,
                std::max(C, zoom ? M : 0), A);
    if (A != 64)
        return set_error(MMW_ERR_UNSUPPORTED, "the batched Doppler-azimuth entries are built for 64 angle bins, not %d (the "
                         "single-frame entries take other sizes)", A);
    if (n_sets > 65535) return set_error(MMW_ERR_UNSUPPORTED, "%d antenna sets: at most 65535", n_sets);
    if (zoom && dopaz_zoom_lds(n_used) > 160 * 1024)
        return set_error(MMW_ERR_UNSUPPORTED, "zoom kernel: %d chirps need %zu bytes of LDS (at most 160 KiB)", n_used, dopaz_zoom_lds(n_used));
    // the union of the sets, and every set again as indices into it (the zoom transform only makes those planes)
    std::vector<int> where((size_t)V, 0);
    for (int v = 0; v < V; ++v)
        if (used[v]) {
            where[v] = (int)call->ants.size();
            call->ants.push_back(v);
        }
    call->U = (int)call->ants.size();
    call->sets_u = call->sets;
    for (int k = 0; k < n_sets; ++k)
        for (int j = 0; j < n; ++j) call->sets_u[(size_t)k * DOPAZ_SET_WORDS + j] = where[call->sets[(size_t)k * DOPAZ_SET_WORDS + j]];
    return MMW_OK;
}

size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

long chunk_frames(const mmw_ctx *ctx, size_t frame_bytes, int n_frames, int n_sets) {
    const size_t budget = (size_t)std::max(1, opt_int(ctx, "MMW_DOPAZ_CHUNK_MB", 1024)) << 20;      // <= 1 GiB of intermediates per pass
    return std::max<long>(1, std::min<long>({(long)(budget / frame_bytes), 65535L / n_sets, (long)n_frames}));
}

int launch_rmean(mmw_ctx *ctx, DopazArgs a) {
    const dim3 grid((unsigned)((a.ncols + 63) / 64), (unsigned)a.pmax, (unsigned)(a.nf * a.n_sets));
    if (a.n <= 4) hipLaunchKernelGGL(k_dopaz_rmean<4>, grid, dim3(256), 0, ctx->stream, a);
    else if (a.n <= 8) hipLaunchKernelGGL(k_dopaz_rmean<8>, grid, dim3(256), 0, ctx->stream, a);
    else if (a.n <= 12) hipLaunchKernelGGL(k_dopaz_rmean<12>, grid, dim3(256), 0, ctx->stream, a);
    else hipLaunchKernelGGL(k_dopaz_rmean<16>, grid, dim3(256), 0, ctx->stream, a);
    MMW_TRY(check_launch("dopaz_rmean"));
    const long total = 64L * a.ncols * a.nf * a.n_sets;
    hipLaunchKernelGGL(k_dopaz_finish, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, a);
    return check_launch("dopaz_finish");
}

// host tables of a call -> the head of the scratch; *base is the first byte behind them
struct DeviceTables {
    int2 *rows, *rows0;
    int *sets, *sets_u, *ants;
    double *freq;
    char *rest;
};

size_t tables_bytes(const DopazCall &c, size_t n_freq) {
    return 2 * up256(c.rows.size() * sizeof(int2)) + 2 * up256(c.sets.size() * sizeof(int)) + up256(c.ants.size() * sizeof(int)) +
           up256(n_freq * sizeof(double));
}

int upload_tables(mmw_ctx *ctx, const DopazCall &c, const double *h_freq, size_t n_freq, DeviceTables *t) {
    char *p = (char *)ctx->scratch;
    auto put = [&](const void *h, size_t bytes) -> void * {
        void *d = p;
        if (bytes) (void)hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, ctx->stream);
        p += up256(bytes);
        return d;
    };
    t->rows = (int2 *)put(c.rows.data(), c.rows.size() * sizeof(int2));
    t->rows0 = (int2 *)put(c.rows0.data(), c.rows0.size() * sizeof(int2));
    t->sets = (int *)put(c.sets.data(), c.sets.size() * sizeof(int));
    t->sets_u = (int *)put(c.sets_u.data(), c.sets_u.size() * sizeof(int));
    t->ants = (int *)put(c.ants.data(), c.ants.size() * sizeof(int));
    t->freq = (double *)put(h_freq, n_freq * sizeof(double));
    t->rest = p;
    MMW_HIP(hipStreamSynchronize(ctx->stream));     // the tables are host memory of this call (and reports a failed copy)
    return MMW_OK;
}

void fill_window(DopazArgs *a, int n, int flags) {
    for (int j = 0; j < DOPAZ_MAX_N; ++j) a->h[j] = j >= n ? 0.f : ((flags & MMW_ANGLE_NO_WINDOW) ? 1.f : (float)np_window(TAB_HANN, j, n));
}

}  // namespace

extern "C" {

int mmw_doppler_azimuth_batch(mmw_ctx *ctx, const void *d_cubes, float *d_out, int n_frames, int V, int S, int C, int A,
                              const int32_t *h_rx, int n_sets, int n_rx, const int32_t *h_set_flags, const int32_t *h_rows, int flags) {
    DopazCall call;
    MMW_TRY(dz_validate(ctx != nullptr, d_cubes, d_out, n_frames, V, S, C, A, h_rx, n_sets, n_rx, h_set_flags, h_rows, flags, false, 0,
                        nullptr, 0, &call));
    if (n_frames == 0) return MMW_OK;
    MMW_JOIN(ctx);
    const size_t cube_bytes = (size_t)V * S * C * sizeof(float2);
    const size_t part_bytes = (size_t)n_sets * call.pmax * 64 * C * sizeof(float);
    const long chunk = chunk_frames(ctx, cube_bytes + part_bytes, n_frames, n_sets);
    const size_t tabs = tables_bytes(call, 0);
    MMW_TRY(ensure_scratch(ctx, tabs + up256((size_t)chunk * cube_bytes) + (size_t)chunk * part_bytes));
    DeviceTables t;
    MMW_TRY(upload_tables(ctx, call, nullptr, 0, &t));
    char *d_rd = t.rest;
    DopazArgs a{};
    a.src = (const cplx<float> *)d_rd;
    a.frame_stride = (long)V * S * C;
    a.plane_stride = (long)S * C;
    a.ncols = C;
    a.sets = t.sets;
    a.part = (float *)(d_rd + up256((size_t)chunk * cube_bytes));
    a.out_set_stride = (long)n_frames * C * 64;
    a.n_sets = n_sets, a.n = call.n, a.pmax = call.pmax;
    fill_window(&a, call.n, flags);
    for (long f0 = 0; f0 < n_frames; f0 += chunk) {
        const int nf = (int)std::min<long>(chunk, n_frames - f0);
        // one range-Doppler pass over all V antennas of the chunk, whatever the number of sets (profile family "rd")
        MMW_TRY(mmw_range_doppler(ctx, (const char *)d_cubes + (size_t)f0 * cube_bytes, d_rd, nullptr, nf, V, S, C));
        ProfScope ps(ctx, "dopaz_batch");
        a.rows = t.rows + f0;
        a.out = d_out + (size_t)f0 * C * 64;
        a.nf = nf;
        MMW_TRY(launch_rmean(ctx, a));
    }
    return MMW_OK;
}

int mmw_doppler_azimuth_zoom_batch(mmw_ctx *ctx, const void *d_cubes, float *d_out, int n_frames, int V, int S, int C, int A,
                                   const int32_t *h_rx, int n_sets, int n_rx, const int32_t *h_set_flags, const int32_t *h_rows, int flags,
                                   int n_used, const double *h_freq, int M) {
    DopazCall call;
    MMW_TRY(dz_validate(ctx != nullptr, d_cubes, d_out, n_frames, V, S, C, A, h_rx, n_sets, n_rx, h_set_flags, h_rows, flags, true,
                        n_used, h_freq, M, &call));
    if (n_frames == 0) return MMW_OK;
    MMW_JOIN(ctx);
    const int U = call.U, rmax = std::max(1, call.max_rows);
    const size_t cube_bytes = (size_t)V * S * C * sizeof(float2), zoom_bytes = (size_t)U * rmax * M * sizeof(float2);
    const size_t part_bytes = (size_t)n_sets * call.pmax * 64 * M * sizeof(float);
    const long chunk = chunk_frames(ctx, cube_bytes + zoom_bytes + part_bytes, n_frames, n_sets);
    const size_t tabs = tables_bytes(call, (size_t)n_frames * M);
    MMW_TRY(ensure_scratch(ctx, tabs + up256((size_t)chunk * cube_bytes) + up256((size_t)chunk * zoom_bytes) + (size_t)chunk * part_bytes));
    DeviceTables t;
    MMW_TRY(upload_tables(ctx, call, h_freq, (size_t)n_frames * M, &t));
    char *d_rng = t.rest, *d_zoom = d_rng + up256((size_t)chunk * cube_bytes);
    const size_t lds = dopaz_zoom_lds(n_used);
    if (lds > 64 * 1024)
        MMW_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_dopaz_zoom), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    DopazZoomArgs zz{};
    zz.rng = (const float2 *)d_rng;
    zz.ants = t.ants;
    zz.out = (float2 *)d_zoom;
    zz.U = U, zz.V = V, zz.S = S, zz.C = C, zz.n_used = n_used, zz.M = M, zz.rmax = rmax;
    DopazArgs a{};
    a.src = (const cplx<float> *)d_zoom;
    a.frame_stride = (long)U * rmax * M;
    a.plane_stride = (long)rmax * M;
    a.ncols = M;
    a.sets = t.sets_u;
    a.part = (float *)(d_zoom + up256((size_t)chunk * zoom_bytes));
    a.out_set_stride = (long)n_frames * M * 64;
    a.n_sets = n_sets, a.n = call.n, a.pmax = call.pmax;
    fill_window(&a, call.n, flags);
    ProfScope ps(ctx, "dopaz_zoom_batch");
    for (long f0 = 0; f0 < n_frames; f0 += chunk) {
        const int nf = (int)std::min<long>(chunk, n_frames - f0);
        {
            ProfScope p1(ctx, "dopaz_zoom_range");
            FftArgs r{};                                 // range FFT, Hann(S) x Hann(C) folded into the load: once for all sets
            r.in = (const char *)d_cubes + (size_t)f0 * cube_bytes;
            r.out = d_rng;
            r.outer = nf * V;
            r.inner = C;
            r.n_in = S;
            r.in_outer_stride = r.out_outer_stride = (long)S * C;
            r.in_axis_stride = r.out_axis_stride = C;
            r.in_inner_stride = r.out_inner_stride = 1;
            MMW_TRY(get_table<float>(ctx, TAB_HANN, S, &r.win_axis));
            MMW_TRY(get_table<float>(ctx, TAB_HANN, C, &r.win_inner));
            r.scale = 1.0;
            MMW_TRY((launch_fft_axis<float, float>(ctx, r, S, false)));
        }
        {
            ProfScope p2(ctx, "dopaz_zoom_rows");
            zz.freq = t.freq + (size_t)f0 * M;
            zz.rows = t.rows + f0;
            hipLaunchKernelGGL(k_dopaz_zoom, dim3((unsigned)((M + DOPAZ_ZB - 1) / DOPAZ_ZB), (unsigned)nf), dim3(256), lds, ctx->stream, zz);
            MMW_TRY(check_launch("dopaz_zoom"));
        }
        ProfScope p3(ctx, "dopaz_zoom_mean");
        a.rows = t.rows0 + f0;
        a.out = d_out + (size_t)f0 * M * 64;
        a.nf = nf;
        MMW_TRY(launch_rmean(ctx, a));
    }
    return MMW_OK;
}

}  // extern "C"
