// Translation unit of the antenna-integrated detection plane (mmw_integrated.h): mmw_range_doppler_power64 and
// mmw_detect_batch_integrated.
#include "mmw_entry.h"
#include "mmw_integrated.h"

#include <algorithm>

using namespace mmw;

namespace {

int fill_power_list(const int *h_ants, int n_ants, int V, AntList *ants) {
    MMW_REQUIRE(h_ants && n_ants >= 1 && n_ants <= MAX_ANT && n_ants <= V, "antenna list must have 1..min(V, %d) entries", MAX_ANT);
    ants->n = n_ants;
    for (int i = 0; i < n_ants; ++i) {
        MMW_REQUIRE(h_ants[i] >= 0 && h_ants[i] < V, "antenna index %d out of range [0, %d)", h_ants[i], V);
        for (int j = 0; j < i; ++j) MMW_REQUIRE(h_ants[j] != h_ants[i], "antenna index %d is listed twice", h_ants[i]);
        ants->idx[i] = h_ants[i];
    }
    return MMW_OK;
}

// one launch for the whole batch: a frame (every antenna of the list) per workgroup
int launch_rd_pow64_fused(mmw_ctx *ctx, const void *d_cubes, double *d_pow, int n_frames, int V, const AntList &ants) {
    constexpr int S = P64_S, C = P64_C;
    const int grid = std::min(n_frames, ctx->num_cu);
    MMW_TRY(ensure_scratch(ctx, (size_t)grid * S * C * sizeof(cplx<double>)));
    Pow64Args pa{};
    pa.cubes = (const float2 *)d_cubes;
    pa.frame_stride = (long)V * S * C;
    pa.pow = d_pow;
    pa.scratch = (cplx<double> *)ctx->scratch;
    pa.n_frames = n_frames;
    pa.ants = ants;
    const void *p;
    MMW_TRY(get_table<double>(ctx, TAB_HANN, S, &p));
    pa.ws = (const double *)p;
    MMW_TRY(get_table<double>(ctx, TAB_HANN, C, &p));
    pa.wc = (const double *)p;
    MMW_TRY(get_table<double>(ctx, TAB_TWIDDLE, S, &p));
    pa.twS = (const cplx<double> *)p;
    MMW_TRY(get_table<double>(ctx, TAB_TWIDDLE, C, &p));
    pa.twC = (const cplx<double> *)p;
    const size_t lds = pow64_lds();
    MMW_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_rd_pow64_256x128), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_rd_pow64_256x128, dim3((unsigned)grid), dim3(C64_NT), lds, ctx->stream, pa);
    return check_launch("rd_pow64_256x128");
}

// The per-antenna route: mmw_range_doppler_mag64's own pass (whichever kernels it takes for the shape) into a plane behind
// its scratch, then k_pow_accum; chunks of frames whose |RD| planes stay in the Infinity Cache between the two (64 MB).
int rd_pow64_per_antenna(mmw_ctx *ctx, const void *d_cubes, double *d_pow, int n_frames, int V, int S, int C, const AntList &ants) {
    const size_t plane = (size_t)S * C;
    const int chunk = (int)std::min<size_t>((size_t)n_frames, std::max<size_t>(1, ((size_t)64 << 20) / (plane * sizeof(double))));
    // the one-antenna pass works in the head of the scratch (and must not move it once the chunk's planes lie behind it)
    const size_t head = (rd_mag64_scratch_bytes(ctx, chunk, S, C) + 255) & ~(size_t)255;
    MMW_TRY(ensure_scratch(ctx, head + (size_t)chunk * plane * sizeof(double)));
    double *d_mag = (double *)((char *)ctx->scratch + head);
    for (long f0 = 0; f0 < n_frames; f0 += chunk) {
        const int nf = (int)std::min<long>(chunk, n_frames - f0);
        const size_t n = (size_t)nf * plane;
        const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, (size_t)ctx->num_cu * 16);
        for (int ai = 0; ai < ants.n; ++ai) {
            MMW_TRY(range_doppler_mag64_impl(ctx, (const float2 *)d_cubes + f0 * (long)V * S * C, d_mag, nf, V, S, C, ants.idx[ai]));
            hipLaunchKernelGGL(k_pow_accum, dim3(grid), dim3(256), 0, ctx->stream, d_mag, d_pow + f0 * (long)plane, n, ai == 0 ? 1 : 0);
            MMW_TRY(check_launch("pow_accum"));
        }
    }
    return MMW_OK;
}

int range_doppler_power64_impl(mmw_ctx *ctx, const void *d_cubes, double *d_pow, int n_frames, int V, int S, int C,
                               const int *h_ants, int n_ants) {
    MMW_REQUIRE(ctx && d_cubes && d_pow, "null argument");
    MMW_REQUIRE(n_frames >= 0 && V > 0 && S > 0 && C > 0, "bad shape");
    AntList ants;
    MMW_TRY(fill_power_list(h_ants, n_ants, V, &ants));
    if (n_frames == 0) return MMW_OK;
    ProfScope ps(ctx, "rd_pow64");
    // batches only, as the one-antenna kernel; MMW_POW64_FUSED=0: the per-antenna route on every shape
    if (rd_mag64_fused_ok(S, C) && n_frames >= 8 && opt_int(ctx, "MMW_POW64_FUSED", 1))
        return launch_rd_pow64_fused(ctx, d_cubes, d_pow, n_frames, V, ants);
    return rd_pow64_per_antenna(ctx, d_cubes, d_pow, n_frames, V, S, C, ants);
}

}  // namespace

extern "C" {

int mmw_range_doppler_power64(mmw_ctx *ctx, const void *d_cubes, double *d_pow, int n_frames, int V, int S, int C,
                              const int *h_ants, int n_ants) {
    MMW_REQUIRE(ctx, "ctx is null");
    MMW_JOIN(ctx);
    return range_doppler_power64_impl(ctx, d_cubes, d_pow, n_frames, V, S, C, h_ants, n_ants);
}

// mmw_detect_batch with the antenna-integrated power plane in the place of antenna 0's |RD|
int mmw_detect_batch_integrated(mmw_ctx *ctx, const void *d_cubes, void *d_rd, double *d_pow, uint8_t *d_mask, int32_t *d_dets,
                                int32_t *d_counts, float *d_l1, int n_frames, int V, int S, int C, int cfar_kind, int train_r,
                                int train_d, int guard_r, int guard_d, double scale, int k_rank, int cap, const int *h_ants,
                                int n_ants) {
    MMW_REQUIRE(ctx && d_cubes && d_rd && d_pow && d_mask && d_dets && d_counts, "null argument");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_frames >= 0 && n_frames <= 65535 && V > 0 && S > 0 && C > 0 && cap >= 0, "bad shape");
    AntList ants;
    MMW_TRY(fill_power_list(h_ants, n_ants, V, &ants));       // (before the first launch: a refused list leaves every output untouched)
    if (n_frames == 0) return MMW_OK;
    MMW_TRY(range_doppler_impl(ctx, d_cubes, d_rd, nullptr, n_frames, V, S, C, RawView{1, 0}, d_l1));
    MMW_TRY(range_doppler_power64_impl(ctx, d_cubes, d_pow, n_frames, V, S, C, h_ants, n_ants));
    MMW_TRY(cfar2d_impl(ctx, d_pow, nullptr, nullptr, d_mask, n_frames, S, C, cfar_kind, train_r, train_d, guard_r, guard_d, scale,
                        k_rank));
    return compact2d_impl(ctx, d_mask, d_dets, d_counts, n_frames, S, C, cap);
}

}  // extern "C"
