// Translation unit of the TDM-MIMO velocity unwrapping (mmw_tdm_hyp.h): mmw_angle_argmax_tdm_hyp, mmw_angle_argmax_cells64_tdm_hyp,
// the host twin of the float64 stage mmw_diag_angle_argmax_tdm_hyp_host, and mmw_tdm_unwrap_velocity.
#include "mmw_entry.h"
// mmw_argmax.h and mmw_tdm.h also DEFINE the non-template kernels of mmw_tu_points.hip and mmw_tu_tdm.hip; a second definition with
// external linkage would collide at link time, so this unit's copies get names of their own (k_tdm_gather_dets is launched here
// under its name).
#define k_argmax64_cells k_argmax64_cells_in_tu_tdm_hyp
#define k_argmax_refine_part k_argmax_refine_part_in_tu_tdm_hyp
#define k_argmax_refine_finish k_argmax_refine_finish_in_tu_tdm_hyp
#define k_refine_cells_sum k_refine_cells_sum_in_tu_tdm_hyp
#define k_argmax_refine_whole k_argmax_refine_whole_in_tu_tdm_hyp
#define k_tdm_gather_dets k_tdm_gather_dets_in_tu_tdm_hyp
#define k_argmax64_cells_tdm k_argmax64_cells_tdm_in_tu_tdm_hyp
#include "mmw_tdm_hyp.h"
#undef k_argmax64_cells
#undef k_argmax_refine_part
#undef k_argmax_refine_finish
#undef k_refine_cells_sum
#undef k_argmax_refine_whole
#undef k_tdm_gather_dets
#undef k_argmax64_cells_tdm

#include <algorithm>

using namespace mmw;

namespace {

// a device allocation of one call (the scratch of the context belongs to the entries this unit calls)
struct DevBlock {
    void *p = nullptr;
    DevBlock() = default;
    DevBlock(const DevBlock &) = delete;
    DevBlock &operator=(const DevBlock &) = delete;
    ~DevBlock() {
        if (p) (void)hipFree(p);
    }
    int alloc(size_t bytes) {
        if (hipMalloc(&p, std::max<size_t>(bytes, 256)) != hipSuccess) {
            p = nullptr;
            return set_error(MMW_ERR_NOMEM, "hipMalloc(%zu) for the hypothesis argmax failed", bytes);
        }
        return MMW_OK;
    }
};

size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// the list rules of mmw_angle_argmax_exact
int fill_hyp_list(const int *h_ant, int n_ant, int V, int A, AntList *ants) {
    MMW_REQUIRE(n_ant >= 1 && n_ant <= MAX_ANT && n_ant <= A && h_ant, "antenna list must have 1..%d entries (<= A)", MAX_ANT);
    ants->n = n_ant;
    for (int i = 0; i < n_ant; ++i) {
        int a = h_ant[i];
        if (a < 0) a += V;
        MMW_REQUIRE(a >= 0 && a < V, "antenna index %d out of range", h_ant[i]);
        ants->idx[i] = a;
    }
    return MMW_OK;
}

template <int NA>
void launch_argmax_tdm_hyp(mmw_ctx *ctx, dim3 grid, size_t lds, const float2 *rd, const int32_t *dets, const int32_t *counts, int32_t *idx,
                           int32_t *hyp, int hyp_given, int V, int S, int C, int cap, const AntList &ants, int A, int shift,
                           const float2 *twA, const float2 *ph32, const TdmHypRows &rows, const ArgmaxRefine &rf, float k_tdm) {
    hipLaunchKernelGGL(k_argmax_tdm_hyp<NA>, grid, dim3(256), lds, ctx->stream, rd, dets, counts, idx, hyp, hyp_given, V, S, C, cap, ants, A,
                       shift, twA, ph32, rows, rf, k_tdm);
}

}  // namespace

extern "C" {

int mmw_angle_argmax_tdm_hyp(mmw_ctx *ctx, const void *d_cubes, const float *d_l1, const void *d_rd, const int32_t *d_dets,
                             const int32_t *d_counts, int32_t *d_idx, int32_t *d_hyp, int hyp_given, int n_frames, int V, int S, int C,
                             int cap, const int *h_ant, int n_ant, int A, int shift, const double *h_phase, int H, int *h_n_refined) {
    MMW_REQUIRE(ctx && d_cubes && d_l1 && d_rd && d_dets && d_counts && d_idx && d_hyp && h_phase, "null argument");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_frames >= 0 && n_frames <= 65535 && V > 0 && S > 0 && S <= 65535 && C > 0 && cap >= 0 && A > 0, "bad shape");
    MMW_REQUIRE((long)n_frames * cap < (1L << 31), "too many detection slots for one call");
    MMW_REQUIRE(H >= 1 && H <= TDM_MAX_HYP, "%d hypotheses: need 1..%d", H, TDM_MAX_HYP);
    AntList ants{};
    MMW_TRY(fill_hyp_list(h_ant, n_ant, V, A, &ants));
    if (h_n_refined) *h_n_refined = 0;
    if (n_frames == 0 || cap == 0) return MMW_OK;
    std::vector<float> ph32;
    const TdmHypRows rows = tdm_hyp_plan(h_phase, H, n_ant, C, &ph32);
    const dim3 grid((unsigned)((cap + 255) / 256), (unsigned)n_frames);
    // One distinct hypothesis: there is nothing to choose, and the compensated entry answers with table 0 (bit for bit what it
    // answers without the other tables; for a single-slot list that is mmw_angle_argmax_exact).
    if (rows.n_hyp == 1) {
        MMW_TRY(mmw_angle_argmax_tdm(ctx, d_cubes, d_l1, d_rd, d_dets, d_counts, d_idx, n_frames, V, S, C, cap, h_ant, n_ant, A, shift, h_phase,
                                     h_n_refined));
        if (hyp_given) return MMW_OK;
        hipLaunchKernelGGL(k_tdm_hyp_fill, grid, dim3(256), 0, ctx->stream, d_counts, d_hyp, cap);
        return check_launch("tdm_hyp_fill");
    }
    const size_t lds = tdm_lds(A, rows.n_rows, C);
    if (lds > 48 * 1024)
        return set_error(MMW_ERR_UNSUPPORTED, "mmw_angle_argmax_tdm_hyp: %d angle bins + %d phase rows of %d columns exceed 48 KiB of LDS", A,
                         rows.n_rows, C);
    const void *twA = nullptr;
    MMW_TRY(get_table<float>(ctx, TAB_TWIDDLE, A, &twA));
    // scratch of the context: count | list of undecided detections | float32 phasor rows (all read back or done with before
    // the float64 cells, which own the scratch after that)
    const int list_cap = n_frames * cap;
    const size_t list_bytes = up256(256 + (size_t)list_cap * sizeof(int));
    MMW_TRY(ensure_scratch(ctx, list_bytes + up256(ph32.size() * sizeof(float))));
    int *d_nflag = (int *)ctx->scratch, *d_list = (int *)((char *)ctx->scratch + 256);
    float2 *d_ph32 = (float2 *)((char *)ctx->scratch + list_bytes);
    MMW_HIP(hipMemsetAsync(d_nflag, 0, 256, ctx->stream));
    MMW_HIP(hipMemcpyAsync(d_ph32, ph32.data(), ph32.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    const float eps = 5.9604645e-8f;
    ArgmaxRefine rf{};
    rf.l1 = d_l1, rf.n_flag = d_nflag, rf.list = d_list, rf.list_cap = list_cap;
    rf.k_fft = (float)rd_error_ulps(S, C) * eps, rf.k_ang = 4.f * (float)(n_ant + 4) * eps;
    int n_flag = 0;
    {
        ProfScope ps(ctx, "argmax_tdm_hyp");
#define MMW_TDM_HYP(NA) \
    launch_argmax_tdm_hyp<NA>(ctx, grid, lds, (const float2 *)d_rd, d_dets, d_counts, d_idx, d_hyp, hyp_given ? 1 : 0, V, S, C, cap, ants, A, \
                              shift, (const float2 *)twA, d_ph32, rows, rf, TDM_PRODUCT_ULPS * eps)
        if (n_ant <= 4) MMW_TDM_HYP(4);
        else if (n_ant <= 8) MMW_TDM_HYP(8);
        else if (n_ant <= 16) MMW_TDM_HYP(16);
        else MMW_TDM_HYP(32);
#undef MMW_TDM_HYP
        MMW_TRY(check_launch("argmax_tdm_hyp"));
    }
    MMW_HIP(hipMemcpyAsync(&n_flag, d_nflag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    MMW_HIP(hipStreamSynchronize(ctx->stream));             // (also: ph32 may leave scope)
    n_flag = std::min(n_flag, list_cap);
    if (h_n_refined) *h_n_refined = n_flag;
    if (n_flag <= 0) return MMW_OK;

    // ---- float64 re-evaluation of the undecided detections, by the route of mmw_angle_argmax_tdm: per-frame lists of them,
    // their complex128 cells from the direct route of mmw_rd_cells64_at, the float64 stage over the distinct hypotheses
    std::vector<int> list((size_t)n_flag);
    MMW_HIP(hipMemcpy(list.data(), d_list, list.size() * sizeof(int), hipMemcpyDeviceToHost));
    std::sort(list.begin(), list.end());
    std::vector<int32_t> counts2((size_t)n_frames, 0);
    for (int s : list) {
        MMW_REQUIRE(s >= 0 && s < list_cap, "undecided list holds slot %d outside [0, %d)", s, list_cap);
        ++counts2[(size_t)(s / cap)];
    }
    const int cap2 = *std::max_element(counts2.begin(), counts2.end());
    const size_t rows2 = (size_t)n_frames * cap2;
    MMW_REQUIRE(rows2 < ((size_t)1 << 31), "too many undecided detection slots for one call");
    std::vector<int32_t> slot2(rows2, -1), fill((size_t)n_frames, 0);
    for (int s : list) {
        const int f = s / cap;
        slot2[(size_t)f * cap2 + fill[(size_t)f]++] = s;
    }
    const size_t ph_bytes = (size_t)H * n_ant * C * 16;
    const size_t b_cnt = up256((size_t)n_frames * 4), b_slot = up256(rows2 * 4), b_dets = up256(rows2 * 8),
                 b_cells = up256(rows2 * n_ant * sizeof(cplx<double>)), b_ph = up256(ph_bytes);
    DevBlock blk;
    MMW_TRY(blk.alloc(b_cnt + b_slot + b_dets + b_cells + b_ph));
    char *base = (char *)blk.p;
    int32_t *d_cnt2 = (int32_t *)base, *d_slot2 = (int32_t *)(base + b_cnt), *d_dets2 = (int32_t *)(base + b_cnt + b_slot);
    double *d_cells = (double *)(base + b_cnt + b_slot + b_dets), *d_ph64 = (double *)(base + b_cnt + b_slot + b_dets + b_cells);
    MMW_HIP(hipMemcpyAsync(d_cnt2, counts2.data(), (size_t)n_frames * 4, hipMemcpyHostToDevice, ctx->stream));
    MMW_HIP(hipMemcpyAsync(d_slot2, slot2.data(), rows2 * 4, hipMemcpyHostToDevice, ctx->stream));
    MMW_HIP(hipMemcpyAsync(d_ph64, h_phase, ph_bytes, hipMemcpyHostToDevice, ctx->stream));
    MMW_HIP(hipMemsetAsync(d_dets2, 0, rows2 * 8, ctx->stream));
    hipLaunchKernelGGL(k_tdm_gather_dets_in_tu_tdm_hyp, dim3((unsigned)((rows2 + 255) / 256)), dim3(256), 0, ctx->stream, d_dets, d_slot2,
                       d_dets2, (int)rows2);
    int rc = check_launch("tdm_gather_dets");
    if (rc == MMW_OK) {
        int idx[MAX_ANT];
        for (int i = 0; i < n_ant; ++i) idx[i] = ants.idx[i];
        rc = mmw_rd_cells64_at(ctx, d_cubes, d_dets2, d_cnt2, d_cells, n_frames, V, S, C, cap2, idx, n_ant, MMW_CELLS64_DIRECT);
    }
    const void *twA64 = nullptr;
    if (rc == MMW_OK) rc = get_table<double>(ctx, TAB_TWIDDLE, A, &twA64);
    if (rc == MMW_OK) {
        ProfScope ps(ctx, "argmax_tdm_hyp64");
        hipLaunchKernelGGL(k_argmax64_cells_tdm_hyp, dim3((unsigned)((rows2 + 3) / 4)), dim3(256), 0, ctx->stream, d_cells, d_dets2 + 1, 2, d_ph64,
                           rows, d_slot2, d_cnt2, cap2, d_idx, d_hyp, hyp_given ? 1 : 0, (long)rows2, n_ant, C, A, shift, (const double *)twA64);
        rc = check_launch("argmax64_cells_tdm_hyp");
    }
    const hipError_t e = hipStreamSynchronize(ctx->stream);  // (in any case: the block and the host vectors leave scope)
    MMW_TRY(rc);
    MMW_HIP(e);
    return MMW_OK;
}

int mmw_angle_argmax_cells64_tdm_hyp(mmw_ctx *ctx, const void *d_cells, const int32_t *d_cols, const double *h_phase, int H, int32_t *d_idx,
                                     int32_t *d_hyp, int hyp_given, int n_rows, int n_ant, int C, int A, int shift) {
    MMW_REQUIRE(ctx && d_cells && d_cols && h_phase && d_idx && d_hyp, "null argument");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_rows >= 0 && n_ant >= 1 && n_ant <= MAX_ANT && A >= n_ant && C > 0, "bad shape (need 1 <= n_ant <= min(A, %d), C > 0)",
                MAX_ANT);
    MMW_REQUIRE(H >= 1 && H <= TDM_MAX_HYP, "%d hypotheses: need 1..%d", H, TDM_MAX_HYP);
    if (n_rows == 0) return MMW_OK;
    const TdmHypRows rows = tdm_hyp_plan(h_phase, H, n_ant, C, nullptr);
    const void *twA64;
    MMW_TRY(get_table<double>(ctx, TAB_TWIDDLE, A, &twA64));
    const size_t ph_bytes = (size_t)H * n_ant * C * 16;
    DevBlock blk;
    MMW_TRY(blk.alloc(ph_bytes));
    MMW_HIP(hipMemcpyAsync(blk.p, h_phase, ph_bytes, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_argmax64_cells_tdm_hyp, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, ctx->stream, (const double *)d_cells, d_cols,
                       1, (const double *)blk.p, rows, (const int32_t *)nullptr, (const int32_t *)nullptr, 1, d_idx, d_hyp, hyp_given ? 1 : 0,
                       (long)n_rows, n_ant, C, A, shift, (const double *)twA64);
    const int rc = check_launch("argmax64_cells_tdm_hyp");
    const hipError_t e = hipStreamSynchronize(ctx->stream);  // (the table's block leaves scope)
    MMW_TRY(rc);
    MMW_HIP(e);
    return MMW_OK;
}

// The float64 stage on the host: the functions the kernel calls, the twiddles get_table uploads.  No device is touched.
int mmw_diag_angle_argmax_tdm_hyp_host(const void *h_cells, const int32_t *h_cols, const double *h_phase, int H, int32_t *h_idx,
                                       int32_t *h_hyp, int hyp_given, int n_rows, int n_ant, int C, int A, int shift) {
    MMW_REQUIRE(h_cells && h_cols && h_phase && h_idx && h_hyp, "null argument");
    MMW_REQUIRE(n_rows >= 0 && n_ant >= 1 && n_ant <= MAX_ANT && A >= n_ant && C > 0, "bad shape (need 1 <= n_ant <= min(A, %d), C > 0)",
                MAX_ANT);
    MMW_REQUIRE(H >= 1 && H <= TDM_MAX_HYP, "%d hypotheses: need 1..%d", H, TDM_MAX_HYP);
    const TdmHypRows rows = tdm_hyp_plan(h_phase, H, n_ant, C, nullptr);
    const std::vector<double> tw = make_table<double>(TAB_TWIDDLE, A);
    const double *cells = (const double *)h_cells;
    for (long row = 0; row < n_rows; ++row) {
        int c = h_cols[row];
        c = c < 0 ? 0 : (c >= C ? C - 1 : c);               // (as the kernel)
        int d_lo = 0, d_hi = rows.n_hyp;
        if (hyp_given) {
            int h = h_hyp[row];
            h = h < 0 ? 0 : (h >= H ? H - 1 : h);
            d_lo = rows.map[h];
            d_hi = d_lo + 1;
        }
        int idx, d;
        tdm_hyp_row64_host(cells + 2 * row * n_ant, h_phase, rows, d_lo, d_hi, c, n_ant, C, A, shift, tw.data(), &idx, &d);
        h_idx[row] = idx;
        if (!hyp_given) h_hyp[row] = rows.orig[d];
    }
    return MMW_OK;
}

int mmw_tdm_unwrap_velocity(mmw_ctx *ctx, double *d_points, const int32_t *d_dets, const int32_t *d_counts, const int32_t *d_hyp,
                            int n_frames, int cap, int C, int n_slots, double span) {
    MMW_REQUIRE(ctx && d_points && d_dets && d_counts && d_hyp, "null argument");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_frames >= 0 && n_frames <= 65535 && cap >= 0 && C > 0, "bad shape");
    MMW_REQUIRE((long)n_frames * cap < (1L << 31), "too many detection slots for one call");
    MMW_REQUIRE(n_slots >= 1 && n_slots <= TDM_MAX_HYP, "%d transmit slots: need 1..%d", n_slots, TDM_MAX_HYP);
    if (n_frames == 0 || cap == 0) return MMW_OK;
    ProfScope ps(ctx, "tdm_unwrap");
    hipLaunchKernelGGL(k_tdm_unwrap_velocity, dim3((unsigned)((cap + 255) / 256), (unsigned)n_frames), dim3(256), 0, ctx->stream, d_points,
                       d_dets, d_counts, d_hyp, cap, C, n_slots, span);
    return check_launch("tdm_unwrap_velocity");
}

}  // extern "C"
