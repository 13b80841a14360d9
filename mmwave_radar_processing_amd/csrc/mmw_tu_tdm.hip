// Translation unit of the TDM-MIMO Doppler phase compensation (mmw_tdm.h): mmw_angle_argmax_tdm, mmw_angle_argmax_cells64_tdm
// and the host twin of the float64 stage, mmw_diag_angle_argmax_tdm_host.
#include "mmw_entry.h"
// mmw_argmax.h (for its device helpers and ArgmaxRefine) also DEFINES the non-template kernels of mmw_tu_points.hip; a second
// definition with external linkage would collide at link time, so this unit's unused copies get names of their own.
#define k_argmax64_cells k_argmax64_cells_in_tu_tdm
#define k_argmax_refine_part k_argmax_refine_part_in_tu_tdm
#define k_argmax_refine_finish k_argmax_refine_finish_in_tu_tdm
#define k_refine_cells_sum k_refine_cells_sum_in_tu_tdm
#define k_argmax_refine_whole k_argmax_refine_whole_in_tu_tdm
#include "mmw_tdm.h"
#undef k_argmax64_cells
#undef k_argmax_refine_part
#undef k_argmax_refine_finish
#undef k_refine_cells_sum
#undef k_argmax_refine_whole

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
            return set_error(MMW_ERR_NOMEM, "hipMalloc(%zu) for the compensated argmax failed", bytes);
        }
        return MMW_OK;
    }
};

size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// the list rules of mmw_angle_argmax_exact
int fill_tdm_list(const int *h_ant, int n_ant, int V, int A, AntList *ants) {
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

// rows of the [n_ant][C] complex128 table that are the same bit for bit share one float32 row (one per transmit slot)
TdmRows dedupe_rows(const double *h_phase, int n_ant, int C, std::vector<float> *ph32) {
    TdmRows rows{};
    int first[MAX_ANT];
    const size_t row_bytes = (size_t)C * 2 * sizeof(double);
    for (int i = 0; i < n_ant; ++i) {
        int r = -1;
        for (int j = 0; j < rows.n_rows && r < 0; ++j)
            if (std::memcmp(h_phase + (size_t)i * C * 2, h_phase + (size_t)first[j] * C * 2, row_bytes) == 0) r = j;
        if (r < 0) {
            r = rows.n_rows++;
            first[r] = i;
            for (int c = 0; c < 2 * C; ++c) ph32->push_back((float)h_phase[(size_t)i * C * 2 + c]);
        }
        rows.row[i] = (unsigned char)r;
    }
    return rows;
}

template <int NA>
void launch_argmax_tdm(mmw_ctx *ctx, dim3 grid, size_t lds, const float2 *rd, const int32_t *dets, const int32_t *counts, int32_t *idx,
                       int V, int S, int C, int cap, const AntList &ants, int A, int shift, const float2 *twA, const float2 *ph32,
                       const TdmRows &rows, const ArgmaxRefine &rf, float k_tdm) {
    hipLaunchKernelGGL(k_argmax_tdm<NA>, grid, dim3(256), lds, ctx->stream, rd, dets, counts, idx, V, S, C, cap, ants, A, shift, twA,
                       ph32, rows, rf, k_tdm);
}

}  // namespace

extern "C" {

int mmw_angle_argmax_tdm(mmw_ctx *ctx, const void *d_cubes, const float *d_l1, const void *d_rd, const int32_t *d_dets,
                         const int32_t *d_counts, int32_t *d_idx, int n_frames, int V, int S, int C, int cap, const int *h_ant,
                         int n_ant, int A, int shift, const double *h_phase, int *h_n_refined) {
    MMW_REQUIRE(ctx && d_cubes && d_l1 && d_rd && d_dets && d_counts && d_idx && h_phase, "null argument");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_frames >= 0 && n_frames <= 65535 && V > 0 && S > 0 && S <= 65535 && C > 0 && cap >= 0 && A > 0, "bad shape");
    MMW_REQUIRE((long)n_frames * cap < (1L << 31), "too many detection slots for one call");
    AntList ants{};
    MMW_TRY(fill_tdm_list(h_ant, n_ant, V, A, &ants));
    if (h_n_refined) *h_n_refined = 0;
    if (n_frames == 0 || cap == 0) return MMW_OK;
    std::vector<float> ph32;
    const TdmRows rows = dedupe_rows(h_phase, n_ant, C, &ph32);
    // One shared row is a phase common to every antenna of the list: it cannot move a magnitude, and the uncompensated entry
    // answers (bit for bit what it answers without the table, as the contract of single-slot lists demands).
    if (rows.n_rows == 1)
        return mmw_angle_argmax_exact(ctx, d_cubes, d_l1, d_rd, d_dets, d_counts, d_idx, n_frames, V, S, C, cap, h_ant, n_ant, A, shift,
                                      h_n_refined);
    const size_t lds = tdm_lds(A, rows.n_rows, C);
    if (lds > 48 * 1024)
        return set_error(MMW_ERR_UNSUPPORTED, "mmw_angle_argmax_tdm: %d angle bins + %d phase rows of %d columns exceed 48 KiB of LDS", A,
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
        ProfScope ps(ctx, "argmax_tdm");
        const dim3 grid((unsigned)((cap + 255) / 256), (unsigned)n_frames);
#define MMW_TDM(NA) \
    launch_argmax_tdm<NA>(ctx, grid, lds, (const float2 *)d_rd, d_dets, d_counts, d_idx, V, S, C, cap, ants, A, shift, (const float2 *)twA, \
                          d_ph32, rows, rf, TDM_PRODUCT_ULPS * eps)
        if (n_ant <= 4) MMW_TDM(4);
        else if (n_ant <= 8) MMW_TDM(8);
        else if (n_ant <= 16) MMW_TDM(16);
        else MMW_TDM(32);
#undef MMW_TDM
        MMW_TRY(check_launch("argmax_tdm"));
    }
    MMW_HIP(hipMemcpyAsync(&n_flag, d_nflag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    MMW_HIP(hipStreamSynchronize(ctx->stream));             // (also: ph32 may leave scope)
    n_flag = std::min(n_flag, list_cap);
    if (h_n_refined) *h_n_refined = n_flag;
    if (n_flag <= 0) return MMW_OK;

    // ---- float64 re-evaluation of the undecided detections: per-frame lists of them, their complex128 cells from the direct
    // route of mmw_rd_cells64_at, the float64 stage
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
    const size_t b_cnt = up256((size_t)n_frames * 4), b_slot = up256(rows2 * 4), b_dets = up256(rows2 * 8),
                 b_cells = up256(rows2 * n_ant * sizeof(cplx<double>)), b_ph = up256((size_t)n_ant * C * 16);
    DevBlock blk;
    MMW_TRY(blk.alloc(b_cnt + b_slot + b_dets + b_cells + b_ph));
    char *base = (char *)blk.p;
    int32_t *d_cnt2 = (int32_t *)base, *d_slot2 = (int32_t *)(base + b_cnt), *d_dets2 = (int32_t *)(base + b_cnt + b_slot);
    double *d_cells = (double *)(base + b_cnt + b_slot + b_dets), *d_ph64 = (double *)(base + b_cnt + b_slot + b_dets + b_cells);
    MMW_HIP(hipMemcpyAsync(d_cnt2, counts2.data(), (size_t)n_frames * 4, hipMemcpyHostToDevice, ctx->stream));
    MMW_HIP(hipMemcpyAsync(d_slot2, slot2.data(), rows2 * 4, hipMemcpyHostToDevice, ctx->stream));
    MMW_HIP(hipMemcpyAsync(d_ph64, h_phase, (size_t)n_ant * C * 16, hipMemcpyHostToDevice, ctx->stream));
    MMW_HIP(hipMemsetAsync(d_dets2, 0, rows2 * 8, ctx->stream));
    hipLaunchKernelGGL(k_tdm_gather_dets, dim3((unsigned)((rows2 + 255) / 256)), dim3(256), 0, ctx->stream, d_dets, d_slot2, d_dets2, (int)rows2);
    int rc = check_launch("tdm_gather_dets");
    if (rc == MMW_OK) {
        int idx[MAX_ANT];
        for (int i = 0; i < n_ant; ++i) idx[i] = ants.idx[i];
        rc = mmw_rd_cells64_at(ctx, d_cubes, d_dets2, d_cnt2, d_cells, n_frames, V, S, C, cap2, idx, n_ant, MMW_CELLS64_DIRECT);
    }
    const void *twA64 = nullptr;
    if (rc == MMW_OK) rc = get_table<double>(ctx, TAB_TWIDDLE, A, &twA64);
    if (rc == MMW_OK) {
        ProfScope ps(ctx, "argmax_tdm64");
        hipLaunchKernelGGL(k_argmax64_cells_tdm, dim3((unsigned)((rows2 + 3) / 4)), dim3(256), 0, ctx->stream, d_cells, d_dets2 + 1, 2, d_ph64,
                           d_slot2, d_cnt2, cap2, d_idx, (long)rows2, n_ant, C, A, shift, (const double *)twA64);
        rc = check_launch("argmax64_cells_tdm");
    }
    const hipError_t e = hipStreamSynchronize(ctx->stream);  // (in any case: the block and the host vectors leave scope)
    MMW_TRY(rc);
    MMW_HIP(e);
    return MMW_OK;
}

int mmw_angle_argmax_cells64_tdm(mmw_ctx *ctx, const void *d_cells, const int32_t *d_cols, const double *h_phase, int32_t *d_idx,
                                 int n_rows, int n_ant, int C, int A, int shift) {
    MMW_REQUIRE(ctx && d_cells && d_cols && h_phase && d_idx, "null argument");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_rows >= 0 && n_ant >= 1 && n_ant <= MAX_ANT && A >= n_ant && C > 0, "bad shape (need 1 <= n_ant <= min(A, %d), C > 0)",
                MAX_ANT);
    if (n_rows == 0) return MMW_OK;
    const void *twA64;
    MMW_TRY(get_table<double>(ctx, TAB_TWIDDLE, A, &twA64));
    DevBlock blk;
    MMW_TRY(blk.alloc((size_t)n_ant * C * 16));
    MMW_HIP(hipMemcpyAsync(blk.p, h_phase, (size_t)n_ant * C * 16, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_argmax64_cells_tdm, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, ctx->stream, (const double *)d_cells, d_cols, 1,
                       (const double *)blk.p, (const int32_t *)nullptr, (const int32_t *)nullptr, 1, d_idx, (long)n_rows, n_ant, C, A, shift,
                       (const double *)twA64);
    const int rc = check_launch("argmax64_cells_tdm");
    const hipError_t e = hipStreamSynchronize(ctx->stream);  // (the table's block leaves scope)
    MMW_TRY(rc);
    MMW_HIP(e);
    return MMW_OK;
}

// The float64 stage on the host: the functions the kernel calls, the twiddles get_table uploads.  No device is touched.
int mmw_diag_angle_argmax_tdm_host(const void *h_cells, const int32_t *h_cols, const double *h_phase, int32_t *h_idx, int n_rows,
                                   int n_ant, int C, int A, int shift) {
    MMW_REQUIRE(h_cells && h_cols && h_phase && h_idx, "null argument");
    MMW_REQUIRE(n_rows >= 0 && n_ant >= 1 && n_ant <= MAX_ANT && A >= n_ant && C > 0, "bad shape (need 1 <= n_ant <= min(A, %d), C > 0)",
                MAX_ANT);
    const std::vector<double> tw = make_table<double>(TAB_TWIDDLE, A);
    const double *cells = (const double *)h_cells;
    for (long row = 0; row < n_rows; ++row) {
        int c = h_cols[row];
        c = c < 0 ? 0 : (c >= C ? C - 1 : c);               // (as the kernel)
        double y[2 * MAX_ANT], best;
        for (int i = 0; i < n_ant; ++i) tdm_compensate(cells + 2 * (row * n_ant + i), h_phase + 2 * ((long)i * C + c), y + 2 * i);
        int idx;
        tdm_argmax64_bins(y, n_ant, A, shift, tw.data(), 0, 1, &best, &idx);
        h_idx[row] = idx;
    }
    return MMW_OK;
}

}  // extern "C"
