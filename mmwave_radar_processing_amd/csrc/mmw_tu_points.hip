// Translation unit of the point cloud: the per-detection angle argmax with its float64 refinement (mmw_argmax.h), the dense float64
// cells (mmw_cells64.h) and mmw_detect_points (mmw_detect.h).
#include "mmw_entry.h"
#include "mmw_launch.h"
#include "mmw_argmax.h"
#include "mmw_detect.h"
#include "mmw_cells64.h"

#include <algorithm>

using namespace mmw;

// ------------------------------------------------------------------ float64 |range-Doppler| of 256 x 128 planes (range_doppler_mag64_impl)
bool mmw::rd_mag64_fused_ok(int S, int C) { return S == R64_S && C == R64_C; }

// one launch, the complex128 intermediate in per-workgroup scratch that never leaves the caches (mmw_cells64.h); a whole
// frame per workgroup
int mmw::launch_rd_mag64_fused(mmw_ctx *ctx, const void *d_cubes, double *d_mag, int n_frames, int V, int rx_idx) {
    constexpr int S = R64_S, C = R64_C;
    const int grid = std::min(n_frames, ctx->num_cu);
    MMW_TRY(ensure_scratch(ctx, (size_t)grid * S * C * sizeof(cplx<double>)));
    Rd64Args ra{};
    ra.cubes = (const float2 *)d_cubes + (long)rx_idx * S * C;
    ra.frame_stride = (long)V * S * C;
    ra.mag = d_mag;
    ra.scratch = (cplx<double> *)ctx->scratch;
    ra.n_frames = n_frames;
    const void *p;
    MMW_TRY(get_table<double>(ctx, TAB_HANN, S, &p));
    ra.ws = (const double *)p;
    MMW_TRY(get_table<double>(ctx, TAB_HANN, C, &p));
    ra.wc = (const double *)p;
    MMW_TRY(get_table<double>(ctx, TAB_TWIDDLE, S, &p));
    ra.twS = (const cplx<double> *)p;
    MMW_TRY(get_table<double>(ctx, TAB_TWIDDLE, C, &p));
    ra.twC = (const cplx<double> *)p;
    const size_t lds = rd64_lds();
    MMW_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_rd_mag64_256x128), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_rd_mag64_256x128, dim3((unsigned)grid), dim3(C64_NT), lds, ctx->stream, ra);
    return check_launch("rd_mag64_256x128");
}

// ------------------------------------------------------------------ point cloud
static int fill_ant_list(const int *h_ant, int n_ant, int V, int A, AntList *ants) {
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

static void launch_angle_argmax(mmw_ctx *ctx, dim3 grid, const float2 *rd, const int32_t *dets, const int32_t *counts,
                                int32_t *idx, int V, int S, int C, int cap, const AntList &ants, int A, int shift,
                                const float2 *twA, const ArgmaxRefine &rf) {
#define MMW_ARGMAX(NA) \
    hipLaunchKernelGGL(k_angle_argmax<NA>, grid, dim3(256), 0, ctx->stream, rd, dets, counts, idx, V, S, C, cap, ants, A, shift, twA, rf)
    // lists of up to 8 antennas with the error bound: the lane-resident routine of the fused detection stage
    if (rf.l1 && ants.n <= DET_LATE_MAX_ANT && A == 64 && opt_int(ctx, "MMW_ARGMAX_FORM", 1) == 1) {
        // one lane per detection (64 bins as register FFTs): 256 detections of a frame per workgroup and pass
        const dim3 g2((unsigned)std::min((cap + 255) / 256, 4), grid.y);
#define MMW_ARGMAX_DETS(NA, SH) \
    hipLaunchKernelGGL((k_angle_argmax_dets<NA, SH>), g2, dim3(256), 0, ctx->stream, rd, dets, counts, idx, V, S, C, cap, ants, twA, rf)
        if (ants.n <= 4) {
            if (shift) MMW_ARGMAX_DETS(4, true); else MMW_ARGMAX_DETS(4, false);
        } else if (ants.n <= 8) {
            if (shift) MMW_ARGMAX_DETS(8, true); else MMW_ARGMAX_DETS(8, false);
        } else {
            if (shift) MMW_ARGMAX_DETS(16, true); else MMW_ARGMAX_DETS(16, false);
        }
#undef MMW_ARGMAX_DETS
        return;
    }
    if (rf.l1 && ants.n <= DET_MAX_ANT && A <= 1024) {
        if (ants.n <= 4)
            hipLaunchKernelGGL(k_angle_argmax_lanes<4>, grid, dim3(256), (size_t)A * 8, ctx->stream, rd, dets, counts, idx, V, S, C, cap, ants, A,
                               shift, twA, rf);
        else
            hipLaunchKernelGGL(k_angle_argmax_lanes<DET_MAX_ANT>, grid, dim3(256), (size_t)A * 8, ctx->stream, rd, dets, counts, idx, V, S, C,
                               cap, ants, A, shift, twA, rf);
        return;
    }
    if (ants.n <= 4) MMW_ARGMAX(4);
    else if (ants.n <= 8) MMW_ARGMAX(8);
    else if (ants.n <= 16) MMW_ARGMAX(16);
    else MMW_ARGMAX(32);
#undef MMW_ARGMAX
}

// The launch of k_argmax_refine_part, shared by the refinement and by the read-out of its slices (mmw_rd_cells64_at): `units`
// workgroups per slice walk the entries of the list.
static int launch_refine_part(mmw_ctx *ctx, const RefineArgs &ra, int units) {
    const size_t lds = refine_tabs_lds(ra.S, ra.C);
    MMW_REQUIRE(lds <= 150 * 1024, "plane %d x %d too large for the refinement tables", ra.S, ra.C);
    if (lds > 48 * 1024)
        MMW_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_argmax_refine_part), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_argmax_refine_part, dim3(ra.parts, units), dim3(256), lds, ctx->stream, ra);
    return check_launch("argmax_refine_part");
}

// float64 re-evaluation of the detections k_angle_argmax flagged (ra.n_flag / ra.list): fixed grids, the flagged count
// stays on the device, workgroups beyond it leave at once.  ra.partial must hold n_split * REFINE_PARTS * ants.n entries.
static int launch_argmax_refine(mmw_ctx *ctx, const RefineArgs &ra) {
    const size_t lds = refine_tabs_lds(ra.S, ra.C);
    MMW_REQUIRE(lds <= 150 * 1024, "plane %d x %d too large for the refinement tables", ra.S, ra.C);
    if (lds > 48 * 1024)
        MMW_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_argmax_refine_whole), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (ra.n_split > 0) {
        MMW_TRY(launch_refine_part(ctx, ra, std::min(ra.n_split, 512)));
        hipLaunchKernelGGL(k_argmax_refine_finish, dim3(std::min((ra.n_split + 3) / 4, ctx->num_cu)), dim3(256), 0, ctx->stream, ra);
        MMW_TRY(check_launch("argmax_refine_finish"));
    }
    if (ra.list_cap > ra.n_split) {
        hipLaunchKernelGGL(k_argmax_refine_whole, dim3(ctx->num_cu), dim3(256), lds, ctx->stream, ra);
        MMW_TRY(check_launch("argmax_refine_whole"));
    }
    return MMW_OK;
}

// Slices per plane sum: a few flagged evaluations per hundred frames are expected, and ~1000 workgroups of the slice
// kernel are resident at once: 16 slices (latency of the single task), fewer and longer ones for very large batches.
static int refine_parts(int n_frames) {
    int p = REFINE_PARTS;
    while (p > 2 && (long)p * n_frames > 60000) p /= 2;
    return p;
}

// what every caller of launch_argmax_refine sets the same way: output buffers, antenna lists, shifts and the dense path are its own
static int fill_refine_args(mmw_ctx *ctx, RefineArgs *ra, const void *d_cubes, const int32_t *d_dets, const int *n_flag, const int *list,
                            int list_cap, int n_split, cplx<double> *partial, int n_frames, int V, int S, int C, int cap, int A) {
    ra->cubes = (const float2 *)d_cubes, ra->dets = d_dets, ra->V = V, ra->cap = cap;
    ra->n_flag = n_flag, ra->list = list, ra->list_cap = list_cap;
    ra->partial = partial, ra->n_split = n_split, ra->parts = refine_parts(n_frames);
    const void *twA64, *twS64, *twC64, *ws64, *wc64;
    MMW_TRY(get_table<double>(ctx, TAB_TWIDDLE, A, &twA64));
    MMW_TRY(get_table<double>(ctx, TAB_TWIDDLE, S, &twS64));
    MMW_TRY(get_table<double>(ctx, TAB_TWIDDLE, C, &twC64));
    MMW_TRY(get_table<double>(ctx, TAB_HANN, S, &ws64));
    MMW_TRY(get_table<double>(ctx, TAB_HANN, C, &wc64));
    ra->S = S;
    ra->C = C;
    ra->A = A;
    ra->ws = (const double *)ws64;
    ra->wc = (const double *)wc64;
    ra->twS = (const cplx<double> *)twS64;
    ra->twC = (const cplx<double> *)twC64;
    ra->twA = (const cplx<double> *)twA64;
    return MMW_OK;
}

// The launch of the dense cell kernel the plan names -- k_cells64<128> (mmw_cells64.h) or k_cells64_mixed<C> (mmw_cells64_mixed.h) --, shared by the
// dense refinement and by the read-out of its cells (mmw_rd_cells64_at): tables from the RefineArgs of the same call, one
// workgroup per (antenna of the list, frame).
static int launch_cells64(mmw_ctx *ctx, const RefineArgs &ra, const int32_t *d_counts, const int *d_flagpos, int dense_min,
                          cplx<double> *d_cells, int n_frames, const Cells64Plan &plan) {
    Cells64Args ca{};
    ca.cubes = ra.cubes;
    ca.dets = ra.dets;
    ca.counts = d_counts;
    ca.flagpos = d_flagpos;
    ca.n_flag = ra.n_flag;
    ca.dense_min = dense_min;
    ca.out = d_cells;
    ca.V = ra.V;
    ca.S = ra.S;
    ca.cap = ra.cap;
    ca.n_ant = ra.ants.n;
    ca.max_cells = plan.cells;
    ca.ants = ra.ants;
    ca.ws = ra.ws;
    ca.wc = ra.wc;
    ca.twS = ra.twS;
    ca.twC = ra.twC;
    if (plan.kind == C64_KIND_MIXED) return launch_cells64_mixed(ctx, ca, ra.C, n_frames, plan.lds);
    MMW_REQUIRE(plan.kind == C64_KIND_128, "no dense float64 cell kernel for %d x %d planes", ra.S, ra.C);
    const size_t lds = cells64_lds(ra.S, ra.C, plan.cells);
    MMW_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_cells64<128>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_cells64<128>, dim3((unsigned)ra.ants.n, (unsigned)n_frames), dim3(C64_NT), lds, ctx->stream, ca);
    return check_launch("cells64");
}

// MMW_ARGMAX_DENSE_MIXED: whether mmw_angle_argmax_exact uses k_cells64_mixed<C> where the plan has it (C != 128).  The default
// is set by measurement (profiles/os_pipeline_np2.json).
constexpr int ARGMAX_DENSE_MIXED_DEFAULT = 0;

// The worst-case bound assumes every rounding error of every partial sum lines up; measured float32 errors stay below
// 1.2 % of it on synthetic frames (tests/argmax_margin.py: 68 000 evaluations on the 256 x 128 and 63 x 100 planes) and
// below 7.5 % of its range-Doppler part on adversarial planes (tests/test_gpu_rd_error_bound.py, profiles/rd_error_bound.json).
//  * mmw_detect_points (CA-CFAR detections: strong cells) uses the FULL worst-case bound with the pairwise form of the test:
//    0.15 % of the evaluations are re-done in float64.
//  * the stand-alone mmw_angle_argmax_exact serves the other detectors.  With the GUI's OS-CFAR parameters (rho 0.7, alpha 2:
//    470 mostly noise-level detections per 256 x 128 frame, flat angle spectra) the full bound sends 12.8 % of the
//    evaluations to float64 -- 120 per frame, each a direct DFT sum over whole planes: 29-36 us/frame against 7.2 with an
//    eighth of the bound (~10x above anything observed on those frames; 1.6 % refined).  Default: the worst case (divisor 1)
//    + the pairwise pass (lists of up to 8 antennas); MMW_ARGMAX_BOUND_DIV=8 selects the eighth again.
static float argmax_bound_div(const mmw_ctx *ctx) { return (float)std::max(1, opt_int(ctx, "MMW_ARGMAX_BOUND_DIV", 1)); }

// ------------------------------------------------------------------ fused detection + point-cloud indices (mmw_detect.h)
// The two queues of the overlapped detection schedule: the range-Doppler producer owns the first rd_cus CU-mask bits, the
// screening consumer the rest (mask bit i belongs to XCD i % 8, and to that XCD's shader engines in turn: multiples of 32
// keep every engine of every XCD equally populated -- an engine with fewer CUs than its neighbours paces the whole launch).
// A new split drains and destroys the whole detection group (a pending tail included); detect_tail makes its two queues again.
static int ensure_det_queues(mmw_ctx *ctx, int rd_cus) {
    if (ctx->det_unavailable) return set_error(MMW_ERR_UNSUPPORTED, "detection queues unavailable on this runtime");
    if (ctx->q_drd && ctx->q_drd_cus == rd_cus) return MMW_OK;
    MMW_HIP(destroy_queues(ctx, Q_DETECT));
    if (!ctx->det_begin) {
        MMW_HIP(hipEventCreateWithFlags(&ctx->det_begin, hipEventDisableTiming));
        MMW_HIP(hipEventCreateWithFlags(&ctx->det_rd_done, hipEventDisableTiming));
        MMW_HIP(hipEventCreateWithFlags(&ctx->det_scr_done, hipEventDisableTiming));
    }
    const hipError_t e = create_split_queues(ctx, rd_cus, {&ctx->q_drd, &ctx->q_dscr});
    if (e != hipSuccess) {
        ctx->det_unavailable = true;
        return set_error(MMW_ERR_UNSUPPORTED, "detection queue creation failed: %s", hipGetErrorString(e));
    }
    ctx->q_drd_cus = rd_cus;
    return MMW_OK;
}

// one launch of a detection screening kernel (serial: one workgroup per frame; overlapped: persistent workgroups) on ctx->stream
template <typename K> static int launch_screen(mmw_ctx *ctx, K kern, int grid, size_t lds, const DetectArgs &a) {
    MMW_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(DET_NT), lds, ctx->stream, a);
    return MMW_OK;
}

namespace {
struct DetectPlan {
    bool ok, ct_window;
    int band_rows, band_pitch, words;
    size_t lds_screen, lds_cell;
};
DetectPlan detect_plan(int S, int C, int kind, int tr, int td, int gr, int gd, int n_az, int n_el, int A = 64) {
    DetectPlan p{};
    const long n = (long)S * C;
    const int hr = tr + gr, hd = td + gd;
    // lists of up to 8 antennas: any angle FFT size; 9 to 16: the late argmax only, i.e. 64 angle bins
    const int n_max = A == 64 ? DET_LATE_MAX_ANT : DET_MAX_ANT;
    if (kind != MMW_CFAR_CA || n_az > n_max || n_el > n_max || n > (1L << 20) || A < 1 || A > 1024) return p;
    p.words = (int)((n + 31) / 32);
    p.lds_cell = cell_exact_lds(S, C, 2 * hr + 1, 2 * hd + 1);
    if (p.lds_cell > 64 * 1024) return p;
    // compile-time windows (with_cfar_window lists them): four rows / columns per thread, padded band rows
    p.ct_window = with_cfar_window(tr, td, gr, gd, [](auto w) { return decltype(w)::compile_time; });
    p.band_pitch = p.ct_window ? det_band_pitch(C, hd) : C;
    const int unit = p.ct_window ? 4 : 1;
    // Band of rows under test: its cells and the 2 hr halo rows travel as at most DET_LOADS loads per thread (two cells per
    // load); 32 rows x 128 columns give each of the 1024 threads one item in either CFAR pass.
    const long cap_cells = (long)DET_LOADS * DET_NT * 2;
    int band = std::min<long>(std::max(1, tune_int("MMW_DETECT_BAND", DET_NT >= 1024 ? 32 : 24)), cap_cells / C - 2 * hr);
    band = std::min(band, std::max(unit, S - 2 * hr));
    band = band / unit * unit;
    if (band < unit) return p;                              // rows too long for the band loads
    p.band_rows = band;
    p.lds_screen = detect_screen_lds(band + 2 * hr, C, band, p.band_pitch, p.words, A);
    p.ok = p.lds_screen <= 160 * 1024 - 64;
    return p;
}
int fill_det_ant(const int *h_ant, int n_ant, int V, int A, DetAnt *out, AntList *full) {
    out->n = 0;
    full->n = 0;
    if (n_ant == 0) return MMW_OK;
    MMW_TRY(fill_ant_list(h_ant, n_ant, V, A, full));
    out->n = full->n;
    for (int i = 0; i < full->n && i < DET_LATE_MAX_ANT; ++i) out->idx[i] = full->idx[i];
    return MMW_OK;
}

// ---- mmw_detect_points, stage by stage (the driver is at the end)
// Scratch of one call, as byte offsets of its regions -- each 256-byte aligned, in this order -- and their total:
//   counters | flagged frames | undecided cells | speculative slots of the frames with undecided cells |
//   hand-over counters (overlapped schedule only) | flagged argmax evaluations, their partial sums (with an antenna list only) |
//   late argmax only: records, their detection slots, copy of the plane norms
struct DetectLayout {
    int cell_cap, list_cap, list_cap2;      // undecided cells | detection slots | flagged evaluations: both lists flag into one
    bool late;                              // the late argmax's regions exist (their 1 GiB rule is decided here)
    size_t ctl, flag_frames, cells, spec, sync, sync_bytes, list, part, rec_cells, rec_slot, l1_copy, total;
};
DetectLayout detect_layout(int n_frames, int cap, int V, int n_az, int n_el, int n_split, bool overlap, bool late_eligible) {
    DetectLayout l{};
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    auto region = [&](size_t bytes) { const size_t off = l.total; l.total += up(bytes); return off; };     // appended behind the last
    l.cell_cap = std::max(4096, 16 * n_frames);
    l.list_cap = n_frames * cap;
    l.list_cap2 = (int)std::min<long>(2L * l.list_cap, 0x7fffffffL);
    l.ctl = region(DCTL_WORDS * sizeof(int));
    l.flag_frames = region((size_t)n_frames * sizeof(int));
    l.cells = region((size_t)l.cell_cap * 2 * sizeof(int));
    l.spec = region((size_t)n_frames * (2 * DET_SPEC + 1) * sizeof(int));
    l.sync = region(overlap ? (CTL_CNT + (size_t)n_frames) * sizeof(unsigned) : 0);      // tickets, abort word | planes published per frame
    l.sync_bytes = l.total - l.sync;
    if (n_az || n_el) {
        l.list = region((size_t)std::max(l.list_cap2, 1) * sizeof(int));
        l.part = region((size_t)std::min(l.list_cap2, n_split) * REFINE_PARTS * std::max(std::max(n_az, n_el), 1) * sizeof(cplx<double>));
    }
    const size_t b_rec = up((size_t)l.list_cap * (n_az + n_el) * sizeof(float2)), b_rslot = up((size_t)l.list_cap * sizeof(int32_t)),
                 b_l1c = up((size_t)n_frames * V * sizeof(float));
    l.late = late_eligible && b_rec + b_rslot + b_l1c <= ((size_t)1 << 30);
    if (l.late) l.rec_cells = region(b_rec), l.rec_slot = region(b_rslot), l.l1_copy = region(b_l1c);
    return l;
}
// One call: what every stage works on.  The shapes, the CFAR window and the caller's output buffers are where the kernels read
// them: in `a` (the driver sets those fields, detect_fill_args the rest).
struct DetectCall {
    mmw_ctx *ctx;
    const void *cubes;                      // the caller's input, and the outputs of the range-Doppler stage as it wants them
    void *rd;
    float *l1;
    long n_train;
    int n_az, n_el;
    AntList az_full, el_full;
    DetectPlan plan;
    DetectLayout lay;
    DetectArgs a;
    bool overlap, refine;                   // the overlapped schedule | a float64 refinement behind the argmax (late argmax: lay.late)
    int scr_cus, n_split;                   // CUs of the overlapped consumer | flagged evaluations whose plane sums are split
    unsigned *sync_words;                   // scratch regions that are not part of `a`: lay.sync, lay.list, lay.part
    int *list;
    cplx<double> *part;
    const void *twA, *ws64, *wc64, *twS64, *twC64;
};

int detect_check(DetectCall &d, const int *h_az, const int *h_el) {
    const DetectArgs &a = d.a;
    MMW_REQUIRE(a.n_frames >= 0 && a.V > 0 && a.S > 0 && a.C > 0 && a.cap >= 0 && a.A > 0, "bad shape");
    MMW_REQUIRE(a.tr >= 0 && a.td >= 0 && a.gr >= 0 && a.gd >= 0, "negative window size");
    MMW_REQUIRE(d.n_az >= 0 && d.n_el >= 0 && (d.n_az == 0 || a.az_idx) && (d.n_el == 0 || a.el_idx), "antenna list without an index buffer");
    MMW_REQUIRE((long)a.n_frames * std::max(a.cap, 1) < (1L << 31) && (long)a.n_frames * 64 < (1L << 31), "too many detection slots for one call");
    d.plan = detect_plan(a.S, a.C, a.kind, a.tr, a.td, a.gr, a.gd, d.n_az, d.n_el, a.A);
    if (!d.plan.ok)
        return set_error(MMW_ERR_UNSUPPORTED, "mmw_detect_points: no screening kernel for this request (CA-CFAR on planes whose "
                         "float32 magnitudes fit the LDS, <= %d antennas per list, <= %d with 64 angle bins): use mmw_detect_batch + "
                         "mmw_angle_argmax_exact", DET_MAX_ANT, DET_LATE_MAX_ANT);
    const int hr = a.tr + a.gr, hd = a.td + a.gd;
    d.n_train = (long)(2 * hr + 1) * (2 * hd + 1) - (long)(2 * a.gr + 1) * (2 * a.gd + 1);
    MMW_REQUIRE(d.n_train >= 1 && d.n_train < (1L << 30), "empty training window");
    if (a.kind == MMW_CFAR_OS) MMW_REQUIRE(a.k_rank >= 1 && a.k_rank <= d.n_train, "k_rank must be between 1 and %ld, got %d", d.n_train, a.k_rank);
    MMW_TRY(fill_det_ant(h_az, d.n_az, a.V, a.A, &d.a.az, &d.az_full));
    return fill_det_ant(h_el, d.n_el, a.V, a.A, &d.a.el, &d.el_full);
}

// tables, the schedule of this call, its scratch
int detect_prepare(DetectCall &d) {
    mmw_ctx *ctx = d.ctx;
    const DetectArgs &a = d.a;
    MMW_TRY(get_table<float>(ctx, TAB_TWIDDLE, a.A, &d.twA));
    MMW_TRY(get_table<double>(ctx, TAB_TWIDDLE, a.S, &d.twS64));
    MMW_TRY(get_table<double>(ctx, TAB_TWIDDLE, a.C, &d.twC64));
    MMW_TRY(get_table<double>(ctx, TAB_HANN, a.S, &d.ws64));
    MMW_TRY(get_table<double>(ctx, TAB_HANN, a.C, &d.wc64));
    // Overlapped schedule (256 x 128 planes): the range-Doppler producer and the screening consumer run side by side on disjoint
    // CU sets, frames handed over through counters in device memory.  Built, tested and MEASURED: it does not
    // beat the serial schedule on this chip -- the range-Doppler kernel keeps its 5.2 TB/s down to ~224 CUs only, and the
    // screening of 1250 frames needs ~70 CU-milliseconds, i.e. 2.2 ms on the 32 CUs that leaves -- so it is an option, not the
    // default: MMW_DETECT_OVERLAP=1 selects it; MMW_DETECT_SCR_CUS = CUs of the consumer (a multiple of 32);
    // MMW_DETECT_TAIL=0: no second consumer launch behind the producer on the producer's CUs.
    d.scr_cus = opt_int(ctx, "MMW_DETECT_SCR_CUS", 32);
    if (d.scr_cus < 1 || d.scr_cus >= ctx->num_cu) d.scr_cus = 32;
    d.overlap = fused_rd_runs(a.S, a.C) && opt_int(ctx, "MMW_DETECT_OVERLAP", -1) == 1 &&
                ensure_det_queues(ctx, ctx->num_cu - d.scr_cus) == MMW_OK;
    // Late argmax (64 angle bins -- the reference's az_el_fft_size --, MMW_DETECT_LATE_ARGMAX=0: in the screening kernel): the
    // screening workgroup stops at the ordered detection list and copies each detection's range-Doppler cells into a flat
    // record list of the context; both angle estimates are launches of the lane-per-detection routine over those records
    // (k_angle_argmax_recs: the same float32 test with the same worst-case bound) on the side queue, in front of the float64
    // refinement -- part of the tail, so with the tail deferred they run beside the NEXT call's range-Doppler kernel, and they
    // read nothing that call overwrites.  The in-kernel form (one wave per detection, ~1.2 detections' worth of lanes busy)
    // cost the screening launch a third of its time: 0.27 -> 0.18 ms per 1250 frames.
    const bool late_eligible = a.cap > 0 && d.n_az + d.n_el > 0 && a.A == 64 && opt_int(ctx, "MMW_ARGMAX_FORM", 1) == 1 &&
                               opt_int(ctx, "MMW_DETECT_LATE_ARGMAX", 1) != 0;
    d.n_split = std::min(a.n_frames * a.cap, std::max(0, opt_int(ctx, "MMW_REFINE_SPLIT", 32768)));
    d.lay = detect_layout(a.n_frames, a.cap, a.V, d.n_az, d.n_el, d.n_split, d.overlap, late_eligible);
    d.refine = a.cap > 0 && (d.n_az || d.n_el);
    if ((d.n_az > DET_MAX_ANT || d.n_el > DET_MAX_ANT) && !d.lay.late)
        return set_error(MMW_ERR_UNSUPPORTED, "mmw_detect_points: lists of more than %d antennas need the late argmax (64 angle bins, "
                         "MMW_DETECT_LATE_ARGMAX / MMW_ARGMAX_FORM at their defaults, a detection capacity whose records fit 1 GiB)", DET_MAX_ANT);
    return ensure_scratch(ctx, d.lay.total);
}

void detect_fill_args(DetectCall &d) {
    DetectArgs &a = d.a;
    const DetectLayout &l = d.lay;
    char *base = (char *)d.ctx->scratch;
    const bool lists = d.n_az || d.n_el;
    d.sync_words = (unsigned *)(base + l.sync);
    d.list = lists ? (int *)(base + l.list) : nullptr;
    d.part = lists ? (cplx<double> *)(base + l.part) : nullptr;
    a.ctl = (int *)(base + l.ctl), a.flag_frames = (int *)(base + l.flag_frames);
    a.cells = (int *)(base + l.cells), a.cell_cap = l.cell_cap, a.spec = (int *)(base + l.spec);
    a.words = d.plan.words, a.band_rows = d.plan.band_rows, a.band_pitch = d.plan.band_pitch, a.n_train = (int)d.n_train;
    const float eps = 5.9604645e-8f, div = argmax_bound_div(d.ctx);
    const int ulps = rd_error_ulps(a.S, a.C);
    // the screening band always uses the full worst-case bound (MMW_DETECT_BAND_MULT widens it: test hook that sends more
    // cells through the float64 decision, or -- when huge -- whole frames back to the caller)
    a.k_fft = (float)ulps * eps * (float)std::max(1, opt_int(d.ctx, "MMW_DETECT_BAND_MULT", 1));
    a.twA = (const float2 *)d.twA;
    a.rf_az = ArgmaxRefine{d.l1, a.ctl + DCTL_ARGMAX, d.list, l.list_cap2, (float)ulps * eps / div, 4.f * (float)(d.n_az + 4) * eps / div};
    a.rf_el = ArgmaxRefine{d.l1, a.ctl + DCTL_ARGMAX, d.list, l.list_cap2, (float)ulps * eps / div, 4.f * (float)(d.n_el + 4) * eps / div};
    a.rf_el.tag = REFINE_SECOND, a.rf_el.n_tagged = a.ctl + DCTL_EL;
    if (l.late) {
        a.rec_cells = (float2 *)(base + l.rec_cells), a.rec_slot = (int32_t *)(base + l.rec_slot), a.rec_cap = l.list_cap;
        a.l1_copy = (float *)(base + l.l1_copy);
        a.rf_az.l1 = a.rf_el.l1 = a.l1_copy;
    }
    if (d.overlap) {
        a.sy_ctl = d.sync_words, a.sy_frame_cnt = d.sync_words + CTL_CNT;
        a.sy_timeout = (unsigned long long)std::max(1, opt_int(d.ctx, "MMW_CHAIN_TIMEOUT_MS", 2000)) * 100000ull;       // 100 MHz ticks
        a.sy_naps = std::max(0, opt_int(d.ctx, "MMW_DETECT_NAPS", 4));
    }
}

// Behind a pending tail the range-Doppler planes of a 256 x 128 batch are handed out by TICKETS (the producer kernel of the
// overlapped schedule: it never waits for anybody; same arithmetic, sc1 stores), so that a second launch of the same kernel can
// join in.  The counters are an allocation of their own: the scratch belongs to the pending tail.
int detect_rd_ticketed(DetectCall &d, int grid_main, int grid_help) {
    mmw_ctx *ctx = d.ctx;
    const DetectArgs &a = d.a;
    const size_t words = CTL_CNT + (size_t)a.n_frames;
    MMW_TRY(ensure_help_sync(ctx, words));
    const ChainSync cs = rd_ticket_sync(ctx->help_sync, a.n_frames, a.V);
    MMW_HIP(hipMemsetAsync(ctx->help_sync, 0, words * sizeof(unsigned), ctx->stream));
    MMW_HIP(hipEventRecord(ctx->help_begin, ctx->stream));
    MMW_HIP(hipStreamWaitEvent(ctx->q_tail, ctx->help_begin, 0));
    int rc;
    {
        ProfScope ps(ctx, "rd");
        rc = launch_rd_fused_det(ctx, d.cubes, d.rd, d.l1, a.n_frames * a.V, cs, grid_main);
    }
    if (rc == MMW_OK) {
        StreamScope on(ctx, ctx->q_tail);
        ProfScope ps(ctx, "rd_help");
        rc = launch_rd_fused_det(ctx, d.cubes, d.rd, d.l1, a.n_frames * a.V, cs, grid_help);
    }
    MMW_HIP(hipEventRecord(ctx->help_done, ctx->q_tail));       // (in any case: joined by the caller)
    if (rc != MMW_OK) MMW_HIP(hipStreamWaitEvent(ctx->stream, ctx->help_done, 0));
    return rc;
}

// range-Doppler of every antenna (float32) with the planes' L1 norms; joins the previous call's tail; resets the counters
int detect_range_doppler(DetectCall &d) {
    mmw_ctx *ctx = d.ctx;
    const DetectArgs &a = d.a;
    // Back-to-back calls (a frame loop over resident chunks): the previous call's tail -- exact cells, list insertion, float64
    // refinement: ~0.15 ms of latency-bound launches that leave the chip almost idle -- is still running on its side queues.
    // This call's range-Doppler kernel touches nothing the tail uses (the fused 256 x 128 kernel needs no scratch; its output
    // buffers are checked against the tail's), so it goes first and the tail is joined in front of the screening stage.
    // (the same holds for the compile-time mixed-radix kernels -- every shipped cfg's plane --: tables only, no scratch)
    bool rd_first = !d.overlap && ctx->tail_pending && rd_needs_no_scratch(a.S, a.C), helper = false;
    if (rd_first) {
        const std::pair<const char *, size_t> outs[2] = {{(const char *)d.rd, (size_t)a.n_frames * a.V * a.S * a.C * 8},
                                                         {(const char *)d.l1, (size_t)a.n_frames * a.V * sizeof(float)}};
        for (const auto &o : outs)
            for (const auto &t : ctx->tail_bufs)
                if (o.first < t.first + t.second && t.first < o.first + o.second) rd_first = false;
    }
    if (rd_first) {
        // the persistent kernel holds one workgroup per CU for its whole run: it leaves a few CUs to the tail's short workgroups
        // (32 at least: with fewer some shader engine has no free CU, and the dispatcher -- which places a launch's workgroups
        // engine by engine -- holds the tail's launches back until the range-Doppler launch ends)
        const int leave = std::max(0, std::min(opt_int(ctx, "MMW_DETECT_TAIL_CUS", 40), ctx->num_cu / 4));
        helper = fused_rd_runs(a.S, a.C) && a.n_frames * a.V > 4 * ctx->num_cu && leave > 0 && opt_int(ctx, "MMW_DETECT_RD_HELPER", 1) != 0;
        if (helper) {
            // On num_cu - leave CUs the launch is bound by CU-time (15000 planes x 23 us on 216 CUs: 1.60 ms), and the tail needs
            // its CUs for the first ~0.7-1.0 ms only: a second launch, `leave` workgroups, sits in the tail's queue BEHIND the
            // tail -- when the tail is done its CUs draw tickets too.
            MMW_TRY(detect_rd_ticketed(d, ctx->num_cu - leave, leave));
        } else {
            ctx->rd_leave_cus = leave;
            const int rc = range_doppler_impl(ctx, d.cubes, d.rd, nullptr, a.n_frames, a.V, a.S, a.C, RawView{1, 0}, d.l1);
            ctx->rd_leave_cus = 0;
            MMW_TRY(rc);
        }
    }
    MMW_TRY(join_tail(ctx));
    if (helper) MMW_HIP(hipStreamWaitEvent(ctx->stream, ctx->help_done, 0));
    MMW_HIP(hipMemsetAsync(a.ctl, 0, DCTL_WORDS * sizeof(int), ctx->stream));      // counters
    if (d.overlap) MMW_HIP(hipMemsetAsync(d.sync_words, 0, d.lay.sync_bytes, ctx->stream));
    if (!d.overlap && !rd_first) MMW_TRY(range_doppler_impl(ctx, d.cubes, d.rd, nullptr, a.n_frames, a.V, a.S, a.C, RawView{1, 0}, d.l1));
    return MMW_OK;
}

int detect_screen_serial(DetectCall &d) {
    mmw_ctx *ctx = d.ctx;
    ProfScope ps(ctx, "detect");
    DetectArgs a = d.a;
    PhaseClocks clk;       // diagnostics: shader clocks of a mid-batch workgroup's phases (load + |.|, CFAR bands, compaction, argmax)
    if (opt_int(ctx, "MMW_PHASE_CLOCKS", 0)) MMW_TRY(clk.alloc(5, ctx->stream));
    a.clk = clk.d;
    MMW_TRY(with_cfar_window(a.tr, a.td, a.gr, a.gd, [&](auto w) {
        using W = decltype(w);
        return launch_screen(ctx, k_detect_screen<W::tr, W::td, W::gr, W::gd>, a.n_frames, d.plan.lds_screen, a);
    }));
    if (clk.d) {
        long long h[5] = {0};
        MMW_TRY(clk.fetch(h, 5, ctx->stream));
        std::fprintf(stderr, "detect_screen %dx%d clocks: load %lld cfar %lld compact %lld argmax %lld\n", a.S, a.C, h[1] - h[0],
                     h[2] - h[1], h[3] - h[2], h[4] - h[3]);
    }
    return check_launch("detect_screen");
}

// producer on q_drd, consumer on q_dscr (disjoint CU sets), both ordered behind the context stream and joined to it again
int detect_screen_overlapped(DetectCall &d) {
    mmw_ctx *ctx = d.ctx;
    DetectArgs a = d.a;
    const ChainSync cs = rd_ticket_sync(d.sync_words, a.n_frames, a.V);
    const int n_planes = a.n_frames * a.V, rd_cus = ctx->num_cu - d.scr_cus;
    MMW_HIP(hipEventRecord(ctx->det_begin, ctx->stream));
    MMW_HIP(hipStreamWaitEvent(ctx->q_drd, ctx->det_begin, 0));
    MMW_HIP(hipStreamWaitEvent(ctx->q_dscr, ctx->det_begin, 0));
    PhaseClocks clk;       // diagnostics: phase clocks of one consumer workgroup, summed over its frames
    if (opt_int(ctx, "MMW_PHASE_CLOCKS", 0)) MMW_TRY(clk.alloc(16, ctx->stream));
    if (clk.d) MMW_HIP(hipStreamSynchronize(ctx->stream));
    a.clk = clk.d;
    auto screen = [&](int grid) -> int {
        MMW_TRY(with_cfar_window(a.tr, a.td, a.gr, a.gd, [&](auto w) {
            using W = decltype(w);
            return launch_screen(ctx, k_detect_screen_sync<W::tr, W::td, W::gr, W::gd>, grid, d.plan.lds_screen, a);
        }));
        return check_launch("detect_screen_sync");
    };
    int rc = MMW_OK;
    if (!opt_int(ctx, "MMW_DETECT_DIAG_SKIP_RD", 0)) {      // (test hook: no producer -- the consumer's bounded wait must give up)
        StreamScope on(ctx, ctx->q_drd);
        ProfScope ps(ctx, "rd");
        rc = launch_rd_fused_det(ctx, d.cubes, d.rd, d.l1, n_planes, cs, std::min(rd_cus, n_planes));
    }
    if (rc == MMW_OK) {
        StreamScope on(ctx, ctx->q_dscr);
        ProfScope ps(ctx, "detect");
        rc = screen(std::min(d.scr_cus * (1024 / DET_NT), a.n_frames));       // (512-thread workgroups: two per CU)
    }
    if (rc == MMW_OK && opt_int(ctx, "MMW_DETECT_TAIL", 1)) {
        // frames the consumer's CUs have not reached when the producer drains: the same kernel (same ticket counter) on
        // the producer's CUs, behind it in its queue
        StreamScope on(ctx, ctx->q_drd);
        ProfScope ps(ctx, "detect_tail");
        rc = screen(std::min(rd_cus * (1024 / DET_NT), a.n_frames));
    }
    // join in any case: whatever was enqueued runs to its end (bounded waits) before the context's next work
    MMW_HIP(hipEventRecord(ctx->det_rd_done, ctx->q_drd));
    MMW_HIP(hipEventRecord(ctx->det_scr_done, ctx->q_dscr));
    MMW_HIP(hipStreamWaitEvent(ctx->stream, ctx->det_rd_done, 0));
    MMW_HIP(hipStreamWaitEvent(ctx->stream, ctx->det_scr_done, 0));
    if (clk.d) {
        long long h[16] = {0};
        MMW_TRY(clk.fetch(h, 16, ctx->stream));
        std::fprintf(stderr, "detect_screen_sync %dx%d, workgroup 0 of the consumer: %lld frames; clocks per frame: wait %lld load %lld cfar %lld "
                     "compact %lld argmax %lld\n", a.S, a.C, h[7], h[5] / std::max(1LL, h[7]), h[0] / std::max(1LL, h[7]), h[1] / std::max(1LL, h[7]),
                     h[2] / std::max(1LL, h[7]), h[3] / std::max(1LL, h[7]));
        const long long nf = std::max(1LL, h[7]);
        std::fprintf(stderr, "  band loop per frame: top %lld land(+load wait) %lld issue+barrier %lld pass1 %lld pass2 %lld pass3 %lld; candidates %lld\n",
                     h[8] / nf, h[9] / nf, h[10] / nf, h[11] / nf, h[12] / nf, h[13] / nf, h[14] / nf);
    }
    return rc;
}

// the late argmax of one antenna list: one lane per record (ctx->stream)
void launch_argmax_recs(const DetectCall &d, int off, int32_t *idx, const AntList &ants, int shift, const ArgmaxRefine &rf) {
    if (ants.n == 0) return;
    const DetectArgs &a = d.a;
    const unsigned grid = (unsigned)std::max(1, std::min((d.lay.list_cap + 255) / 256, 2 * d.ctx->num_cu));
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, d.ctx->stream, (const float2 *)a.rec_cells, (const int32_t *)a.rec_slot,
                           (const int *)(a.ctl + DCTL_RECS), a.rec_cap, d.n_az + d.n_el, off, (const float *)a.l1_copy, idx, a.V, a.cap,
                           ants, (const float2 *)d.twA, rf);
    };
    if (ants.n <= 4) shift ? go(k_angle_argmax_recs<4, true>) : go(k_angle_argmax_recs<4, false>);
    else if (ants.n <= 8) shift ? go(k_angle_argmax_recs<8, true>) : go(k_angle_argmax_recs<8, false>);
    else shift ? go(k_angle_argmax_recs<16, true>) : go(k_angle_argmax_recs<16, false>);
}
// tail, side queue: angle estimates of every record (late argmax), then the float64 refinement of what the argmax flagged
int detect_tail_refine(DetectCall &d) {
    mmw_ctx *ctx = d.ctx;
    const DetectArgs &a = d.a;
    StreamScope on(ctx, ctx->q_side);
    int rc = MMW_OK;
    if (d.lay.late) {
        ProfScope ps(ctx, "argmax_tail");
        launch_argmax_recs(d, 0, a.az_idx, d.az_full, a.shift_az, a.rf_az);
        launch_argmax_recs(d, d.n_az, a.el_idx, d.el_full, a.shift_el, a.rf_el);
        rc = check_launch("angle_argmax_recs");
    }
    if (rc == MMW_OK) {
        ProfScope ps(ctx, "argmax_refine");
        RefineArgs ra{};
        rc = fill_refine_args(ctx, &ra, d.cubes, a.dets, a.ctl + DCTL_ARGMAX, d.list, d.lay.list_cap2, d.n_split, d.part, a.n_frames, a.V,
                              a.S, a.C, a.cap, a.A);
        ra.out_idx = a.az_idx, ra.ants = d.az_full, ra.shift = a.shift_az;
        ra.out_idx2 = a.el_idx, ra.ants2 = d.el_full, ra.shift2 = a.shift_el;
        if (rc == MMW_OK) rc = launch_argmax_refine(ctx, ra);
    }
    return rc;
}

// tail, tail queue: the float64 decision of the undecided cells, then (behind the refinement) the insertion of the positive ones
int detect_tail_exact(DetectCall &d) {
    mmw_ctx *ctx = d.ctx;
    const DetectArgs &a = d.a;
    StreamScope on(ctx, ctx->q_tail);
    ProfScope ps(ctx, "detect_exact");
    CellExactArgs ce{};
    ce.cubes = (const float2 *)d.cubes;
    ce.cells = a.cells, ce.n_cells = a.ctl + DCTL_CELLS, ce.cell_cap = d.lay.cell_cap, ce.spec = a.spec;
    ce.V = a.V, ce.S = a.S, ce.C = a.C;
    ce.kind = a.kind, ce.tr = a.tr, ce.td = a.td, ce.gr = a.gr, ce.gd = a.gd;
    ce.n_train = a.n_train, ce.k_rank = a.k_rank, ce.scale = a.scale;
    ce.ws = (const double *)d.ws64, ce.wc = (const double *)d.wc64;
    ce.twS = (const cplx<double> *)d.twS64, ce.twC = (const cplx<double> *)d.twC64;
    PhaseClocks clk;
    if (opt_int(ctx, "MMW_PHASE_CLOCKS", 0)) MMW_TRY(clk.alloc(5, ctx->stream));
    ce.clk = clk.d;
    hipLaunchKernelGGL(k_cfar_cell_exact, dim3(std::min(d.lay.cell_cap, 2 * ctx->num_cu)), dim3(CE_NT), d.plan.lds_cell, ctx->stream, ce);
    if (clk.d) {
        long long h[5] = {0};
        MMW_TRY(clk.fetch(h, 5, ctx->stream));
        std::fprintf(stderr, "cfar_cell_exact clocks: tables %lld range sums %lld doppler sums %lld decision %lld\n", h[1] - h[0], h[2] - h[1],
                     h[3] - h[2], h[4] - h[3]);
    }
    int rc = check_launch("cfar_cell_exact");
    if (d.refine) MMW_HIP(hipStreamWaitEvent(ctx->q_tail, ctx->side_join, 0));       // the refinement is done with the speculative slots
    if (rc == MMW_OK) {
        hipLaunchKernelGGL(k_detect_insert, dim3(std::min(a.n_frames, 4 * ctx->num_cu)), dim3(INS_NT), 0, ctx->stream, d.a);
        rc = check_launch("detect_insert");
    }
    return rc;
}

// the tail is registered as pending with what it reads / writes besides the scratch; join_now: the context stream waits for it
int detect_tail_end(DetectCall &d, bool join_now) {
    mmw_ctx *ctx = d.ctx;
    const DetectArgs &a = d.a;
    MMW_HIP(hipEventRecord(ctx->tail_done, ctx->q_tail));
    ctx->tail_pending = true;
    const size_t slots = (size_t)a.n_frames * a.cap;
    ctx->tail_bufs = {{(const char *)d.cubes, (size_t)a.n_frames * a.V * a.S * a.C * 8}, {(const char *)a.dets, slots * 8},
                      {(const char *)a.counts, (size_t)a.n_frames * 4}, {(const char *)a.az_idx, a.az_idx ? slots * 4 : 0},
                      {(const char *)a.el_idx, a.el_idx ? slots * 4 : 0}};
    return join_now ? join_tail(ctx) : MMW_OK;
}
// Behind the screening: the exact decision of the undecided cells (tail queue) and the float64 refinement of the flagged
// argmax evaluations (side queue) run SIDE BY SIDE -- neither needs the other: the frames with undecided cells carry them in
// speculative slots --, then k_detect_insert puts the cells decided positive into their lists.
int detect_tail(DetectCall &d, bool want_stats) {
    mmw_ctx *ctx = d.ctx;
    // (each handle on its own: ensure_det_queues destroys the whole detection group when the CU split changes, the events stay)
    for (hipStream_t *q : {&ctx->q_side, &ctx->q_tail})
        if (!*q) MMW_HIP(hipStreamCreateWithFlags(q, hipStreamNonBlocking));
    for (hipEvent_t *e : {&ctx->side_fork, &ctx->side_join, &ctx->tail_done, &ctx->help_begin, &ctx->help_done})
        if (!*e) MMW_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
    MMW_HIP(hipEventRecord(ctx->side_fork, ctx->stream));
    MMW_HIP(hipStreamWaitEvent(ctx->q_tail, ctx->side_fork, 0));
    // from here on the context stream is only the point the tail is joined to: on error, or when the caller wants the
    // statistics / the tail is not to be deferred (MMW_DETECT_DEFER_TAIL=0), before this call returns; else at the next entry point
    if (d.refine) {
        MMW_HIP(hipStreamWaitEvent(ctx->q_side, ctx->side_fork, 0));
        const int rc = detect_tail_refine(d);
        MMW_HIP(hipEventRecord(ctx->side_join, ctx->q_side));      // (joined in any case: in front of the list insertion)
        if (rc != MMW_OK) {
            MMW_HIP(hipStreamWaitEvent(ctx->q_tail, ctx->side_join, 0));
            (void)detect_tail_end(d, true);
            return rc;
        }
    }
    const int rc_tail = detect_tail_exact(d);
    const int rc_end = detect_tail_end(d, rc_tail != MMW_OK || want_stats || !opt_int(ctx, "MMW_DETECT_DEFER_TAIL", 1));
    MMW_TRY(rc_tail);
    return rc_end;
}

int detect_read_stats(DetectCall &d, int *h_stats) {
    int h[DCTL_WORDS];
    MMW_HIP(hipMemcpyAsync(h, d.a.ctl, sizeof(h), hipMemcpyDeviceToHost, d.ctx->stream));
    MMW_HIP(hipStreamSynchronize(d.ctx->stream));
    h_stats[0] = h[DCTL_FLAG_FRAMES], h_stats[1] = h[DCTL_CELLS], h_stats[2] = h[DCTL_FALLBACK];
    h_stats[3] = h[DCTL_ARGMAX] - h[DCTL_EL], h_stats[4] = h[DCTL_EL];
    return MMW_OK;
}

}  // namespace

extern "C" {

int mmw_angle_argmax(mmw_ctx *ctx, const void *d_rd, const int32_t *d_dets, const int32_t *d_counts,
                     int32_t *d_idx, int n_frames, int V, int S, int C, int cap, const int *h_ant, int n_ant,
                     int A, int shift) {
    MMW_REQUIRE(ctx && d_rd && d_dets && d_counts && d_idx, "null argument");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_frames >= 0 && n_frames <= 65535 && V > 0 && S > 0 && C > 0 && cap >= 0 && A > 0, "bad shape");
    AntList ants{};
    MMW_TRY(fill_ant_list(h_ant, n_ant, V, A, &ants));
    if (n_frames == 0 || cap == 0) return MMW_OK;
    const void *twA = nullptr;
    MMW_TRY(get_table<float>(ctx, TAB_TWIDDLE, A, &twA));
    ProfScope ps(ctx, "argmax");
    dim3 grid(std::min((cap + 3) / 4, 32), n_frames);      // 128 detections per frame in one pass, more by looping
    launch_angle_argmax(ctx, grid, (const float2 *)d_rd, d_dets, d_counts, d_idx, V, S, C, cap, ants, A, shift,
                        (const float2 *)twA, ArgmaxRefine{});
    return check_launch("angle_argmax");
}

int mmw_angle_argmax_exact(mmw_ctx *ctx, const void *d_cubes, const float *d_l1, const void *d_rd, const int32_t *d_dets,
                           const int32_t *d_counts, int32_t *d_idx, int n_frames, int V, int S, int C, int cap,
                           const int *h_ant, int n_ant, int A, int shift, int *h_n_refined) {
    MMW_REQUIRE(ctx && d_cubes && d_l1 && d_rd && d_dets && d_counts && d_idx, "null argument");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_frames >= 0 && n_frames <= 65535 && V > 0 && S > 0 && C > 0 && cap >= 0 && A > 0, "bad shape");
    MMW_REQUIRE((long)n_frames * cap < (1L << 31), "too many detection slots for one call");
    AntList ants{};
    MMW_TRY(fill_ant_list(h_ant, n_ant, V, A, &ants));
    if (h_n_refined) *h_n_refined = 0;
    if (n_frames == 0 || cap == 0) return MMW_OK;
    const void *twA = nullptr;
    MMW_TRY(get_table<float>(ctx, TAB_TWIDDLE, A, &twA));
    const int list_cap = n_frames * cap;
    const int n_split = std::min(list_cap, std::max(0, opt_int(ctx, "MMW_REFINE_SPLIT", 32768)));   // flagged detections whose
                                                                                          // plane sums are split over workgroups
    // Dense refinement (mmw_cells64.h): when many evaluations are flagged -- noise-level detections, e.g. the GUI's OS-CFAR --
    // the float64 cells of a whole frame come from one Doppler FFT per sample row + 256-term range sums instead of one
    // 32768-term sum per cell and antenna.  On when the call flags >= dense_min evaluations (8 per frame; MMW_ARGMAX_DENSE_MIN)
    // and the plane has a kernel (cells64_plan: 128 chirps, or a chirp count of k_cells64_mixed with MMW_ARGMAX_DENSE_MIXED on);
    // covers the first dense_cap entries of the list, the direct kernels the rest.
    Cells64Plan plan = cells64_plan(S, C);
    if (plan.kind == C64_KIND_MIXED && !opt_int(ctx, "MMW_ARGMAX_DENSE_MIXED", ARGMAX_DENSE_MIXED_DEFAULT)) plan = Cells64Plan{};
    const int max_cells = plan.cells;
    const int dense_min = max_cells > 0 ? std::max(1, opt_int(ctx, "MMW_ARGMAX_DENSE_MIN", 8 * n_frames)) : 0;
    const int dense_cap = dense_min > 0 ? (int)std::min<long>(list_cap, 256L * n_frames) : 0;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t list_bytes = up(256 + (size_t)list_cap * sizeof(int));
    const size_t part_bytes = up((size_t)n_split * REFINE_PARTS * n_ant * sizeof(cplx<double>));
    const size_t pos_bytes = dense_min > 0 ? up((size_t)list_cap * sizeof(int)) : 0;
    const size_t cell_bytes = up((size_t)dense_cap * n_ant * sizeof(cplx<double>));
    MMW_TRY(ensure_scratch(ctx, list_bytes + part_bytes + pos_bytes + cell_bytes));
    int *d_nflag = (int *)ctx->scratch, *d_list = (int *)((char *)ctx->scratch + 256);
    int *d_flagpos = dense_min > 0 ? (int *)((char *)ctx->scratch + list_bytes + part_bytes) : nullptr;
    cplx<double> *d_cells = (cplx<double> *)((char *)ctx->scratch + list_bytes + part_bytes + pos_bytes);
    MMW_HIP(hipMemsetAsync(d_nflag, 0, 256, ctx->stream));
    if (d_flagpos) MMW_HIP(hipMemsetAsync(d_flagpos, 0, (size_t)list_cap * sizeof(int), ctx->stream));
    const float eps = 5.9604645e-8f, div = argmax_bound_div(ctx);
    ArgmaxRefine rf{d_l1, d_nflag, d_list, list_cap, (float)rd_error_ulps(S, C) * eps / div, 4.f * (float)(n_ant + 4) * eps / div,
                    d_flagpos, dense_cap};
    ProfScope ps(ctx, "argmax");
    dim3 grid(std::min((cap + 3) / 4, 32), n_frames);      // 128 detections per frame in one pass, more by looping
    launch_angle_argmax(ctx, grid, (const float2 *)d_rd, d_dets, d_counts, d_idx, V, S, C, cap, ants, A, shift,
                        (const float2 *)twA, rf);
    MMW_TRY(check_launch("angle_argmax"));
    RefineArgs ra{};
    MMW_TRY(fill_refine_args(ctx, &ra, d_cubes, d_dets, d_nflag, d_list, list_cap, n_split, (cplx<double> *)((char *)ctx->scratch + list_bytes),
                             n_frames, V, S, C, cap, A));
    ra.out_idx = d_idx;
    ra.ants = ants;
    ra.shift = shift;
    ra.dense_min = dense_min;
    ra.dense_cap = dense_cap;
    if (dense_min > 0) {
        MMW_TRY(launch_cells64(ctx, ra, d_counts, d_flagpos, dense_min, d_cells, n_frames, plan));
        Argmax64ListArgs la{d_cells, d_nflag, d_list, dense_min, dense_cap, n_ant, A, shift, d_idx, ra.twA};
        hipLaunchKernelGGL(k_argmax64_list, dim3((unsigned)std::min(std::max(dense_cap / 4, 1), 4 * ctx->num_cu)), dim3(256), 0, ctx->stream, la);
        MMW_TRY(check_launch("argmax64_list"));
    }
    MMW_TRY(launch_argmax_refine(ctx, ra));
    if (h_n_refined) {
        MMW_HIP(hipMemcpyAsync(h_n_refined, d_nflag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        MMW_HIP(hipStreamSynchronize(ctx->stream));
    }
    return MMW_OK;
}

int mmw_detect_points_supported(int S, int C, int cfar_kind, int train_r, int train_d, int guard_r, int guard_d, int n_az,
                                int n_el, int A) {
    if (S <= 0 || C <= 0 || train_r < 0 || train_d < 0 || guard_r < 0 || guard_d < 0 || n_az < 0 || n_el < 0) return 0;
    return detect_plan(S, C, cfar_kind, train_r, train_d, guard_r, guard_d, n_az, n_el, A).ok ? 1 : 0;
}

// Invariants of every return path:
//  1. ctx->stream is the context's main stream (the stages switch it with StreamScope only);
//  2. everything enqueued on the detection group (q_drd, q_dscr, q_side, q_tail) is ordered before the main stream or registered as
//     the pending tail with its buffer list (detect_tail_end).  The stages' own joins "in any case" cover a failed launch; a failed HIP
//     call between a launch and its join is covered by ONE mechanism, drain(ctx, Q_DETECT) at the end of the driver, not by the guards;
//  3. no device allocation made by the call outlives it (the diagnostics' buffers are PhaseClocks; the rest belongs to the context).
int mmw_detect_points(mmw_ctx *ctx, const void *d_cubes, void *d_rd, float *d_l1, float *d_mag32, int32_t *d_dets,
                      int32_t *d_counts, int32_t *d_az_idx, int32_t *d_el_idx, int n_frames, int V, int S, int C, int cfar_kind,
                      int train_r, int train_d, int guard_r, int guard_d, double scale, int k_rank, int cap, const int *h_az,
                      int n_az, int shift_az, const int *h_el, int n_el, int shift_el, int A, int *h_stats) {
    MMW_REQUIRE(ctx && d_cubes && d_rd && d_l1 && d_dets && d_counts, "null argument");
    MMW_TRY(join_pipe(ctx, true));      // (the previous call's deferred tail: joined behind this call's range-Doppler kernel)
    DetectCall d{};
    DetectArgs &a = d.a;
    d.ctx = ctx, d.cubes = d_cubes, d.rd = d_rd, d.l1 = d_l1, d.n_az = n_az, d.n_el = n_el;
    a.rd = (const float2 *)d_rd, a.l1 = d_l1, a.mag32 = d_mag32;
    a.dets = d_dets, a.counts = d_counts, a.az_idx = d_az_idx, a.el_idx = d_el_idx;
    a.n_frames = n_frames, a.V = V, a.S = S, a.C = C, a.A = A, a.cap = cap, a.shift_az = shift_az, a.shift_el = shift_el;
    a.kind = cfar_kind, a.tr = train_r, a.td = train_d, a.gr = guard_r, a.gd = guard_d, a.k_rank = k_rank, a.scale = scale;
    MMW_TRY(detect_check(d, h_az, h_el));
    if (h_stats) std::fill(h_stats, h_stats + 5, 0);
    if (n_frames == 0) return MMW_OK;
    MMW_TRY(detect_prepare(d));
    detect_fill_args(d);
    int rc = detect_range_doppler(d);
    if (rc == MMW_OK) rc = d.overlap ? detect_screen_overlapped(d) : detect_screen_serial(d);
    if (rc == MMW_OK) rc = detect_tail(d, h_stats != nullptr);
    if (rc == MMW_OK && h_stats) rc = detect_read_stats(d, h_stats);
    if (rc != MMW_OK) (void)drain(ctx, Q_DETECT);       // invariant 2 on every failure path (also waits for a previous call's pending tail: errors only)
    return rc;
}

int mmw_angle_argmax_cells64(mmw_ctx *ctx, const void *d_cells, int32_t *d_idx, int n_rows, int n_ant, int A, int shift) {
    MMW_REQUIRE(ctx && d_cells && d_idx, "null argument");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_rows >= 0 && n_ant >= 1 && A >= n_ant, "bad shape (need 1 <= n_ant <= A)");
    if (n_rows == 0) return MMW_OK;
    const void *twA64;
    MMW_TRY(get_table<double>(ctx, TAB_TWIDDLE, A, &twA64));
    hipLaunchKernelGGL(k_argmax64_cells, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, ctx->stream,
                       (const cplx<double> *)d_cells, d_idx, n_rows, n_ant, A, shift, (const cplx<double> *)twA64);
    return check_launch("argmax64_cells");
}

// The float64 range-Doppler cells behind the exact argmax, read out: the dense routes are k_cells64<128> and k_cells64_mixed<C>
// themselves with every listed detection marked flagged (list position f * cap + det, so its output array IS d_out), the direct route the slices of
// k_argmax_refine_part added in k_argmax_refine_finish's order.  A test entry: it synchronises and validates the list on the host.
int mmw_rd_cells64_at(mmw_ctx *ctx, const void *d_cubes, const int32_t *d_dets, const int32_t *d_counts, void *d_out, int n_frames,
                      int V, int S, int C, int cap, const int *h_ant, int n_ant, int route) {
    MMW_REQUIRE(ctx && d_cubes && d_dets && d_counts && d_out, "null argument");
    MMW_JOIN(ctx);
    MMW_REQUIRE(n_frames >= 0 && n_frames <= 65535 && V > 0 && S > 0 && S <= 65535 && C > 0 && cap >= 0, "bad shape");
    MMW_REQUIRE((long)n_frames * cap < (1L << 31), "too many detection slots for one call");
    MMW_REQUIRE(route == MMW_CELLS64_DENSE || route == MMW_CELLS64_DIRECT || route == MMW_CELLS64_DENSE_MIXED,
                "route must be MMW_CELLS64_DENSE, MMW_CELLS64_DIRECT or MMW_CELLS64_DENSE_MIXED");
    AntList ants{};
    MMW_TRY(fill_ant_list(h_ant, n_ant, V, MAX_ANT, &ants));
    // MMW_CELLS64_DENSE: the 128-chirp kernel only; MMW_CELLS64_DENSE_MIXED: k_cells64_mixed<C>, also at C == 128
    Cells64Plan plan{};
    if (route == MMW_CELLS64_DENSE && C == 128) plan = cells64_plan(S, C);
    if (route == MMW_CELLS64_DENSE_MIXED) plan = cells64_mixed_plan(S, C);
    const bool dense = route != MMW_CELLS64_DIRECT;
    if (dense && plan.kind == C64_KIND_NONE)
        return set_error(MMW_ERR_UNSUPPORTED, "no dense float64 cell kernel for %d x %d planes", S, C);
    if (n_frames == 0 || cap == 0) return MMW_OK;
    const int list_cap = n_frames * cap;
    std::vector<int32_t> counts(n_frames), dets((size_t)list_cap * 2);
    MMW_HIP(hipMemcpyAsync(counts.data(), d_counts, counts.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    MMW_HIP(hipMemcpyAsync(dets.data(), d_dets, dets.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    MMW_HIP(hipStreamSynchronize(ctx->stream));
    // words 0 .. 63: the count; then the list (direct: the listed slots in order; dense: flagpos[F][cap])
    std::vector<int> host(64 + (size_t)list_cap, 0);
    int n = 0;
    for (int f = 0; f < n_frames; ++f)
        for (int det = 0; det < std::min(std::max(counts[f], 0), cap); ++det) {
            const int slot = f * cap + det, r = dets[2 * (size_t)slot], d = dets[2 * (size_t)slot + 1];
            MMW_REQUIRE(r >= 0 && r < S && d >= 0 && d < C, "detection %d of frame %d lies outside the %d x %d plane", det, f, S, C);
            if (dense) host[64 + slot] = slot + 1;
            else host[64 + n] = slot;
            ++n;
        }
    if (n == 0) return MMW_OK;
    host[0] = dense ? list_cap : n;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const int parts = refine_parts(n_frames);
    const size_t list_bytes = up(host.size() * sizeof(int));
    const size_t part_bytes = route == MMW_CELLS64_DIRECT ? up((size_t)n * parts * n_ant * sizeof(cplx<double>)) : 0;
    MMW_TRY(ensure_scratch(ctx, list_bytes + part_bytes));
    int *d_nflag = (int *)ctx->scratch, *d_list = d_nflag + 64;
    MMW_HIP(hipMemcpyAsync(d_nflag, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    MMW_HIP(hipStreamSynchronize(ctx->stream));       // (`host` is pageable and leaves scope on every return below)
    RefineArgs ra{};
    MMW_TRY(fill_refine_args(ctx, &ra, d_cubes, d_dets, d_nflag, d_list, n, n, (cplx<double> *)((char *)ctx->scratch + list_bytes),
                             n_frames, V, S, C, cap, MAX_ANT));
    ra.ants = ants;
    int rc = MMW_OK;
    if (dense) {
        rc = launch_cells64(ctx, ra, d_counts, d_list, 1, (cplx<double> *)d_out, n_frames, plan);
    } else {
        MMW_TRY(launch_refine_part(ctx, ra, std::min(n, 512)));
        hipLaunchKernelGGL(k_refine_cells_sum, dim3((unsigned)(((long)n * n_ant + 255) / 256)), dim3(256), 0, ctx->stream, ra,
                           (cplx<double> *)d_out, n);
        rc = check_launch("refine_cells_sum");
    }
    MMW_TRY(rc);
    MMW_HIP(hipStreamSynchronize(ctx->stream));       // a test entry: d_out is complete at return
    return MMW_OK;
}

int mmw_diag_cells64_plan(int S, int C, int plan[8]) {
    MMW_REQUIRE(plan && S > 0 && C > 0, "bad argument");
    for (int i = 0; i < 8; ++i) plan[i] = 0;
    const Cells64Plan p = cells64_plan(S, C);
    plan[0] = p.kind;
    if (p.kind != C64_KIND_NONE) {
        plan[1] = p.R1;
        plan[2] = p.R2;
        plan[3] = p.rows;
        plan[4] = (int)p.lds;
        plan[5] = p.cells;
        plan[6] = p.pitch;
    }
    plan[7] = cells64_mixed_plan(S, C).kind == C64_KIND_MIXED;
    return MMW_OK;
}

int mmw_diag_detect_plan(int S, int C, int cfar_kind, int train_r, int train_d, int guard_r, int guard_d, int n_az, int n_el, int A,
                         int plan[8]) {
    MMW_REQUIRE(plan && S > 0 && C > 0 && train_r >= 0 && train_d >= 0 && guard_r >= 0 && guard_d >= 0 && n_az >= 0 && n_el >= 0,
                "bad argument");
    const DetectPlan p = detect_plan(S, C, cfar_kind, train_r, train_d, guard_r, guard_d, n_az, n_el, A);
    plan[0] = p.ok;
    plan[1] = p.ok ? 1 : 0;                                 // workgroups per frame (row tiles went with the band-streamed kernel)
    plan[2] = p.ok ? (int)(((long)DET_LOADS * DET_NT * 2) / C) : 0;      // rows one band's loads can carry (band + halo)
    plan[3] = p.band_rows;
    plan[4] = p.band_pitch;
    plan[5] = (int)p.lds_screen;
    plan[6] = p.ct_window;
    plan[7] = rd_error_ulps(S, C);
    return MMW_OK;
}

}  // extern "C"
