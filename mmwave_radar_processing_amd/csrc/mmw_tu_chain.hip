// Translation unit of the FFT chain: the angle stage, the schedule of one chain call (serial, overlapped, device-synchronised),
// the sync-slot table of the device-synchronised form, chain_settle, and the chain / raw-cube entry points.
// Launches through mmw_launch.h only: every kernel behind it is compiled in a unit of its own.
#include "mmw_entry.h"
#include "mmw_launch.h"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>

using namespace mmw;

// Does the angle stage of this call run k_angle64's ZE variant (planes 0 and V-1 never loaded)?
static bool angle_fast_path(int V, long bins, int A, bool mag) {      // per launch of at most 65535 frames
    // odd bin counts: complex output only (k_angle64_rows_odd)
    return A == 64 && (bins % 2 == 0 || !mag) && !env_int("MMW_NO_FUSED_ANGLE", 0) && (V == 4 || V == 8 || V == 12 || V == 16);
}
static bool angle_skips_end_planes(const mmw_ctx *ctx, int V, long bins, int A, int flags) {
    return angle_fast_path(V, bins, A, (flags & MMW_ANGLE_MAGNITUDE) != 0) && V > 2 && !(flags & MMW_ANGLE_NO_WINDOW) &&
           np_window(TAB_HANN, 0, V) == 0.0 && np_window(TAB_HANN, V - 1, V) == 0.0 && opt_int(ctx, "MMW_ANGLE_ZE", 1) != 0;
}

int mmw::angle_fft_impl(mmw_ctx *ctx, const void *d_rd, void *d_out, int n_frames, int V, int S, int C, int A, int flags) {
    MMW_REQUIRE(ctx && d_rd && d_out, "null argument");
    MMW_REQUIRE(n_frames >= 0 && V > 0 && S > 0 && C > 0 && A >= V, "bad shape (need A >= V)");
    MMW_REQUIRE((flags & ~7) == 0, "unknown flag bits %d", flags);
    if (n_frames == 0) return MMW_OK;
    const bool magnitude = flags & MMW_ANGLE_MAGNITUDE, window = !(flags & MMW_ANGLE_NO_WINDOW),
               shift = !(flags & MMW_ANGLE_NO_SHIFT);
    ProfScope ps(ctx, "angle");
    const long bins = (long)S * C;
    if (n_frames <= 65535 && angle_fast_path(V, bins, A, magnitude)) {
        float h[16];
        for (int i = 0; i < V; ++i) h[i] = window ? (float)np_window(TAB_HANN, i, V) : 1.f;
        switch (V) {
            case 4: return launch_angle64<4>(ctx, d_rd, d_out, n_frames, bins, magnitude, h, shift);
            case 8: return launch_angle64<8>(ctx, d_rd, d_out, n_frames, bins, magnitude, h, shift);
            case 12: return launch_angle64<12>(ctx, d_rd, d_out, n_frames, bins, magnitude, h, shift);
            default: return launch_angle64<16>(ctx, d_rd, d_out, n_frames, bins, magnitude, h, shift);
        }
    }
    FftArgs a{};
    a.in = d_rd;
    a.out = d_out;
    a.outer = n_frames;
    a.inner = (int)bins;
    a.n_in = V;
    a.in_outer_stride = (long)V * bins;
    a.out_outer_stride = (long)A * bins;
    a.in_axis_stride = a.out_axis_stride = bins;
    a.in_inner_stride = a.out_inner_stride = 1;
    if (window) MMW_TRY(get_table<float>(ctx, TAB_HANN, V, &a.win_axis));
    a.scale = 1.0;
    a.shift = shift;
    a.magnitude = magnitude;
    return launch_fft_axis<float, float>(ctx, a, A, false);
}

// Lazily create the two CU-masked queues of the overlapped chain: the RD queue owns the first rd_cus
// CU-mask bits, the angle queue the rest, so workgroups of the two kernels are co-resident on the chip.
// rd_cus == 0: no masks (both queues may use every CU).  A failure leaves the context without chain queues
// (pipe_unavailable) and the chain falls back to its serial schedule.
static int ensure_pipe_queues(mmw_ctx *ctx, int rd_cus) {
    if (ctx->pipe_unavailable) return set_error(MMW_ERR_UNSUPPORTED, "chain queues unavailable on this runtime");
    if (ctx->q_rd && ctx->q_rd_cus == rd_cus) return MMW_OK;
    MMW_HIP(destroy_queues(ctx, Q_CHAIN));
    if (!ctx->pipe_begin) {                         // events are created once per context
        for (int i = 0; i < PIPE_RING_MAX; ++i) {
            MMW_HIP(hipEventCreateWithFlags(&ctx->pipe_rd[i], hipEventDisableTiming));
            MMW_HIP(hipEventCreateWithFlags(&ctx->pipe_ang[i], hipEventDisableTiming));
        }
        MMW_HIP(hipEventCreateWithFlags(&ctx->pipe_begin, hipEventDisableTiming));
    }
    // Two angle queues on the same CUs take alternate chunks: the barrier / marker packets around one launch are
    // processed while the other queue's kernel runs (one queue alone idles ~15 us per launch).
    const hipError_t e = create_split_queues(ctx, rd_cus, {&ctx->q_rd, &ctx->q_ang, &ctx->q_ang2});
    if (e != hipSuccess) {
        ctx->pipe_unavailable = true;
        return set_error(MMW_ERR_UNSUPPORTED, "chain queue creation failed: %s", hipGetErrorString(e));
    }
    ctx->q_rd_cus = rd_cus;
    for (int i = 0; i < PIPE_RING_MAX; ++i) ctx->pipe_ang_used[i] = false;   // the old queues were drained above
    return MMW_OK;
}

// Schedule of one chain call (DESIGN.md "chain schedule"), also reported by mmw_diag_chain_plan.
//  serial    : RD then angle over chunks of frames on the context stream.
//  overlapped: RD(k+1) on a queue masked to rd_cus CUs runs beside angle(k) on the remaining CUs.  RD is
//              LDS/ALU/latency bound, angle is HBM-write bound (a CU sustains ~44 GB/s of stores, so it needs
//              about half the chip), and the ring of RD chunks stays resident in the 256 MB Infinity
//              Cache, so the RD->angle intermediate never goes to HBM.  Default for batches of the fused
//              shape; MMW_CHAIN_PIPELINE=0/1 forces a schedule.
struct ChainPlan {
    bool pipelined;
    int chunk, ring, rd_cus, vskip;
    bool sync;              // device-synchronised form: one RD launch + one angle launch per call (ChainSync)
    int ring_frames;        // sync: frames in the ring of RD cubes
};
static ChainPlan chain_plan(const mmw_ctx *ctx, bool keep_rd, bool raw, int n_frames, int V, int S, int C, int A, int flags,
                            bool allow_sync = true, bool i16 = false) {
    ChainPlan p{};
    // Planes nobody reads are not transformed: with the Hann(V) antenna window the end antennas have weight exactly 0
    // (np.hanning end points) and k_angle64's ZE variant never loads them, so when the RD cube is only an internal
    // intermediate (d_rd == NULL) their range-Doppler transform is skipped: 1/6 of the RD work at V = 12.
    // (Non-finite samples in an end antenna: the reference's 0 * inf gives NaN everywhere, this path stays finite.)
    p.vskip = (!keep_rd && angle_skips_end_planes(ctx, V, (long)S * C, A, flags) && opt_int(ctx, "MMW_CHAIN_SKIP_ENDS", 1)) ? V : 0;
    const int v_live = p.vskip > 2 ? V - 2 : V;
    // CU split: half the chip each.  The angle stage is bound by HBM writes and needs ~128 CUs to saturate them (a CU
    // sustains ~44 GB/s of stores); the range-Doppler stage keeps up from 112 CUs on (sweep in DESIGN.md)
    // Mixed-radix planes above 80 KB leave ONE range-Doppler workgroup per CU and are arithmetic bound: 5/8 of the chip
    // (tools/chain_modes.sh: 254 x 50, 100 x 100, 120 x 126 are 6-25 % faster at 160 than at 128 CUs; the angle stage
    // still saturates its store stream from the other 96).
    // Planes with a 127-point level are arithmetic bound wherever they run (the level is a dense real matrix product on
    // float32 MFMAs, which share the vector ALUs): 5/8 as well at 63 x 127 (+4 %), 3/4 at 254 x 50 (one 104 KB plane per
    // CU: 4.06 against 3.82 TB/s at 5/8; sweep of 128..208 CUs in profiles/r03_chain_rd_cus.log).
    const size_t plane_lds = (size_t)S * (C | 1) * sizeof(cplx<float>);
    const bool big_prime = S % 127 == 0 || C % 127 == 0;
    const bool heavy_rd = !fused_rd_ok(S, C) && (plane_lds > 80 * 1024 || big_prime);
    const int rd_cus_dflt = !heavy_rd ? ctx->num_cu / 2 : (big_prime && plane_lds > 100 * 1024) ? ctx->num_cu * 3 / 4 : ctx->num_cu * 5 / 8;
    p.rd_cus = opt_int(ctx, "MMW_RD_CUS", rd_cus_dflt);
    if (p.rd_cus < 0 || p.rd_cus >= ctx->num_cu) p.rd_cus = rd_cus_dflt;         // 0: unmasked queues
    p.ring = std::max(2, std::min(opt_int(ctx, "MMW_CHAIN_RING", 3), (int)PIPE_RING_MAX));
    // chunk: whole RD waves (rd_cus planes each) and `ring` chunks of live RD planes within ~250 MB of cache
    const size_t live_bytes = (size_t)v_live * S * C * sizeof(cplx<float>);
    int chunk_auto = (int)((250u << 20) / ((size_t)p.ring * live_bytes));
    {
        const int wave_cus = p.rd_cus > 0 ? p.rd_cus : ctx->num_cu;
        const int waves = (int)((long)chunk_auto * v_live / wave_cus);
        if (waves >= 1) chunk_auto = (int)((long)waves * wave_cus / v_live);
    }
    if (chunk_auto < 1) chunk_auto = 1;
    const bool fused_shape = (fused_rd_ok(S, C) || rd_lds_supported(S, C) || rd_mixed_supported(S, C)) &&
                             angle_fast_path(V, (long)S * C, A, (flags & MMW_ANGLE_MAGNITUDE) != 0);   // both stages have a single-pass kernel
    // (the split kernel of the 32768-cell planes is latency bound at 2 waves per SIMD: on half the chip it is slower than
    //  the serial schedule -- 5.6 vs 5.3 us/frame at 12 x 512 x 64 -- so those planes stay serial)
    const int want_pipe = opt_int(ctx, "MMW_CHAIN_PIPELINE", -1);
    p.pipelined = !keep_rd && !ctx->pipe_unavailable &&
                  (want_pipe == 1 || (want_pipe == -1 && fused_shape && n_frames >= 2 * chunk_auto));
    p.chunk = opt_int(ctx, "MMW_CHAIN_CHUNK", p.pipelined ? chunk_auto : 1024);
    p.chunk = std::max(1, std::min(p.chunk, std::min(n_frames, 65535)));          // 65535: grid.y of the angle kernel
    // Device-synchronised form (256 x 128 planes): needs the two disjoint CU sets, because persistent angle workgroups
    // that filled every CU would keep the range-Doppler workgroups they wait for from ever becoming resident.
    const char *mode = std::getenv("MMW_CHAIN_MODE");
    // (windowed chains only: the un-windowed angle variants of the persistent kernel exceed its register budget)
    // raw cubes: RAWIN variant of the 256 x 128 kernel, MODE 3 of the compile-time mixed-radix ones
    // (int16 raw cubes: the 256 x 128 producer only)
    const bool sync_shape = fused_rd_ok(S, C) || (!i16 && (raw ? rd_mixed_ct_raw_sync_supported(S, C) : rd_mixed_ct_supported(S, C)));
    p.sync = allow_sync && p.pipelined && sync_shape && p.rd_cus > 0 && p.vskip > 2 && !(mode && !std::strcmp(mode, "events"));
    // ring: ~120 MB of live planes (48 frames at 10 x 256 x 128): the ring and the streaming traffic around it share the
    // 256 MB Infinity Cache; 40-64 frames measured equal, 96 was 8 % slower
    p.ring_frames = (int)((120u << 20) / live_bytes);
    p.ring_frames = std::max(2, std::min(p.ring_frames, (int)CTL_RING_MAX));
    while ((size_t)p.ring_frames * V * S * C * sizeof(cplx<float>) >= ((size_t)1 << 31)) --p.ring_frames;   // 32-bit buffer offsets
    if (p.sync) p.chunk = n_frames;
    return p;
}

// The device-synchronised chain keeps two persistent kernels resident on disjoint halves of the chip.  Two contexts of
// ONE process doing that on the same device could starve each other (each one's consumer holding the slots the other's
// producer needs) until the bounded spins give up, so per device only one context at a time may have such work in
// flight; a second context takes the event schedule for that call.  (Two PROCESSES on one device cannot see each other:
// INTEGRATION.md.)
static std::mutex g_sync_mu;
static mmw_ctx *g_sync_owner[64] = {};
static bool g_sync_launching[64] = {};      // the owner is between acquire and the recording of its completion events
static bool sync_slot_acquire(mmw_ctx *ctx) {
    if (ctx->device < 0 || ctx->device >= 64) return true;
    std::lock_guard<std::mutex> lock(g_sync_mu);
    mmw_ctx *&owner = g_sync_owner[ctx->device];
    if (owner && owner != ctx) {
        // still launching, or still running?  (its last device-synchronised call recorded pipe_ang[0] / [1] behind the two
        // launches, under this mutex: sync_slot_launched)
        bool busy = g_sync_launching[ctx->device];
        for (int i = 0; i < 2 && !busy; ++i)
            if (owner->pipe_ang_used[i] && owner->pipe_ang[i] && hipEventQuery(owner->pipe_ang[i]) == hipErrorNotReady) busy = true;
        (void)hipGetLastError();
        if (busy) return false;
    }
    owner = ctx;
    g_sync_launching[ctx->device] = true;
    if (const int ms = opt_int(ctx, "MMW_SYNC_SLOT_TEST_SLEEP_MS", 0)) {      // test hook: widen the window between acquire and launch
        g_sync_mu.unlock();
        std::this_thread::sleep_for(std::chrono::milliseconds(ms));
        g_sync_mu.lock();
    }
    return true;
}
// the owner's launches are enqueued (or have failed): record the completion events under the mutex, end the launch window
static int sync_slot_launched(mmw_ctx *ctx, bool record) {
    std::lock_guard<std::mutex> lock(g_sync_mu);
    if (ctx->device >= 0 && ctx->device < 64 && g_sync_owner[ctx->device] == ctx) g_sync_launching[ctx->device] = false;
    if (record) {
        MMW_HIP(hipEventRecord(ctx->pipe_ang[0], ctx->q_ang));
        MMW_HIP(hipEventRecord(ctx->pipe_ang[1], ctx->q_rd));
        ctx->pipe_ang_used[0] = ctx->pipe_ang_used[1] = true;
        for (int i = 2; i < PIPE_RING_MAX; ++i) ctx->pipe_ang_used[i] = false;
    }
    return MMW_OK;
}
void mmw::sync_slot_forget(mmw_ctx *ctx) {
    std::lock_guard<std::mutex> lock(g_sync_mu);
    for (int d = 0; d < 64; ++d)
        if (g_sync_owner[d] == ctx) {
            g_sync_owner[d] = nullptr;
            g_sync_launching[d] = false;
        }
}

static int raw_args_ok(int num_rx, int num_tx) {
    MMW_REQUIRE(num_rx > 0 && num_tx > 0 && (long)num_rx * num_tx <= 4096, "bad antenna counts %d x %d", num_rx, num_tx);
    return MMW_OK;
}

// One RD launch + one angle launch for the whole call, synchronised through device counters (ChainSync).
static int chain3d_sync(mmw_ctx *ctx, const ChainPlan &plan, const void *d_cubes, RawView rv, void *d_out, int n_frames, int V,
                        int S, int C, int A_bins, int flags) {
    const size_t cube_bytes = (size_t)V * S * C * sizeof(cplx<float>);
    const long bins = (long)S * C;
    const bool mag_out = (flags & MMW_ANGLE_MAGNITUDE) != 0;
    const int tiles = angle_sync_tiles(bins, mag_out), v_live = plan.vskip > 2 ? V - 2 : V;
    MMW_REQUIRE((long)n_frames * std::max(tiles, v_live) < (1L << 30), "too many frames for one chain call");
    if (ensure_pipe_queues(ctx, plan.rd_cus) != MMW_OK) return MMW_ERR_UNSUPPORTED;
    MMW_TRY(ensure_scratch(ctx, (size_t)plan.ring_frames * cube_bytes));
    if (!ctx->chain_ctl) {
        MMW_HIP(hipMalloc((void **)&ctx->chain_ctl, CTL_WORDS * sizeof(unsigned)));
        ctx->chain_layout[0] = 0;       // forces the reset below
    }
    const long layout[6] = {V, bins, plan.vskip, plan.ring_frames, tiles, (long)(uintptr_t)ctx->scratch};
    if (std::memcmp(layout, ctx->chain_layout, sizeof(layout)) != 0) {
        // new ring layout: nothing of the old one may be in flight, counters restart from zero
        MMW_HIP(drain(ctx, Q_CHAIN));
        MMW_HIP(hipMemsetAsync(ctx->chain_ctl, 0, CTL_WORDS * sizeof(unsigned), ctx->stream));
        MMW_HIP(hipStreamSynchronize(ctx->stream));
        std::memcpy(ctx->chain_layout, layout, sizeof(layout));
        ctx->chain_g = 0;
        ctx->chain_rd_base = ctx->chain_ang_base = 0;
    }
    const bool window = !(flags & MMW_ANGLE_NO_WINDOW), shift = !(flags & MMW_ANGLE_NO_SHIFT), mag = flags & MMW_ANGLE_MAGNITUDE;
    float h[16];
    for (int i = 0; i < V; ++i) h[i] = window ? (float)np_window(TAB_HANN, i, V) : 1.f;
    ChainSync cs{};
    cs.ctl = ctx->chain_ctl;
    cs.rd_base = ctx->chain_rd_base;
    cs.ang_base = ctx->chain_ang_base;
    cs.s0 = (unsigned)(ctx->chain_g % (unsigned long long)plan.ring_frames);
    cs.u0 = (unsigned)(ctx->chain_g / (unsigned long long)plan.ring_frames);
    cs.ring = plan.ring_frames;
    cs.V = V;
    cs.vskip = plan.vskip;
    cs.v_live = v_live;
    cs.tiles = tiles;
    cs.n_frames = n_frames;
    cs.timeout = (unsigned long long)std::max(1, opt_int(ctx, "MMW_CHAIN_TIMEOUT_MS", 2000)) * 100000ull;      // 100 MHz ticks
    // order of the RD work items inside a frame: plain cubes by antenna; raw cubes rx-major, so that the ntx planes that
    // de-interleave the same raw rows are handed out back to back (their second and third read come from cache)
    {
        int n = 0;
        const bool raw = rv.ntx > 1;
        for (int i = 0; i < V && n < 16; ++i) {
            const int v = raw ? (i % rv.ntx) * rv.nrx + i / rv.ntx : i;       // i = rx * ntx + tx when raw
            if (plan.vskip > 2 && (v == 0 || v == V - 1)) continue;
            cs.vmap |= (unsigned long long)v << (4 * n++);
        }
    }
    cs.ntx = rv.ntx > 1 ? rv.ntx : 1;
    cs.nrx = rv.nrx;
    cs.i16 = rv.i16;
    cs.naps_rd = std::max(0, 32);
    cs.naps_ang = std::max(0, 4);
    const int n_rd_items = n_frames * v_live, n_ang_items = n_frames * tiles;
    const bool fused = fused_rd_ok(S, C);
    int rd_grid = std::min(plan.rd_cus, n_rd_items);
    if (!fused)     // compile-time mixed-radix producer: several workgroups per CU where they fit
        MMW_TRY(launch_rd_mixed_ct(ctx, nullptr, 0, nullptr, n_rd_items, S, C, RawView{rv.ntx > 1 ? rv.ntx : 1, rv.nrx}, nullptr, plan.rd_cus,
                                   &rd_grid, true));
    const int ang_grid = std::min((ctx->num_cu - plan.rd_cus) * 3, n_ang_items);
    hipStream_t main_stream = ctx->stream;
    MMW_HIP(hipEventRecord(ctx->pipe_begin, main_stream));
    MMW_HIP(hipStreamWaitEvent(ctx->q_rd, ctx->pipe_begin, 0));
    MMW_HIP(hipStreamWaitEvent(ctx->q_ang, ctx->pipe_begin, 0));
    // an event-mode call that is still running reads the same scratch: order behind it
    for (int i = 0; i < PIPE_RING_MAX; ++i)
        if (ctx->pipe_ang_used[i] && (ctx->pipe_ring != -1)) MMW_HIP(hipStreamWaitEvent(ctx->q_rd, ctx->pipe_ang[i], 0));
    ctx->pipe_ring = -1;            // marks "last chain call was device-synchronised" for the event-mode layout check
    ctx->pipe_slot_bytes = 0;
    ctx->pipe_pending = true;
    ctx->chain_dirty = true;
    // the counters advance by exactly these amounts whether or not the launches below succeed in full
    ctx->chain_g += (unsigned long long)n_frames;
    ctx->chain_rd_base += (unsigned)(n_rd_items + rd_grid);       // every workgroup draws one ticket past the end
    ctx->chain_ang_base += (unsigned)(n_ang_items + ang_grid);
    int rc;
    if (opt_int(ctx, "MMW_CHAIN_DIAG_SKIP_RD", 0)) {
        rc = MMW_OK;        // diagnostics: no producer -- the consumer's bounded spin must give up (tests of the abort path)
    } else {
        StreamScope on(ctx, ctx->q_rd);
        ProfScope ps(ctx, "rd");
        if (fused) rc = launch_rd_fused_sync(ctx, d_cubes, ctx->scratch, n_rd_items, cs, rd_grid);
        else rc = launch_rd_mixed_ct(ctx, d_cubes, (long)S * C, ctx->scratch, n_rd_items, S, C, RawView{1, 0}, &cs, plan.rd_cus, &rd_grid);
    }
    if (rc == MMW_OK) {
        StreamScope on(ctx, ctx->q_ang);
        ProfScope ps(ctx, "angle");
        switch (V) {
            case 4: rc = launch_angle64_sync<4>(ctx, ctx->scratch, d_out, bins, mag, h, shift, cs, ang_grid); break;
            case 8: rc = launch_angle64_sync<8>(ctx, ctx->scratch, d_out, bins, mag, h, shift, cs, ang_grid); break;
            case 12: rc = launch_angle64_sync<12>(ctx, ctx->scratch, d_out, bins, mag, h, shift, cs, ang_grid); break;
            default: rc = launch_angle64_sync<16>(ctx, ctx->scratch, d_out, bins, mag, h, shift, cs, ang_grid); break;
        }
    }
    if (rc != MMW_OK) {
        // a launch failed: the counters no longer match the host mirror; drain (the two queues this call used) and force a fresh layout next time
        (void)sync_slot_launched(ctx, false);
        (void)hipStreamSynchronize(ctx->q_rd);
        (void)hipStreamSynchronize(ctx->q_ang);
        ctx->chain_layout[0] = 0;
        return rc;
    }
    MMW_TRY(sync_slot_launched(ctx, true));
    ctx->chain_calls.push_back(ChainCall{d_cubes, d_out, rv.ntx, rv.nrx, n_frames, V, S, C, A_bins, flags, rv.i16});
    return MMW_OK;
}

static int chain3d_impl(mmw_ctx *ctx, const void *d_cubes, RawView rv, void *d_rd, void *d_out, int n_frames, int V, int S, int C,
                        int A, int flags, bool allow_sync = true) {
    const int magnitude = flags & MMW_ANGLE_MAGNITUDE;
    MMW_REQUIRE(ctx && d_cubes && d_out, "null argument");
    MMW_REQUIRE(n_frames >= 0 && V > 0 && S > 0 && C > 0 && A >= V, "bad shape (need A >= V)");
    if (n_frames == 0) return MMW_OK;
    MMW_HIP(hipSetDevice(ctx->device));
    const size_t cube_bytes = (size_t)V * S * C * sizeof(cplx<float>);
    const size_t in_frame_bytes = rv.i16 ? cube_bytes / 2 : cube_bytes;      // int16 (I, Q) cells are 4 bytes
    const size_t out_frame_bytes = (size_t)A * S * C * (magnitude ? sizeof(float) : sizeof(cplx<float>));
    ChainPlan plan = chain_plan(ctx, d_rd != nullptr, rv.ntx > 1, n_frames, V, S, C, A, flags, allow_sync, rv.i16 != 0);
    if (plan.sync && ctx->chain_calls.size() >= 256) MMW_TRY(chain_settle(ctx));     // bound the unchecked backlog
    if (plan.sync && !sync_slot_acquire(ctx))       // another context of this process has synchronised work in flight here
        plan = chain_plan(ctx, d_rd != nullptr, rv.ntx > 1, n_frames, V, S, C, A, flags, false, rv.i16 != 0);
    rv.vskip = plan.vskip;
    const bool pipelined = plan.pipelined;
    const int ring = plan.ring, rd_cus = plan.rd_cus;
    int chunk = plan.chunk;
    if (plan.sync) {
        const int rc = chain3d_sync(ctx, plan, d_cubes, rv, d_out, n_frames, V, S, C, A, flags);
        if (rc != MMW_OK) (void)sync_slot_launched(ctx, false);         // (whatever the exit path: end the launch window)
        if (rc != MMW_ERR_UNSUPPORTED) return rc;          // queues unavailable: the serial schedule below
        chunk = std::min(n_frames, 1024);
    }
    const bool queues_ok = pipelined && ensure_pipe_queues(ctx, rd_cus) == MMW_OK;
    if (!queues_ok) {
        // serial schedule (also the fallback when the chain queues cannot be created: same results)
        MMW_JOIN(ctx);
        if (pipelined) chunk = std::min(n_frames, 1024);
        void *rd_scratch = nullptr;
        if (!d_rd) {
            MMW_TRY(ensure_scratch(ctx, (size_t)chunk * cube_bytes));
            rd_scratch = ctx->scratch;
        }
        for (int f0 = 0; f0 < n_frames; f0 += chunk) {
            const int nf = std::min(chunk, n_frames - f0);
            const char *in = (const char *)d_cubes + (size_t)f0 * in_frame_bytes;
            char *rd = d_rd ? (char *)d_rd + (size_t)f0 * cube_bytes : (char *)rd_scratch;
            MMW_TRY(range_doppler_impl(ctx, in, rd, nullptr, nf, V, S, C, rv));
            MMW_TRY(angle_fft_impl(ctx, rd, (char *)d_out + (size_t)f0 * out_frame_bytes, nf, V, S, C, A, flags));
        }
        return MMW_OK;
    }
    MMW_TRY(ensure_scratch(ctx, (size_t)ring * chunk * cube_bytes));
    char *rd_scratch = (char *)ctx->scratch;
    hipStream_t main_stream = ctx->stream;
    // both queues start after whatever the caller enqueued on the context stream
    MMW_HIP(hipEventRecord(ctx->pipe_begin, main_stream));
    MMW_HIP(hipStreamWaitEvent(ctx->q_rd, ctx->pipe_begin, 0));
    MMW_HIP(hipStreamWaitEvent(ctx->q_ang, ctx->pipe_begin, 0));
    MMW_HIP(hipStreamWaitEvent(ctx->q_ang2, ctx->pipe_begin, 0));
    const int n_angq = opt_int(ctx, "MMW_ANGLE_QUEUES", 2) >= 2 ? 2 : 1;
    // The ring slots of this call overlay those of the previous (possibly still running) chain call only if the
    // layout is the same; otherwise RD must not start before every earlier angle launch has read its slot.
    const size_t slot_bytes = (size_t)chunk * cube_bytes;
    if (ctx->pipe_slot_bytes != slot_bytes || ctx->pipe_ring != ring) {
        for (int i = 0; i < PIPE_RING_MAX; ++i)
            if (ctx->pipe_ang_used[i]) MMW_HIP(hipStreamWaitEvent(ctx->q_rd, ctx->pipe_ang[i], 0));
        ctx->pipe_slot_bytes = slot_bytes;
        ctx->pipe_ring = ring;
    }
    ctx->pipe_pending = true;       // from here on work may be in flight on the chain queues, whatever the exit path
    auto fail = [&](int rc) {           // leave nothing in flight that join_pipe's events do not cover
        ctx->stream = main_stream;
        ctx->active_cus = 0;
        (void)drain(ctx, Q_CHAIN);
        return rc;
    };
#define MMW_PIPE_HIP(call)                                                                                        \
    do {                                                                                                          \
        hipError_t e_ = (call);                                                                                   \
        if (e_ != hipSuccess)                                                                                     \
            return fail(set_error(MMW_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__)); \
    } while (0)
    int k = 0;
    for (int f0 = 0; f0 < n_frames; f0 += chunk, ++k) {
        const int nf = std::min(chunk, n_frames - f0), slot = k % ring;
        char *rd = rd_scratch + (size_t)slot * slot_bytes;
        // RD(k) may overwrite its slot only after angle(k - ring) has read it
        // (also across calls: the events persist, so a back-to-back chain keeps the pipeline full)
        if (ctx->pipe_ang_used[slot]) MMW_PIPE_HIP(hipStreamWaitEvent(ctx->q_rd, ctx->pipe_ang[slot], 0));
        int rc;
        {
            StreamScope on(ctx, ctx->q_rd);
            ctx->active_cus = rd_cus > 0 ? rd_cus : ctx->num_cu;
            rc = range_doppler_impl(ctx, (const char *)d_cubes + (size_t)f0 * in_frame_bytes, rd, nullptr, nf, V, S, C, rv);
            ctx->active_cus = 0;
        }
        if (rc != MMW_OK) return fail(rc);
        MMW_PIPE_HIP(hipEventRecord(ctx->pipe_rd[slot], ctx->q_rd));
        hipStream_t q_a = (n_angq == 2 && (k & 1)) ? ctx->q_ang2 : ctx->q_ang;
        MMW_PIPE_HIP(hipStreamWaitEvent(q_a, ctx->pipe_rd[slot], 0));
        {
            StreamScope on(ctx, q_a);
            rc = angle_fft_impl(ctx, rd, (char *)d_out + (size_t)f0 * out_frame_bytes, nf, V, S, C, A, flags);
        }
        if (rc != MMW_OK) return fail(rc);
        MMW_PIPE_HIP(hipEventRecord(ctx->pipe_ang[slot], q_a));
        ctx->pipe_ang_used[slot] = true;
    }
#undef MMW_PIPE_HIP
    // The context stream joins lazily (join_pipe) at the next entry point that uses it.
    return MMW_OK;
}

// Have the device-synchronised chain calls enqueued since the last check completed?  Waits for them, reads the abort
// word and, if a bounded spin gave up (the two launches of a call did not run side by side: a tool that serialises kernel
// dispatches such as rocprofv3 --pmc, another process holding the CUs ...), resets the hand-off state and RE-RUNS the
// affected calls on the event schedule -- same kernels as the serial schedule, no device-side waiting -- so that the
// outputs the caller is about to read are complete.  MMW_CHAIN_NO_RERUN=1: report the timeout instead (MMW_ERR_HIP).
int mmw::chain_settle(mmw_ctx *ctx) {
    if (!ctx->chain_dirty) return MMW_OK;
    ctx->chain_settling = true;
    struct Done {
        mmw_ctx *c;
        ~Done() { c->chain_settling = false; }
    } done{ctx};
    if (ctx->q_rd) {        // the two queues of the device-synchronised calls only (q_ang2 may hold an event-mode call: not waited for)
        MMW_HIP(hipStreamSynchronize(ctx->q_rd));
        MMW_HIP(hipStreamSynchronize(ctx->q_ang));
    }
    MMW_HIP(hipStreamSynchronize(ctx->stream));
    unsigned aborted = 0;
    MMW_HIP(hipMemcpy(&aborted, ctx->chain_ctl + CTL_ABORT, sizeof(unsigned), hipMemcpyDeviceToHost));
    ctx->chain_dirty = false;
    std::vector<ChainCall> calls;
    calls.swap(ctx->chain_calls);
    if (!aborted) return MMW_OK;
    // counters are inconsistent (aborted workgroups leave without drawing their past-the-end ticket): fresh layout
    MMW_HIP(hipMemset(ctx->chain_ctl, 0, CTL_WORDS * sizeof(unsigned)));
    ctx->chain_layout[0] = 0;
    if (opt_int(ctx, "MMW_CHAIN_NO_RERUN", 0))
        return set_error(MMW_ERR_HIP, "chain hand-off timed out on the device (output incomplete): the range-Doppler and angle "
                         "launches of the device-synchronised chain must run concurrently -- a tool that serialises kernel "
                         "dispatches (e.g. rocprofv3 --pmc) needs MMW_CHAIN_MODE=events");
    for (const ChainCall &c : calls) {
        MMW_TRY(chain3d_impl(ctx, c.d_cubes, RawView{c.ntx, c.nrx, 0, c.i16}, nullptr, c.d_out, c.n_frames, c.V, c.S, c.C, c.A, c.flags, false));
        ++ctx->chain_fallbacks;
    }
    if (ctx->pipe_pending) {
        for (int i = 0; i < PIPE_RING_MAX; ++i)
            if (ctx->pipe_ang_used[i]) MMW_HIP(hipStreamWaitEvent(ctx->stream, ctx->pipe_ang[i], 0));
        ctx->pipe_pending = false;
    }
    MMW_HIP(hipStreamSynchronize(ctx->stream));
    return MMW_OK;
}

extern "C" {

int mmw_angle_fft(mmw_ctx *ctx, const void *d_rd, void *d_out, int n_frames, int V, int S, int C, int A,
                  int flags) {
    MMW_REQUIRE(ctx, "ctx is null");
    MMW_JOIN(ctx);
    return angle_fft_impl(ctx, d_rd, d_out, n_frames, V, S, C, A, flags);
}

int mmw_chain3d(mmw_ctx *ctx, const void *d_cubes, void *d_rd, void *d_out, int n_frames, int V, int S, int C,
                int A, int flags) {
    return chain3d_impl(ctx, d_cubes, RawView{1, 0}, d_rd, d_out, n_frames, V, S, C, A, flags);
}

int mmw_range_doppler_raw(mmw_ctx *ctx, const void *d_raw, void *d_out, int n_frames, int num_rx, int num_tx, int S,
                          int loops) {
    MMW_REQUIRE(ctx, "ctx is null");
    MMW_JOIN(ctx);
    MMW_TRY(raw_args_ok(num_rx, num_tx));
    return range_doppler_impl(ctx, d_raw, d_out, nullptr, n_frames, num_rx * num_tx, S, loops, RawView{num_tx, num_rx});
}

int mmw_chain3d_raw(mmw_ctx *ctx, const void *d_raw, void *d_rd, void *d_out, int n_frames, int num_rx, int num_tx,
                    int S, int loops, int A, int flags) {
    MMW_REQUIRE(ctx, "ctx is null");
    MMW_TRY(raw_args_ok(num_rx, num_tx));
    return chain3d_impl(ctx, d_raw, RawView{num_tx, num_rx}, d_rd, d_out, n_frames, num_rx * num_tx, S, loops, A, flags);
}

// int16 (I, Q) raw cubes [F][num_rx][S][num_tx * loops][2]: the conversion to float and the TDM de-interleave happen in the
// loads of the first kernel -- the 4-byte cells are read once, no complex64 cube is written in between.  NO UPSTREAM ORACLE
// for this sample layout (the reference gets complex cubes from the absent cpsl_datasets reader): results are defined as,
// and tested bit-identical to, mmw_virtual_array_reformat_i16 followed by the virtual-array entry point.
int mmw_range_doppler_raw_i16(mmw_ctx *ctx, const void *d_raw_i16, void *d_out, int n_frames, int num_rx, int num_tx, int S,
                              int loops) {
    MMW_REQUIRE(ctx, "ctx is null");
    MMW_JOIN(ctx);
    MMW_TRY(raw_args_ok(num_rx, num_tx));
    MMW_REQUIRE(num_tx > 1, "int16 cubes are raw TDM cubes (num_tx > 1); convert a single-tx cube with mmw_virtual_array_reformat_i16");
    return range_doppler_impl(ctx, d_raw_i16, d_out, nullptr, n_frames, num_rx * num_tx, S, loops, RawView{num_tx, num_rx, 0, 1});
}

int mmw_chain3d_raw_i16(mmw_ctx *ctx, const void *d_raw_i16, void *d_rd, void *d_out, int n_frames, int num_rx, int num_tx, int S,
                        int loops, int A, int flags) {
    MMW_REQUIRE(ctx, "ctx is null");
    MMW_TRY(raw_args_ok(num_rx, num_tx));
    MMW_REQUIRE(num_tx > 1, "int16 cubes are raw TDM cubes (num_tx > 1)");
    return chain3d_impl(ctx, d_raw_i16, RawView{num_tx, num_rx, 0, 1}, d_rd, d_out, n_frames, num_rx * num_tx, S, loops, A, flags);
}

int mmw_diag_chain_plan(mmw_ctx *ctx, int n_frames, int V, int S, int C, int A, int flags, int plan[8]) {
    MMW_REQUIRE(ctx && plan && n_frames > 0 && V > 0 && S > 0 && C > 0 && A >= V, "bad argument");
    const ChainPlan p = chain_plan(ctx, false, false, n_frames, V, S, C, A, flags);
    for (int i = 0; i < 8; ++i) plan[i] = 0;
    plan[0] = p.pipelined;
    plan[1] = p.chunk;
    plan[2] = p.ring;
    plan[3] = p.rd_cus;
    plan[4] = p.vskip > 2 ? V - 2 : V;      // range-Doppler planes transformed per frame
    plan[5] = ctx->chain_fallbacks;      // chain calls re-run on the event schedule after a hand-off timeout (mmw_chain_settle)
    plan[6] = p.sync;
    plan[7] = p.sync ? p.ring_frames : 0;
    return MMW_OK;
}

// Host-logic diagnostics that need no device (run under AddressSanitizer / UBSan by tests/cpp/host_sanitize.cpp):
// the chain schedule for a device with `num_cu` CUs, the tiling of the fused detection stage, the runs a chirp-z plan
// cuts a frequency list into.
int mmw_diag_chain_plan_nodev(int num_cu, int raw, int n_frames, int V, int S, int C, int A, int flags, int plan[8]) {
    MMW_REQUIRE(plan && num_cu > 0 && n_frames > 0 && V > 0 && S > 0 && C > 0 && A >= V, "bad argument");
    mmw_ctx fake;
    fake.num_cu = num_cu;
    const ChainPlan p = chain_plan(&fake, false, raw != 0, n_frames, V, S, C, A, flags);
    plan[0] = p.pipelined;
    plan[1] = p.chunk;
    plan[2] = p.ring;
    plan[3] = p.rd_cus;
    plan[4] = p.vskip > 2 ? V - 2 : V;
    plan[5] = 0;
    plan[6] = p.sync;
    plan[7] = p.sync ? p.ring_frames : 0;
    return MMW_OK;
}

}  // extern "C"
