// libmmwgpu.so -- extern "C" entry points declared in include/mmwgpu.h: version and errors, devices, contexts, memory, the copy
// queue and events, timers, the profile, options.  No kernels here; the other entry points are in the mmw_tu_*.hip unit of their domain.
#include "mmw_entry.h"

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <memory>

using namespace mmw;

int mmw::env_int(const char *name, int dflt) {
    const char *s = std::getenv(name);
    return (s && *s) ? std::atoi(s) : dflt;
}

extern "C" {

const char *mmw_version(void) { return "mmwgpu 0.3 (gfx950)"; }
int mmw_abi_version(void) { return MMWGPU_ABI_VERSION; }
const char *mmw_last_error(void) { return g_last_error.c_str(); }

int mmw_device_count(int *count) {
    MMW_REQUIRE(count, "count is null");
    MMW_HIP(hipGetDeviceCount(count));
    return MMW_OK;
}

int mmw_device_info(int device, char *name, int name_len, char *arch, int arch_len, int *num_cu,
                    size_t *total_mem) {
    hipDeviceProp_t prop;
    MMW_HIP(hipGetDeviceProperties(&prop, device));
    if (name && name_len > 0) {
        // hipDeviceProp_t::name comes back empty on this image's MI355X boxes: ask the runtime's other query, and failing that
        // name the product from what identifies it (gfx950 with 256 compute units is the MI355X / MI350X package)
        char buf[256] = {0};
        snprintf(buf, sizeof(buf), "%s", prop.name);
        if (!buf[0] && hipDeviceGetName(buf, (int)sizeof(buf), device) != hipSuccess) buf[0] = 0;
        (void)hipGetLastError();
        if (!buf[0] && !std::strncmp(prop.gcnArchName, "gfx950", 6))
            snprintf(buf, sizeof(buf), "AMD Instinct MI355X (identified by arch %s, %d CUs, %.0f GiB: the runtime reports no name)",
                     prop.gcnArchName, prop.multiProcessorCount, (double)prop.totalGlobalMem / (1 << 30));
        snprintf(name, name_len, "%s", buf);
    }
    if (arch && arch_len > 0) snprintf(arch, arch_len, "%s", prop.gcnArchName);
    if (num_cu) *num_cu = prop.multiProcessorCount;
    if (total_mem) *total_mem = prop.totalGlobalMem;
    return MMW_OK;
}

int mmw_ctx_create(mmw_ctx **out, int device) {
    MMW_REQUIRE(out, "out is null");
    int n = 0;
    MMW_HIP(hipGetDeviceCount(&n));
    MMW_REQUIRE(device >= 0 && device < n, "device %d out of range (%d visible)", device, n);
    MMW_HIP(hipSetDevice(device));
    // released to the caller on success; any early return below tears the half-built context down again
    std::unique_ptr<mmw_ctx, int (*)(mmw_ctx *)> c(new mmw_ctx(), mmw_ctx_destroy);
    c->device = device;
    hipDeviceProp_t prop;
    MMW_HIP(hipGetDeviceProperties(&prop, device));
    c->num_cu = prop.multiProcessorCount;
    MMW_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    MMW_HIP(hipEventCreate(&c->t0));
    MMW_HIP(hipEventCreate(&c->t1));
    *out = c.release();
    return MMW_OK;
}

int mmw_ctx_destroy(mmw_ctx *ctx) {
    if (!ctx) return MMW_OK;
    sync_slot_forget(ctx);
    (void)hipSetDevice(ctx->device);
    (void)drain_all(ctx);       // first: a deferred detection tail, chain work and copies are not joined into the main stream
    for (auto &kv : ctx->tables) (void)hipFree(kv.second);
    for (auto &pl : ctx->czt_plans) {
        (void)hipFree(pl.d_segs);
        (void)hipFree(pl.d_tabs);
    }
    for (void *p : ctx->owned) (void)hipFree(p);
    if (ctx->scratch) (void)hipFree(ctx->scratch);
    if (ctx->capon_z) (void)hipFree(ctx->capon_z);
    if (ctx->capon_dop_tab) (void)hipFree(ctx->capon_dop_tab);
    if (ctx->chain_ctl) (void)hipFree(ctx->chain_ctl);
    if (ctx->help_sync) (void)hipFree(ctx->help_sync);
    for (void *p : ctx->host_owned) (void)hipHostFree(p);
    drain_profile(ctx);
    for (int g = 0; g < Q_GROUPS; ++g) (void)destroy_queues(ctx, g);
    // every event of the context (a half-built one has nulls among them)
    std::vector<hipEvent_t> events = {ctx->pipe_begin, ctx->det_begin, ctx->det_rd_done, ctx->det_scr_done, ctx->side_fork, ctx->side_join,
                                      ctx->tail_done, ctx->help_begin, ctx->help_done, ctx->t0, ctx->t1};
    events.insert(events.end(), ctx->pipe_rd, ctx->pipe_rd + PIPE_RING_MAX);
    events.insert(events.end(), ctx->pipe_ang, ctx->pipe_ang + PIPE_RING_MAX);
    events.insert(events.end(), ctx->ev_pool.begin(), ctx->ev_pool.end());
    for (hipEvent_t e : events)
        if (e) (void)hipEventDestroy(e);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return MMW_OK;
}

int mmw_sync(mmw_ctx *ctx) {
    MMW_REQUIRE(ctx, "ctx is null");
    MMW_JOIN(ctx);
    MMW_HIP(hipStreamSynchronize(ctx->stream));     // (MMW_JOIN above has settled any device-synchronised chain call)
    return MMW_OK;
}

int mmw_malloc(mmw_ctx *ctx, void **d_ptr, size_t bytes) {
    MMW_REQUIRE(ctx && d_ptr, "null argument");
    MMW_HIP(hipSetDevice(ctx->device));
    void *p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess)
        return set_error(MMW_ERR_NOMEM, "hipMalloc(%zu) failed", bytes);
    ctx->owned.push_back(p);
    *d_ptr = p;
    return MMW_OK;
}

int mmw_free(mmw_ctx *ctx, void *d_ptr) {
    MMW_REQUIRE(ctx, "ctx is null");
    MMW_JOIN(ctx);
    if (!d_ptr) return MMW_OK;
    auto it = std::find(ctx->owned.begin(), ctx->owned.end(), d_ptr);
    MMW_REQUIRE(it != ctx->owned.end(), "pointer was not allocated by this context");
    MMW_HIP(hipStreamSynchronize(ctx->stream));
    MMW_HIP(hipFree(d_ptr));
    ctx->owned.erase(it);
    return MMW_OK;
}

int mmw_memcpy_h2d(mmw_ctx *ctx, void *d_dst, const void *h_src, size_t bytes) {
    MMW_REQUIRE(ctx && (bytes == 0 || (d_dst && h_src)), "null argument");
    MMW_JOIN(ctx);
    if (!bytes) return MMW_OK;
    MMW_HIP(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream));
    MMW_HIP(hipStreamSynchronize(ctx->stream));
    return MMW_OK;
}

int mmw_memcpy_d2h(mmw_ctx *ctx, void *h_dst, const void *d_src, size_t bytes) {
    MMW_REQUIRE(ctx && (bytes == 0 || (h_dst && d_src)), "null argument");
    MMW_JOIN(ctx);
    if (!bytes) return MMW_OK;
    MMW_HIP(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    MMW_HIP(hipStreamSynchronize(ctx->stream));
    return MMW_OK;
}

int mmw_memset(mmw_ctx *ctx, void *d_dst, int value, size_t bytes) {
    MMW_REQUIRE(ctx && (bytes == 0 || d_dst), "null argument");
    MMW_JOIN(ctx);
    if (!bytes) return MMW_OK;
    MMW_HIP(hipMemsetAsync(d_dst, value, bytes, ctx->stream));
    return MMW_OK;
}

// ------------------------------------------------------------------ host streaming (pinned staging, copy queue, events)
// A frame loop that receives its cubes on the host (scripts/test_vel_estimation.py:145-151 in the reference) uploads chunk
// k + 1 while chunk k is processed: pinned host blocks, a second queue for the copies, events to order the two.
int mmw_host_alloc(mmw_ctx *ctx, void **h_ptr, size_t bytes) {
    MMW_REQUIRE(ctx && h_ptr, "null argument");
    MMW_HIP(hipSetDevice(ctx->device));
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess)
        return set_error(MMW_ERR_NOMEM, "hipHostMalloc(%zu) failed", bytes);
    ctx->host_owned.push_back(p);
    *h_ptr = p;
    return MMW_OK;
}

int mmw_host_free(mmw_ctx *ctx, void *h_ptr) {
    MMW_REQUIRE(ctx, "ctx is null");
    if (!h_ptr) return MMW_OK;
    auto it = std::find(ctx->host_owned.begin(), ctx->host_owned.end(), h_ptr);
    MMW_REQUIRE(it != ctx->host_owned.end(), "pointer was not allocated by mmw_host_alloc of this context");
    MMW_HIP(hipSetDevice(ctx->device));
    MMW_HIP(drain(ctx, Q_COPY));
    MMW_HIP(hipStreamSynchronize(ctx->stream));
    MMW_HIP(hipHostFree(h_ptr));
    ctx->host_owned.erase(it);
    return MMW_OK;
}

static int queue_of(mmw_ctx *ctx, int queue, hipStream_t *out) {
    MMW_REQUIRE(queue == MMW_QUEUE_COMPUTE || queue == MMW_QUEUE_COPY, "queue must be MMW_QUEUE_COMPUTE or MMW_QUEUE_COPY");
    MMW_HIP(hipSetDevice(ctx->device));
    if (queue == MMW_QUEUE_COPY && !ctx->q_copy) MMW_HIP(hipStreamCreateWithFlags(&ctx->q_copy, hipStreamNonBlocking));
    *out = queue == MMW_QUEUE_COPY ? ctx->q_copy : ctx->stream;
    return MMW_OK;
}

int mmw_memcpy_async(mmw_ctx *ctx, void *dst, const void *src, size_t bytes, int to_host, int queue) {
    MMW_REQUIRE(ctx && (bytes == 0 || (dst && src)), "null argument");
    hipStream_t q;
    MMW_TRY(queue_of(ctx, queue, &q));
    if (queue == MMW_QUEUE_COMPUTE) MMW_JOIN(ctx);
    if (!bytes) return MMW_OK;
    MMW_HIP(hipMemcpyAsync(dst, src, bytes, to_host ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice, q));
    return MMW_OK;
}

int mmw_event_create(mmw_ctx *ctx, void **event) {
    MMW_REQUIRE(ctx && event, "null argument");
    MMW_HIP(hipSetDevice(ctx->device));
    hipEvent_t e = nullptr;
    MMW_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    *event = e;
    return MMW_OK;
}

int mmw_event_destroy(mmw_ctx *ctx, void *event) {
    MMW_REQUIRE(ctx, "ctx is null");
    if (event) MMW_HIP(hipEventDestroy((hipEvent_t)event));
    return MMW_OK;
}

int mmw_event_record(mmw_ctx *ctx, void *event, int queue) {
    MMW_REQUIRE(ctx && event, "null argument");
    hipStream_t q;
    MMW_TRY(queue_of(ctx, queue, &q));
    if (queue == MMW_QUEUE_COMPUTE) MMW_JOIN(ctx);          // chain work of the context is part of "the compute queue so far"
    MMW_HIP(hipEventRecord((hipEvent_t)event, q));
    return MMW_OK;
}

int mmw_queue_wait_event(mmw_ctx *ctx, int queue, void *event) {
    MMW_REQUIRE(ctx && event, "null argument");
    hipStream_t q;
    MMW_TRY(queue_of(ctx, queue, &q));
    MMW_HIP(hipStreamWaitEvent(q, (hipEvent_t)event, 0));
    return MMW_OK;
}

int mmw_event_sync(mmw_ctx *ctx, void *event) {
    MMW_REQUIRE(ctx && event, "null argument");
    MMW_HIP(hipEventSynchronize((hipEvent_t)event));
    return MMW_OK;
}

int mmw_timer_start(mmw_ctx *ctx) {
    MMW_REQUIRE(ctx, "ctx is null");
    MMW_JOIN(ctx);
    MMW_HIP(hipEventRecord(ctx->t0, ctx->stream));
    return MMW_OK;
}

int mmw_timer_stop(mmw_ctx *ctx, float *elapsed_ms) {
    MMW_REQUIRE(ctx && elapsed_ms, "null argument");
    MMW_JOIN(ctx);
    MMW_HIP(hipEventRecord(ctx->t1, ctx->stream));
    MMW_HIP(hipEventSynchronize(ctx->t1));
    MMW_HIP(hipEventElapsedTime(elapsed_ms, ctx->t0, ctx->t1));
    return MMW_OK;
}

int mmw_profile_enable(mmw_ctx *ctx, int on) {
    MMW_REQUIRE(ctx, "ctx is null");
    ctx->profiling = on != 0;
    ctx->prof_every = on > 1 ? on : 1;      // on = n > 1: sample every n-th launch group per family
    ctx->prof_seen.clear();
    return MMW_OK;
}

int mmw_profile_reset(mmw_ctx *ctx) {
    MMW_REQUIRE(ctx, "ctx is null");
    drain_profile(ctx);
    ctx->prof.clear();
    return MMW_OK;
}

int mmw_profile_get(mmw_ctx *ctx, const char *family, float *total_ms, int *launches) {
    MMW_REQUIRE(ctx && family, "null argument");
    drain_profile(ctx);
    auto it = ctx->prof.find(family);
    if (total_ms) *total_ms = it == ctx->prof.end() ? 0.f : (float)it->second.total_ms;
    if (launches) *launches = it == ctx->prof.end() ? 0 : it->second.launches;
    return MMW_OK;
}

int mmw_diag_set_option(mmw_ctx *ctx, const char *name, int value) {
    MMW_REQUIRE(ctx && name && *name, "null argument");
    if (value == INT_MIN) ctx->opts.erase(name);
    else ctx->opts[name] = value;
    return MMW_OK;
}

}  // extern "C"
