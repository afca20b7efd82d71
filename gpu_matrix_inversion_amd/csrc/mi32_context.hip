// mi32_context.hip -- the context of libmat_inv_32.so: life cycle, settings, workspace, profiler.
//
// Replaces the host half of /root/reference/Matlab/mat_inv_32/mat_inv_32/
// mat_inv_32.cpp:206-395.  Where the reference re-creates platform, context,
// queue, six JIT-built programs and four buffers on every call (:238-290, 1.44 s
// of its 4.37 s at N=4096) and tears them down again (:388), this keeps one
// AOT-compiled code object, one stream and one grow-only workspace per context.
#include <cstring>
#include <new>
#include <vector>

#include "mi32_context.h"

using namespace mi32;

thread_local std::string g_last_error;

int hip_status(hipError_t e, const char *what)
{
    if (e == hipSuccess) return MI32_OK;
    g_last_error = std::string(what) + ": " + hipGetErrorString(e);
    return MI32_RUNTIME_ERROR;
}

int visible_devices(int *count)
{
    MI32_HIP(hipGetDeviceCount(count));
    if (*count > 0) return MI32_OK;
    g_last_error = "no HIP device visible";
    return MI32_RUNTIME_ERROR;
}

// Event-pair profiler: one (start, stop) pair per launch, summed per kernel class on demand.
struct EventProfiler : public Profiler {
    struct Rec { int k; hipEvent_t a, b; };
    std::vector<Rec> recs;
    std::vector<hipEvent_t> pool;
    hipEvent_t cur = nullptr;
    hipEvent_t get()
    {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }
    // Records accumulate until mi32_get_profile() collects them: a caller that leaves profiling on and never
    // collects stops recording after kMaxRecs launches instead of growing without bound.
    static constexpr size_t kMaxRecs = 1u << 20;
    void begin(int, hipStream_t s) override
    {
        if (recs.size() >= kMaxRecs) { cur = nullptr; return; }
        cur = get();
        (void)hipEventRecord(cur, s);
    }
    void end(int k, hipStream_t s) override
    {
        if (!cur) return;
        hipEvent_t b = get();
        (void)hipEventRecord(b, s);
        recs.push_back({k, cur, b});
        cur = nullptr;
    }
    void collect(double *ms, long long *count)
    {
        for (auto &r : recs) {
            float t = 0.f;
            if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&t, r.a, r.b) == hipSuccess) {
                ms[r.k] += t;
                count[r.k] += 1;
            }
            pool.push_back(r.a);
            pool.push_back(r.b);
        }
        recs.clear();
    }
    ~EventProfiler() override
    {
        for (auto &r : recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
        for (auto e : pool) (void)hipEventDestroy(e);
    }
};

int sync_all_streams(mi32_context *h)
{
    MI32_HIP(hipStreamSynchronize(h->stream));
    if (h->aux_stream) MI32_HIP(hipStreamSynchronize(h->aux_stream));
    if (h->split_stream) MI32_HIP(hipStreamSynchronize(h->split_stream));
    return MI32_OK;
}

int DeviceBuffer::ensure(mi32_context *h, size_t want)
{
    if (want <= bytes) return MI32_OK;
    if (ptr) {
        MI32_TRY(sync_all_streams(h));
        release();
    }
    MI32_HIP(hipMalloc(&ptr, want));
    bytes = want;
    return MI32_OK;
}

void DeviceBuffer::release()
{
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    bytes = 0;
}

int status_buffer(mi32_context *h, int *d_status, int batch, int **out)
{
    *out = d_status;
    if (d_status) return MI32_OK;
    const int rc = h->d_istatus.ensure(h, (size_t)batch * sizeof(int));
    *out = (int *)h->d_istatus.ptr;
    return rc;
}

int zeroed_status_buffer(mi32_context *h, int *d_status, int batch, int **out)
{
    MI32_TRY(status_buffer(h, d_status, batch, out));
    MI32_HIP(hipMemsetAsync(*out, 0, sizeof(int) * (size_t)batch, h->stream));  // MI32_OK
    return MI32_OK;
}

// ---- the diagnostic guard mode ------------------------------------------------------------------------------------------
static DeviceBuffer &zone_buffer(mi32_context *h, int owner) { return owner == WsCarve::DET ? h->det : h->ws; }

int guard_arm(mi32_context *h, const std::vector<WsCarve> &carves)
{
    const size_t G = g_ws_guard.load();
    h->zones.clear();
    if (G == 0) return MI32_OK;
    MI32_TRY(sync_all_streams(h));  // whatever an earlier call still does in the workspace
    const auto fill = [&](char *p, size_t bytes, uint32_t pattern) {
        return hip_status(hipMemsetD32Async((hipDeviceptr_t)p, (int)pattern, bytes / sizeof(uint32_t), h->stream), "guard fill");
    };
    const auto pattern_of = [](const WsRegion &r) { return r.kind == WS_VALUES ? kWsPoison : 0u; };
    for (const WsCarve &c : carves) {
        DeviceBuffer &buf = zone_buffer(h, c.owner);
        if (c.regions.empty() || c.base + c.bytes > buf.bytes) {
            g_last_error = "guard mode: a carve does not fit its buffer";
            return MI32_RUNTIME_ERROR;
        }
        char *base = (char *)buf.ptr + c.base;
        const WsRegion &first = c.regions.front();
        MI32_TRY(fill(base + first.off - G, G, pattern_of(first)));
        h->zones.push_back(WsZone{c.owner, c.part, -1, first.name, c.base + first.off - G, G, pattern_of(first)});
        for (size_t i = 0; i < c.regions.size(); ++i) {
            const WsRegion &r = c.regions[i];
            if (r.kind == WS_VALUES) MI32_TRY(fill(base + r.off, r.bytes, kWsPoison));
            MI32_TRY(fill(base + r.off + r.bytes, G, pattern_of(r)));
            h->zones.push_back(WsZone{c.owner, c.part, (int)i, r.name, c.base + r.off + r.bytes, G, pattern_of(r)});
        }
    }
    MI32_HIP(hipStreamSynchronize(h->stream));  // the route's other streams start behind the fills too
    return MI32_OK;
}

// the streams and events of a fresh context; what a failure leaves behind is mi32_destroy's
static int create_streams(mi32_context *h)
{
    MI32_HIP(hipSetDevice(h->device));
    MI32_HIP(hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
    h->stream = h->own_stream;
    if (!env_int("MI32_LOOKAHEAD", 1)) return MI32_OK;
    // Look-ahead (see blocked_invert): the half of each rank-bw update that is not on the critical
    // path runs on a second stream as a persistent kernel with one workgroup per CU on all but
    // the compute units lookahead_geometry reserves, which stay free for the panel / in-block kernels.
    // (Tried and rejected on MI355X: a plain second stream -- its workgroups fill every CU's register
    // file and the critical-path kernels queue behind them; hipExtStreamCreateWithCUMask -- it
    // serialises the two queues, 17 ms instead of 11.5.)
    hipDeviceProp_t prop;
    MI32_HIP(hipGetDeviceProperties(&prop, h->device));
    h->cu_count = prop.multiProcessorCount;
    int prio_low = 0, prio_high = 0;
    MI32_HIP(hipDeviceGetStreamPriorityRange(&prio_low, &prio_high));
    MI32_HIP(hipStreamCreateWithPriority(&h->aux_stream, hipStreamNonBlocking, prio_low));
    for (auto &ev : h->la_events) MI32_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    MI32_HIP(hipStreamCreateWithFlags(&h->split_stream, hipStreamNonBlocking));
    return MI32_OK;
}

extern "C" {

int mi32_version(void) { return 148; }
const char *mi32_last_error(void) { return g_last_error.c_str(); }

int mi32_create(mi32_handle_t *out, int device)
{
    if (!out) return MI32_BAD_SHAPE;
    *out = nullptr;
    int count = 0;
    MI32_TRY(visible_devices(&count));
    if (device < 0) MI32_HIP(hipGetDevice(&device));
    if (device >= count) {
        g_last_error = "device ordinal out of range";
        return MI32_RUNTIME_ERROR;
    }
    mi32_context *h = new (std::nothrow) mi32_context();
    if (!h) return MI32_RUNTIME_ERROR;
    h->device = device;
    const int rc = create_streams(h);
    if (rc != MI32_OK) {
        (void)mi32_destroy(h);  // g_last_error keeps the failure: nothing in there sets it
        return rc;
    }
    *out = h;
    return MI32_OK;
}

// tolerates a context that create_streams left half made: every member is null until it exists
int mi32_destroy(mi32_handle_t h)
{
    if (!h) return MI32_OK;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    for (DeviceBuffer *b : {&h->ws, &h->d_in, &h->d_out, &h->d_status, &h->d_istatus, &h->det}) b->release();
    host_copier_destroy(h->copier);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    if (h->switch_event) (void)hipEventDestroy(h->switch_event);
    for (hipStream_t s : {h->aux_stream, h->split_stream}) {
        if (!s) continue;
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
    }
    for (auto ev : h->la_events)
        if (ev) (void)hipEventDestroy(ev);
    delete h->prof;
    delete h;
    return MI32_OK;
}

int mi32_set_stream(mi32_handle_t h, void *hip_stream)
{
    if (!h) return MI32_BAD_SHAPE;
    std::lock_guard<std::mutex> lk(h->mu);
    hipStream_t ns = (hipStream_t)hip_stream;  // NULL is a stream too: HIP's default stream
    if (ns != h->stream) {
        // the workspace is shared by every call on this context: work enqueued on the new stream
        // must wait for what is still running on the old one
        MI32_HIP(hipSetDevice(h->device));
        if (!h->switch_event) MI32_HIP(hipEventCreateWithFlags(&h->switch_event, hipEventDisableTiming));
        MI32_HIP(hipEventRecord(h->switch_event, h->stream));
        MI32_HIP(hipStreamWaitEvent(ns, h->switch_event, 0));
        h->stream = ns;
    }
    return MI32_OK;
}

int mi32_set_algo(mi32_handle_t h, int algo)
{
    if (!h || algo < MI32_ALGO_AUTO || algo > MI32_ALGO_WIDE) return MI32_BAD_SHAPE;
    std::lock_guard<std::mutex> lk(h->mu);
    h->set.algo = algo;
    return MI32_OK;
}

int mi32_set_pivoting(mi32_handle_t h, int enable)
{
    if (!h) return MI32_BAD_SHAPE;
    std::lock_guard<std::mutex> lk(h->mu);
    h->set.pivoting = enable != 0;
    return MI32_OK;
}

int mi32_set_lookahead(mi32_handle_t h, int enable)
{
    if (!h) return MI32_BAD_SHAPE;
    std::lock_guard<std::mutex> lk(h->mu);
    h->set.lookahead = enable != 0;
    return MI32_OK;
}

int mi32_set_blocking(mi32_handle_t h, int panel_width, int block_width)
{
    if (!h || panel_width < 0 || block_width < 0) return MI32_BAD_SHAPE;
    std::lock_guard<std::mutex> lk(h->mu);
    h->set.panel_w = panel_width;
    h->set.block_w = block_width;
    return MI32_OK;
}

int mi32_reserve(mi32_handle_t h, int n, int batch)
{
    if (!h || n <= 0 || batch <= 0) return MI32_BAD_SHAPE;
    std::lock_guard<std::mutex> lk(h->mu);
    MI32_HIP(hipSetDevice(h->device));
    return h->ws.ensure(h, dense_route(h, h->set, n, batch, sizeof(float)).ws_bytes);
}

// tests only: waits for the context's streams, then compares every red zone the LAST call on h armed with its pattern
// (one copy per zone, of the zone alone).  A call made with the guard off, or on a one-launch route, armed none.
int mi32_debug_ws_check(mi32_handle_t h, mi32_debug_ws_report *report)
{
    if (!h || !report) return MI32_BAD_SHAPE;
    std::lock_guard<std::mutex> lk(h->mu);
    MI32_HIP(hipSetDevice(h->device));
    MI32_TRY(sync_all_streams(h));
    *report = mi32_debug_ws_report{};
    std::vector<uint32_t> host;
    for (size_t z = 0; z < h->zones.size(); ++z) {
        const WsZone &zn = h->zones[z];
        const DeviceBuffer &buf = zone_buffer(h, zn.owner);
        if (zn.off + zn.bytes > buf.bytes) return MI32_BAD_SHAPE;  // the buffer was grown since: the zones are gone
        host.resize(zn.bytes / sizeof(uint32_t));
        MI32_HIP(hipMemcpy(host.data(), (const char *)buf.ptr + zn.off, zn.bytes, hipMemcpyDeviceToHost));
        ++report->checked;
        size_t changed = 0, first = zn.bytes;
        const unsigned char *got = reinterpret_cast<const unsigned char *>(host.data());
        const unsigned char *want = reinterpret_cast<const unsigned char *>(&zn.pattern);
        for (size_t i = 0; i < zn.bytes; ++i)
            if (got[i] != want[i % sizeof(uint32_t)]) {
                if (changed++ == 0) first = i;
            }
        if (changed == 0) continue;
        if (report->damaged++ == 0) {
            report->zone = (int)z;
            report->owner = zn.owner;
            report->part = zn.part;
            report->offset = zn.region < 0 ? (long long)first - (long long)zn.bytes : (long long)first;
            report->bytes = changed;
            std::strncpy(report->name, zn.name, sizeof(report->name) - 1);
        }
    }
    return MI32_OK;
}

// tests only: stores one 32-bit word `byte_offset` bytes into red zone `zone` of the last call, so that the checker can
// be shown to notice damage.  Any offset that is not a whole word inside that zone is refused.
int mi32_debug_ws_poke(mi32_handle_t h, int zone, long long byte_offset, unsigned value)
{
    if (!h) return MI32_BAD_SHAPE;
    std::lock_guard<std::mutex> lk(h->mu);
    if (zone < 0 || (size_t)zone >= h->zones.size()) return MI32_BAD_SHAPE;
    const WsZone &zn = h->zones[(size_t)zone];
    const DeviceBuffer &buf = zone_buffer(h, zn.owner);
    if (byte_offset < 0 || byte_offset % 4 != 0 || (unsigned long long)byte_offset + sizeof(uint32_t) > zn.bytes ||
        zn.off + zn.bytes > buf.bytes)
        return MI32_BAD_SHAPE;
    MI32_HIP(hipSetDevice(h->device));
    MI32_TRY(sync_all_streams(h));
    const uint32_t word = value;
    MI32_HIP(hipMemcpy((char *)buf.ptr + zn.off + (size_t)byte_offset, &word, sizeof(word), hipMemcpyHostToDevice));
    return MI32_OK;
}

int mi32_set_profiling(mi32_handle_t h, int enable)
{
    if (!h) return MI32_BAD_SHAPE;
    std::lock_guard<std::mutex> lk(h->mu);
    MI32_HIP(hipSetDevice(h->device));
    if (enable && !h->prof) h->prof = new (std::nothrow) EventProfiler();
    if (!enable && h->prof) {
        MI32_HIP(hipStreamSynchronize(h->stream));
        delete h->prof;
        h->prof = nullptr;
    }
    return MI32_OK;
}

int mi32_get_profile(mi32_handle_t h, double *ms_per_class, long long *launches_per_class, int nclasses)
{
    if (!h || !ms_per_class || !launches_per_class || nclasses < KC_COUNT) return MI32_BAD_SHAPE;
    std::lock_guard<std::mutex> lk(h->mu);
    for (int i = 0; i < nclasses; ++i) { ms_per_class[i] = 0.0; launches_per_class[i] = 0; }
    if (!h->prof) return MI32_OK;
    MI32_HIP(hipSetDevice(h->device));
    static_cast<EventProfiler *>(h->prof)->collect(ms_per_class, launches_per_class);
    return MI32_OK;
}

}  // extern "C"
