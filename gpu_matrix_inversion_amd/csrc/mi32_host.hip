// mi32_host.hip -- host runtime of libmat_inv_32.so: context, workspace cache,
// the C ABI of include/mat_inv_32_c.h and the C++ drop-in of include/mat_inv_32.h.
//
// Replaces the host half of /root/reference/Matlab/mat_inv_32/mat_inv_32/
// mat_inv_32.cpp:206-395.  Where the reference re-creates platform, context,
// queue, six JIT-built programs and four buffers on every call (:238-290, 1.44 s
// of its 4.37 s at N=4096) and tears them down again (:388), this keeps one
// AOT-compiled code object, one stream and one grow-only workspace per context.
#include <chrono>
#include <condition_variable>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include <sys/mman.h>

#include "mat_inv_32.h"
#include "mat_inv_64.h"
#include "mat_inv_bench.h"
#include "mi32_internal.h"

using namespace mi32;

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

// Host <-> device copies of the host-pointer entry points.  The caller's vectors are pageable memory: a plain
// hipMemcpy moves 64 MiB (N = 4096) in 4.6 ms each way on this platform, while the DMA engine needs 1.2 ms from
// pinned memory and pinning the caller's pages (hipHostRegister) costs 4 ms by itself (tools/h2d_probe.hip).
// So: kLanes host threads, each with two pinned 2 MiB buffers and a stream of its own, memcpy chunk i + 1 into one
// buffer while the DMA engine drains chunk i from the other: N = 4096 end to end 16.8-21.6 -> 12.4 ms (8.8 ms of it
// compute), N = 8192 65 -> 52 ms.
struct HostCopier {
    static constexpr int kLanes = 6;
    static constexpr size_t kChunk = 2u << 20;
    static constexpr size_t kMinBytes = 32u << 20;  // below this a plain hipMemcpyAsync wins (measured cross-over)
    char *pin[kLanes][2] = {};
    hipStream_t stream[kLanes] = {};
    hipEvent_t ev[kLanes][2] = {};
    // the lanes are persistent threads (a fresh thread's first HIP call costs more than the copy it would do)
    std::thread th[kLanes];
    std::mutex mu;
    std::condition_variable cv_job, cv_done;
    unsigned long long job_id = 0;  // incremented per job; a lane runs job j when job_id == j > its last one
    int pending = 0;
    bool quit = false;
    int device = 0;
    void *j_dev = nullptr, *j_host = nullptr;
    size_t j_bytes = 0;
    bool j_to_device = true;
    hipError_t j_err[kLanes];
    bool ready = false;

    hipError_t init(int dev)
    {
        if (ready) return hipSuccess;
        device = dev;
        for (int t = 0; t < kLanes; ++t) {
            hipError_t e = hipStreamCreateWithFlags(&stream[t], hipStreamNonBlocking);
            if (e != hipSuccess) return e;
            for (int q = 0; q < 2; ++q) {
                if ((e = hipHostMalloc((void **)&pin[t][q], kChunk, hipHostMallocDefault)) != hipSuccess) return e;
                if ((e = hipEventCreateWithFlags(&ev[t][q], hipEventDisableTiming)) != hipSuccess) return e;
            }
        }
        for (int t = 0; t < kLanes; ++t) th[t] = std::thread([this, t]() { lane_main(t); });
        ready = true;
        return hipSuccess;
    }
    void destroy()
    {
        if (!ready) return;
        {
            std::lock_guard<std::mutex> lk(mu);
            quit = true;
        }
        cv_job.notify_all();
        for (int t = 0; t < kLanes; ++t)
            if (th[t].joinable()) th[t].join();
        for (int t = 0; t < kLanes; ++t) {
            for (int q = 0; q < 2; ++q) {
                if (pin[t][q]) (void)hipHostFree(pin[t][q]);
                if (ev[t][q]) (void)hipEventDestroy(ev[t][q]);
            }
            if (stream[t]) (void)hipStreamDestroy(stream[t]);
        }
        ready = false;
    }
    void lane_main(int t)
    {
        (void)hipSetDevice(device);
        unsigned long long done_id = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(mu);
                cv_job.wait(lk, [&]() { return quit || job_id != done_id; });
                if (quit) return;
                done_id = job_id;
            }
            j_err[t] = lane_copy(t);
            {
                std::lock_guard<std::mutex> lk(mu);
                if (--pending == 0) cv_done.notify_all();
            }
        }
    }
    hipError_t lane_copy(int t)
    {
        const size_t bytes = j_bytes;
        const size_t nchunks = (bytes + kChunk - 1) / kChunk;
        char *dev = (char *)j_dev, *host = (char *)j_host;
        auto span = [&](size_t c, size_t &off, size_t &len) { off = c * kChunk; len = bytes - off < kChunk ? bytes - off : kChunk; };
        hipError_t e = hipSuccess;
        size_t k = 0;  // this lane's chunk counter
        if (j_to_device) {
            for (size_t c = t; c < nchunks && e == hipSuccess; c += kLanes, ++k) {
                size_t off, len;
                span(c, off, len);
                const int q = (int)(k & 1);
                if (k >= 2) e = hipEventSynchronize(ev[t][q]);  // the DMA that last read this buffer
                if (e != hipSuccess) break;
                std::memcpy(pin[t][q], host + off, len);
                e = hipMemcpyAsync(dev + off, pin[t][q], len, hipMemcpyHostToDevice, stream[t]);
                if (e == hipSuccess) e = hipEventRecord(ev[t][q], stream[t]);
            }
        } else {
            size_t off, len;
            if ((size_t)t < nchunks) {
                span(t, off, len);
                e = hipMemcpyAsync(pin[t][0], dev + off, len, hipMemcpyDeviceToHost, stream[t]);
                if (e == hipSuccess) e = hipEventRecord(ev[t][0], stream[t]);
            }
            for (size_t c = t; c < nchunks && e == hipSuccess; c += kLanes, ++k) {
                const int q = (int)(k & 1);
                if (c + kLanes < nchunks) {  // the next chunk of this lane into the other buffer
                    size_t noff, nlen;
                    span(c + kLanes, noff, nlen);
                    e = hipMemcpyAsync(pin[t][q ^ 1], dev + noff, nlen, hipMemcpyDeviceToHost, stream[t]);
                    if (e == hipSuccess) e = hipEventRecord(ev[t][q ^ 1], stream[t]);
                    if (e != hipSuccess) break;
                }
                span(c, off, len);
                e = hipEventSynchronize(ev[t][q]);
                if (e != hipSuccess) break;
                std::memcpy(host + off, pin[t][q], len);
            }
        }
        if (e == hipSuccess) e = hipStreamSynchronize(stream[t]);
        return e;
    }
    // to_device: dev <- host, else host <- dev.  Synchronous: returns when every byte has arrived.
    hipError_t run(void *dev, void *host, size_t bytes, bool to_device)
    {
        std::unique_lock<std::mutex> lk(mu);
        j_dev = dev; j_host = host; j_bytes = bytes; j_to_device = to_device;
        pending = kLanes;
        ++job_id;
        cv_job.notify_all();
        cv_done.wait(lk, [&]() { return pending == 0; });
        for (int t = 0; t < kLanes; ++t)
            if (j_err[t] != hipSuccess) return j_err[t];
        return hipSuccess;
    }
};

struct mi32_context {
    int device = 0;
    HostCopier copier;
    EventProfiler *prof = nullptr;
    hipEvent_t switch_event = nullptr;
    hipStream_t aux_stream = nullptr;   // look-ahead half of the rank-bw updates (lowest priority)
    hipStream_t split_stream = nullptr; // second half of a split batch (same priority as the main stream)
    hipEvent_t la_events[8] = {};
    int cu_count = 0;
    bool lookahead = true;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    void *ws = nullptr;
    size_t ws_bytes = 0;
    int algo = MI32_ALGO_AUTO;
    bool pivoting = true;  // false: the reference's no-pivot variant (the diagonal entry is every step's pivot)
    int panel_w = 0;
    int block_w = 0;
    // staging for the host-pointer entry points
    float *d_in = nullptr, *d_out = nullptr;
    int *d_status = nullptr;
    size_t io_floats = 0, status_ints = 0;  // io_floats: capacity of d_in / d_out in 4-byte units
    // status words of device-resident calls that pass no status buffer: the kernels always have one to flag
    // a bad pivot or a lost panel partner in (a given-up matrix is then skipped and comes out as NaN)
    int *d_istatus = nullptr;
    size_t istatus_ints = 0;
    std::mutex mu;
};

// A variable-size batch plan (mi32_vbatch_create): immutable after creation.  The orders and the sorted member list
// are the only device memory it owns, 8 bytes per member.
static constexpr int kVbatchClasses = 8;
struct mi32_vbatch {
    int device = 0;
    int batch = 0;
    int class_begin[kVbatchClasses + 1] = {};  // class k takes d_members[class_begin[k] .. class_begin[k + 1])
    // the members of order n are d_members[order_begin[n] .. order_begin[n + 1]), n = 1 ... 128 (host only: the solve's
    // launches follow the width n + columns, not the order's class)
    int order_begin[kWorkgroupMaxOrder + 2] = {};
    int *d_orders = nullptr;   // int[batch], the caller's member order
    int *d_members = nullptr;  // int[batch], member indices in ascending order of their orders (stable)
};

static thread_local std::string g_last_error;
// Host-pointer entry points (fp32 and fp64 alike) share the default context's staging buffers and the two
// timing words below: ONE mutex serialises them all.
static std::mutex g_host_call_mu;
static double g_last_total = 0.0, g_last_compute = 0.0;  // guarded by g_host_call_mu

static int fail(hipError_t e, const char *what)
{
    g_last_error = std::string(what) + ": " + hipGetErrorString(e);
    return MI32_RUNTIME_ERROR;
}
#define MI32_HIP(call)                                  \
    do {                                                \
        hipError_t e__ = (call);                        \
        if (e__ != hipSuccess) return fail(e__, #call); \
    } while (0)

static int env_int(const char *name, int dflt)
{
    const char *s = std::getenv(name);
    return (s && *s) ? std::atoi(s) : dflt;
}

// The look-ahead half of a single large matrix (blocked_invert): how many CUs it runs on and whether it shares them.
// Measured on MI355X (256 CUs), ms per inversion, "free CUs / LDS KB per look-ahead workgroup":
//   N  4096:  32/84 8.81   32/156 8.66   64/156 8.53   96/156 8.51   128/156 8.49
//   N  6144:  16/84 18.96  32/84 17.88   32/156 17.78  64/156 17.01  128/156 17.33
//   N  8192:  16/84 30.6   32/156 30.3   64/156 29.5
//   N 10240:  16/84 41.7   32/84 40.6    32/156 42.1   64/156 40.9   128/156 50.2
//   N 12288:  16/84 58.5   32/84 57.9    32/156 59.0   64/156 60.8   128/156 84.7
//   N 16384:  16/84 107.5  32/84 111.4   32/156 125.4  64/156 124.3  (8/84 107.0, 5/84 137.7: the shared panels starve)
// Round 3 (reference-order strips, bw = 256 everywhere), same notation:
//   N  8192:  8/84 34.8   16/84 34.9   32/84 33.2   64/84 33.9   32/156 35.6   64/156 33.9
//   N 12288:  8/84 70.5   16/84 70.4   32/84 66.9   64/84 67.9   32/156 72.8   64/156 68.4
//   N 16384:  8/84 119.1  16/84 121.8  32/84 125.4  64/84 141.9  32/156 134.1
//   (two or three look-ahead workgroups per CU, 76 / 50 KB each: 8192 37.7, 12288 77.8, 16384 143-145: the shared panels starve)
// Up to ~7168 rows the half is short against the panel phase: it gets few CUs, all to itself, and the panel chain
// keeps the rest undisturbed; above, every block waits for the half: it gets all but 32 / 16 CUs and shares them.
static void lookahead_geometry(int cus, int n, int *workgroups, bool *exclusive)
{
    int reserve;
    bool excl;
    if (n < 5120) { reserve = cus / 2; excl = true; }
    else if (n <= 7168) { reserve = cus / 4; excl = true; }
    else if (n <= 14336) { reserve = cus / 8; excl = false; }
    else { reserve = cus / 32; excl = false; }
    if (reserve < 1) reserve = 1;
    if (reserve > cus - 1) reserve = cus - 1;
    *workgroups = cus - reserve;
    *exclusive = excl;
}

// MI32_ALGO_WORKGROUP up to 128 rows: the register-resident path takes the orders it holds, so that one setting serves
// orders on both sides of 64; above 128 it resolves to what AUTO resolves to
static int workgroup_or_resident(int n) { return n <= kResidentMaxOrder ? MI32_ALGO_RESIDENT : MI32_ALGO_WORKGROUP; }

static int resolve_algo(const mi32_context *h, int n)
{
    int algo = h ? h->algo : MI32_ALGO_AUTO;
    if (algo == MI32_ALGO_AUTO) algo = env_int("MI32_ALGO", MI32_ALGO_AUTO);
    // the register-resident path holds orders up to 64; above, RESIDENT resolves to what AUTO resolves to
    if (algo == MI32_ALGO_RESIDENT && n <= kResidentMaxOrder) return algo;
    if (algo == MI32_ALGO_WORKGROUP && n <= kWorkgroupMaxOrder) return workgroup_or_resident(n);
    // the no-pivot variant (fp32): blocked from 512 rows on (the W x W diagonal block is its whole "panel")
    const int cross = (h && !h->pivoting) ? 512 : 32;
    if (algo != MI32_ALGO_SWEEP && algo != MI32_ALGO_BLOCKED) algo = (n >= cross) ? MI32_ALGO_BLOCKED : MI32_ALGO_SWEEP;  // measured cross-over on MI355X
    if (algo == MI32_ALGO_BLOCKED && !blocked_supported(n)) algo = MI32_ALGO_SWEEP;  // panel would not fit in registers
    return algo;
}
static BlockedPlan plan_blocked(const mi32_context *h, int n, int batch)
{
    int w = h && h->panel_w ? h->panel_w : env_int("MI32_PANEL_W", 0);
    int bw = h && h->block_w ? h->block_w : env_int("MI32_BLOCK_W", 0);
    if (bw == 0) {
        // A single matrix is bound by the pivot chain and bw = 256 gives the rank-bw update its best
        // arithmetic intensity.  A batch that fills the GPU is bound by the HBM traffic of the in-block
        // updates (np x bw re-written per sub-panel): bw = 128 halves it (measured 64 x 2048^2:
        // 23.0 ms vs 24.7 ms; single 4096^2: 11.4 ms vs 11.2 ms).
        const double elems = (double)batch * (double)n * (double)n;
        bw = (batch >= 8 && elems >= 64.0 * 1024.0 * 1024.0) ? 128 : 256;
        // (Rounds 1-2 ran N > 14336 with bw = 512 for the rank-bw update's sake: 120 instead of 114 TFLOP/s.  With the
        // pivot-row strips of round 3 an in-block update tile costs more and there are twice as many per sub-panel at
        // 512: 16384^2 122 ms at 256, 126 at 384, 140 at 512; 12288^2 65.5 vs 75.9; 8192^2 33.9 vs 38.0.)
    }
    return make_blocked_plan(n, w, bw, batch);
}
static size_t ws_bytes_for(const mi32_context *h, int n, int batch, int algo)
{
    size_t a;
    if (algo == MI32_ALGO_RESIDENT || algo == MI32_ALGO_WORKGROUP) a = 0;  // no working copy: only the residual check needs a workspace
    else if (algo == MI32_ALGO_SWEEP) a = sweep_workspace_bytes(make_sweep_plan(n), batch, sizeof(float));
    else {
        const BlockedPlan p = plan_blocked(h, n, batch);
        // a batch that may be split in two halves (mi32_inv_device) carves one workspace per half
        a = blocked_workspace_bytes(p, (batch + 1) / 2) + blocked_workspace_bytes(p, batch - (batch + 1) / 2);
        const size_t whole = blocked_workspace_bytes(p, batch);
        if (whole > a) a = whole;
    }
    size_t r = residual_workspace_bytes(n, batch);
    return a > r ? a : r;
}

static int sync_all_streams(mi32_context *h)
{
    MI32_HIP(hipStreamSynchronize(h->stream));
    if (h->aux_stream) MI32_HIP(hipStreamSynchronize(h->aux_stream));
    if (h->split_stream) MI32_HIP(hipStreamSynchronize(h->split_stream));
    return MI32_OK;
}

// the status buffer a device-resident call runs with: the caller's, or the context's own
static int status_buffer(mi32_context *h, int *d_status, int batch, int **out)
{
    *out = d_status;
    if (d_status) return MI32_OK;
    if ((size_t)batch > h->istatus_ints) {
        if (h->d_istatus) {
            int rc = sync_all_streams(h);
            if (rc != MI32_OK) return rc;
            MI32_HIP(hipFree(h->d_istatus));
            h->d_istatus = nullptr;
            h->istatus_ints = 0;
        }
        MI32_HIP(hipMalloc((void **)&h->d_istatus, (size_t)batch * sizeof(int)));
        h->istatus_ints = (size_t)batch;
    }
    *out = h->d_istatus;
    return MI32_OK;
}

static int ensure_ws(mi32_context *h, size_t bytes)
{
    if (bytes <= h->ws_bytes) return MI32_OK;
    if (h->ws) {
        int rc = sync_all_streams(h);
        if (rc != MI32_OK) return rc;
        MI32_HIP(hipFree(h->ws));
        h->ws = nullptr;
        h->ws_bytes = 0;
    }
    MI32_HIP(hipMalloc(&h->ws, bytes));
    h->ws_bytes = bytes;
    return MI32_OK;
}

// A uniform batch on the one-launch paths: the register-resident kernels up to kResidentMaxOrder rows, the
// workgroup-resident ones above (n <= kWorkgroupMaxOrder is the caller's business).  det: where the determinants go,
// empty for none; d_inv may be null only with one.  The caller holds h->mu and has set the device.
template <typename T>
static int one_launch_device(mi32_context *h, const T *d_a, int n, int batch, T *d_inv, int *d_status, const DetOut det)
{
    const int rc = status_buffer(h, d_status, batch, &d_status);
    if (rc != MI32_OK) return rc;
    hipError_t e = hipMemsetAsync(d_status, 0, sizeof(int) * (size_t)batch, h->stream);  // MI32_OK
    if (e == hipSuccess)
        e = n <= kResidentMaxOrder
                ? resident_invert(d_a, d_inv, n, batch, d_status, det, h->stream, h->prof, h->pivoting)
                : workgroup_invert(d_a, d_inv, n, batch, d_status, det, h->stream, h->prof, h->pivoting);
    if (e != hipSuccess) return fail(e, "kernel launch");
    return MI32_OK;
}

// A X = B on the one-launch paths.  A call's nrhs columns are cut into chunks of at most solve_chunk_cols(n): what is
// left of one 64-lane group beside an order up to 32, of the workgroup's 128 columns above (0: no order of these
// kernels, or no spare column).  A chunk whose width n + cols fits a 64-lane group runs on the register-resident
// kernels, a wider one on the workgroup-resident ones.
static int solve_chunk_cols(int n)
{
    return n < 1 || n >= kWorkgroupMaxOrder ? 0 : n <= 32 ? kResidentMaxOrder - n : kWorkgroupMaxOrder - n;
}

// One launch per chunk, full chunks first; every launch repeats the elimination of A, and the status words are zeroed
// once: a launch only ever raises a member's flag.  The caller holds h->mu and has set the device.
template <typename T>
static int one_launch_solve(mi32_context *h, const T *d_a, int n, int batch, const T *d_b, int nrhs, T *d_x, int *d_status)
{
    const int rc = status_buffer(h, d_status, batch, &d_status);
    if (rc != MI32_OK) return rc;
    hipError_t e = hipMemsetAsync(d_status, 0, sizeof(int) * (size_t)batch, h->stream);  // MI32_OK
    const int cap = solve_chunk_cols(n);
    for (int col0 = 0; e == hipSuccess && col0 < nrhs; col0 += cap) {
        const int cols = nrhs - col0 < cap ? nrhs - col0 : cap;
        const SolveArgs<T> s{d_a, d_b, d_x, d_status, n, batch, nrhs, col0, cols};
        e = n + cols <= kResidentMaxOrder ? resident_solve(s, h->stream, h->prof, h->pivoting)
                                          : workgroup_solve(s, h->stream, h->prof, h->pivoting);
    }
    if (e != hipSuccess) return fail(e, "kernel launch");
    return MI32_OK;
}

// the arguments are checked before the context is touched
template <typename T>
static int solve_device(mi32_context *h, const T *d_a, int n, int batch, const T *d_b, int nrhs, T *d_x, int *d_status)
{
    if (!h || !d_a || !d_b || !d_x || solve_chunk_cols(n) == 0 || batch <= 0 || nrhs <= 0 || d_x == d_a) return MI32_BAD_SHAPE;
    std::lock_guard<std::mutex> lk(h->mu);
    MI32_HIP(hipSetDevice(h->device));
    return one_launch_solve(h, d_a, n, batch, d_b, nrhs, d_x, d_status);
}

extern "C" {

int mi32_version(void) { return 142; }
const char *mi32_last_error(void) { return g_last_error.c_str(); }

int mi32_create(mi32_handle_t *out, int device)
{
    if (!out) return MI32_BAD_SHAPE;
    *out = nullptr;
    int count = 0;
    MI32_HIP(hipGetDeviceCount(&count));
    if (count <= 0) {
        g_last_error = "no HIP device visible";
        return MI32_RUNTIME_ERROR;
    }
    if (device < 0) MI32_HIP(hipGetDevice(&device));
    if (device >= count) {
        g_last_error = "device ordinal out of range";
        return MI32_RUNTIME_ERROR;
    }
    mi32_context *h = new (std::nothrow) mi32_context();
    if (!h) return MI32_RUNTIME_ERROR;
    h->device = device;
    MI32_HIP(hipSetDevice(device));
    MI32_HIP(hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
    h->stream = h->own_stream;
    if (env_int("MI32_LOOKAHEAD", 1)) {
        // Look-ahead (see blocked_invert): the half of each rank-bw update that is not on the critical
        // path runs on a second stream as a persistent kernel with one workgroup per CU on all but
        // the compute units lookahead_geometry reserves, which stay free for the panel / in-block kernels.
        // (Tried and rejected on MI355X: a plain second stream -- its workgroups fill every CU's register
        // file and the critical-path kernels queue behind them; hipExtStreamCreateWithCUMask -- it
        // serialises the two queues, 17 ms instead of 11.5.)
        hipDeviceProp_t prop;
        MI32_HIP(hipGetDeviceProperties(&prop, device));
        h->cu_count = prop.multiProcessorCount;
        int prio_low = 0, prio_high = 0;
        MI32_HIP(hipDeviceGetStreamPriorityRange(&prio_low, &prio_high));
        MI32_HIP(hipStreamCreateWithPriority(&h->aux_stream, hipStreamNonBlocking, prio_low));
        for (auto &ev : h->la_events) MI32_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        MI32_HIP(hipStreamCreateWithFlags(&h->split_stream, hipStreamNonBlocking));
    }
    *out = h;
    return MI32_OK;
}

int mi32_destroy(mi32_handle_t h)
{
    if (!h) return MI32_OK;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    if (h->ws) (void)hipFree(h->ws);
    if (h->d_in) (void)hipFree(h->d_in);
    if (h->d_out) (void)hipFree(h->d_out);
    if (h->d_status) (void)hipFree(h->d_status);
    if (h->d_istatus) (void)hipFree(h->d_istatus);
    h->copier.destroy();
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    if (h->switch_event) (void)hipEventDestroy(h->switch_event);
    if (h->aux_stream) {
        (void)hipStreamSynchronize(h->aux_stream);
        (void)hipStreamDestroy(h->aux_stream);
    }
    if (h->split_stream) {
        (void)hipStreamSynchronize(h->split_stream);
        (void)hipStreamDestroy(h->split_stream);
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
    if (!h || algo < MI32_ALGO_AUTO || algo > MI32_ALGO_WORKGROUP) return MI32_BAD_SHAPE;
    std::lock_guard<std::mutex> lk(h->mu);
    h->algo = algo;
    return MI32_OK;
}

int mi32_set_pivoting(mi32_handle_t h, int enable)
{
    if (!h) return MI32_BAD_SHAPE;
    std::lock_guard<std::mutex> lk(h->mu);
    h->pivoting = enable != 0;
    return MI32_OK;
}

int mi32_set_lookahead(mi32_handle_t h, int enable)
{
    if (!h) return MI32_BAD_SHAPE;
    std::lock_guard<std::mutex> lk(h->mu);
    h->lookahead = enable != 0;
    return MI32_OK;
}

int mi32_set_blocking(mi32_handle_t h, int panel_width, int block_width)
{
    if (!h || panel_width < 0 || block_width < 0) return MI32_BAD_SHAPE;
    std::lock_guard<std::mutex> lk(h->mu);
    h->panel_w = panel_width;
    h->block_w = block_width;
    return MI32_OK;
}

size_t mi32_workspace_bytes(int n, int batch, int algo)
{
    if (n <= 0 || batch <= 0) return 0;
    mi32_context tmp;
    tmp.algo = algo;
    return ws_bytes_for(&tmp, n, batch, resolve_algo(&tmp, n));
}

int mi32_resolve_algo(mi32_handle_t h, int n, int /*batch*/) { return resolve_algo(h, n); }

int mi32_resolve_blocking(mi32_handle_t h, int n, int batch, int *panel_width, int *block_width)
{
    if (n <= 0 || batch <= 0) return MI32_BAD_SHAPE;
    const BlockedPlan p = plan_blocked(h, n, batch);
    if (panel_width) *panel_width = p.w;
    if (block_width) *block_width = p.bw;
    return MI32_OK;
}

int mi32_resolve_panel_widths(mi32_handle_t h, int n, int batch, int *widths, int capacity, int *nblocks)
{
    if (n <= 0 || batch <= 0 || capacity < 0 || (capacity > 0 && !widths)) return MI32_BAD_SHAPE;
    const BlockedPlan p = plan_blocked(h, n, batch);
    if (nblocks) *nblocks = p.nblk;
    for (int b = 0; b < p.nblk && b < capacity; ++b) widths[b] = p.wblk[b];
    return MI32_OK;
}

int mi32_resolve_resident(mi32_handle_t /*h*/, int n, int elem_bytes, int *lanes_per_matrix, int *max_order)
{
    if (n <= 0 || (elem_bytes != 4 && elem_bytes != 8)) return MI32_BAD_SHAPE;
    if (lanes_per_matrix) *lanes_per_matrix = resident_lanes(n);
    if (max_order) *max_order = kResidentMaxOrder;
    return MI32_OK;
}

int mi32_resolve_workgroup(mi32_handle_t /*h*/, int n, int elem_bytes, int *threads_per_matrix, int *rows_per_thread,
                           int *max_order)
{
    if (n <= 0 || (elem_bytes != 4 && elem_bytes != 8)) return MI32_BAD_SHAPE;
    const int rpt = workgroup_rows_per_thread(n);
    if (threads_per_matrix) *threads_per_matrix = rpt ? 256 : 0;
    if (rows_per_thread) *rows_per_thread = rpt;
    if (max_order) *max_order = kWorkgroupMaxOrder;
    return MI32_OK;
}

int mi32_resolve_solve(mi32_handle_t /*h*/, int n, int nrhs, int elem_bytes, int *chunk_cols, int *launches, int *lanes,
                       int *rows_per_thread)
{
    const int cap = solve_chunk_cols(n);
    if (cap == 0 || nrhs <= 0 || (elem_bytes != 4 && elem_bytes != 8) || !chunk_cols || !launches || !lanes ||
        !rows_per_thread)
        return MI32_BAD_SHAPE;
    const int width = n + (nrhs < cap ? nrhs : cap);  // the first chunk's
    const bool resident = width <= kResidentMaxOrder;
    *chunk_cols = cap;
    *launches = (int)(((long long)nrhs + cap - 1) / cap);
    *lanes = resident ? resident_lanes(width) : 0;
    *rows_per_thread = resident ? 0 : workgroup_solve_rows_per_thread(n);
    return MI32_OK;
}

const char *mi32_dominant_kernel(int algo)
{
    return algo == MI32_ALGO_WORKGROUP ? "gj_workgroup_kernel"
           : algo == MI32_ALGO_RESIDENT ? "gj_resident_kernel"
           : algo == MI32_ALGO_SWEEP  ? "gj_sweep_step_kernel"
                                      : "gj_rank_bw2_kernel";
}

int mi32_reserve(mi32_handle_t h, int n, int batch)
{
    if (!h || n <= 0 || batch <= 0) return MI32_BAD_SHAPE;
    std::lock_guard<std::mutex> lk(h->mu);
    MI32_HIP(hipSetDevice(h->device));
    return ensure_ws(h, ws_bytes_for(h, n, batch, resolve_algo(h, n)));
}

// A GPU-filling batch of the blocked path is run as two halves on the context's two streams: the MFMA-bound
// rank-bw launches of one half overlap the latency / HBM-bound sub-panel launches of the other (64 x 2048^2:
// 18.5 -> 17.4 ms; three or four parts lose; round 3: 8 x 4096^2 23.6 -> 22.1 ms, 4 x 4096^2 15.7 -> 15.0: from four
// matrices on).  Both halves use the blocking of the whole batch, so a matrix's
// result does not depend on the split; mi32_set_lookahead(h, 0) turns the second stream off altogether.
static bool split_batch(const mi32_context *h, int algo, int n, int batch)
{
    return algo == MI32_ALGO_BLOCKED && h->lookahead && h->split_stream != nullptr && batch >= 4 &&
           (double)batch * n * n >= 64.0 * 1024.0 * 1024.0 && env_int("MI32_BATCH_SPLIT", 1) != 0;
}

int mi32_inv_device(mi32_handle_t h, const float *d_a, int n, int batch, float *d_inv, int *d_status)
{
    if (!h || !d_a || !d_inv || n <= 0 || batch <= 0 || d_a == d_inv) return MI32_BAD_SHAPE;
    std::lock_guard<std::mutex> lk(h->mu);
    MI32_HIP(hipSetDevice(h->device));
    const int algo = resolve_algo(h, n);
    int rc = ensure_ws(h, ws_bytes_for(h, n, batch, algo));
    if (rc != MI32_OK) return rc;
    if (algo == MI32_ALGO_RESIDENT || algo == MI32_ALGO_WORKGROUP)
        return one_launch_device(h, d_a, n, batch, d_inv, d_status, DetOut{nullptr, nullptr});
    rc = status_buffer(h, d_status, batch, &d_status);
    if (rc != MI32_OK) return rc;
    hipError_t e;
    if (algo == MI32_ALGO_SWEEP)
        e = sweep_invert(make_sweep_plan(n), d_a, d_inv, batch, d_status, h->ws, h->stream, h->prof, h->pivoting);
    else {
        BlockedExec ex;
        ex.stream = h->stream;
        ex.aux = h->lookahead ? h->aux_stream : nullptr;
        ex.events = h->la_events;
        ex.n_events = h->aux_stream ? 8 : 0;
        lookahead_geometry(h->cu_count, n, &ex.aux_workgroups, &ex.aux_exclusive);
        ex.prof = h->prof;
        ex.pivoting = h->pivoting;
        const BlockedPlan p = plan_blocked(h, n, batch);
        // (plans with panels shared by several workgroups are not split: those workgroups need whole CUs at the same
        // time, which the other half's rank-bw grid would keep from them for the length of its launch)
        if (!split_batch(h, algo, n, batch) || p.multi_panel) {
            e = blocked_invert(p, d_a, d_inv, batch, d_status, h->ws, ex);
        } else {
            const int b0 = (batch + 1) / 2, b1 = batch - b0;
            const size_t mat = (size_t)n * n;
            char *ws1 = (char *)h->ws + blocked_workspace_bytes(p, b0);  // ws_bytes_for reserved both parts
            // the second stream joins here and is joined again at the end (events 0 and 1 are free: the
            // look-ahead, their other user, only runs for single matrices)
            MI32_HIP(hipEventRecord(h->la_events[0], h->stream));
            MI32_HIP(hipStreamWaitEvent(h->split_stream, h->la_events[0], 0));
            BlockedExec ex0 = ex, ex1 = ex;
            ex0.aux = ex1.aux = nullptr;
            ex1.stream = h->split_stream;
            e = blocked_invert(p, d_a, d_inv, b0, d_status, h->ws, ex0);
            if (e == hipSuccess)
                e = blocked_invert(p, d_a + (size_t)b0 * mat, d_inv + (size_t)b0 * mat, b1,
                                   d_status + b0, ws1, ex1);
            MI32_HIP(hipEventRecord(h->la_events[1], h->split_stream));
            MI32_HIP(hipStreamWaitEvent(h->stream, h->la_events[1], 0));
        }
    }
    if (e != hipSuccess) return fail(e, "kernel launch");
    return MI32_OK;
}

// fp64: blocked (windowed steps + rank-bw updates on the fp64 matrix cores) from N = 256 on, measured cross-over;
// the no-pivot variant: its own blocked path (mi32_nopivot64.hip) from N = 512 on, the cross-over of the fp32
// no-pivot path; MI32_ALGO_SWEEP keeps the unblocked sweep
static int resolve_algo_f64(const mi32_context *h, int n)
{
    int algo = h ? h->algo : MI32_ALGO_AUTO;
    if (algo == MI32_ALGO_AUTO) algo = env_int("MI32_ALGO", MI32_ALGO_AUTO);
    if (algo == MI32_ALGO_RESIDENT && n <= kResidentMaxOrder) return algo;
    if (algo == MI32_ALGO_WORKGROUP && n <= kWorkgroupMaxOrder) return workgroup_or_resident(n);
    const int cross = (h && !h->pivoting) ? 512 : 256;
    if (algo != MI32_ALGO_SWEEP && algo != MI32_ALGO_BLOCKED) algo = (n >= cross) ? MI32_ALGO_BLOCKED : MI32_ALGO_SWEEP;
    return algo;
}
static int block_w64(const mi32_context *h) { return h && h->block_w ? h->block_w : env_int("MI32_BLOCK_W64", 0); }
static Blocked64Plan plan_blocked64(const mi32_context *h, int n) { return make_blocked64_plan(n, block_w64(h)); }
static NoPivot64Plan plan_nopivot64(const mi32_context *h, int n) { return make_nopivot64_plan(n, block_w64(h)); }

int mi32_resolve_blocking_f64(mi32_handle_t h, int n, int *block_width)
{
    if (n <= 0 || !block_width) return MI32_BAD_SHAPE;
    if (resolve_algo_f64(h, n) != MI32_ALGO_BLOCKED) *block_width = 0;
    else *block_width = (h && !h->pivoting) ? plan_nopivot64(h, n).bw : plan_blocked64(h, n).bw;
    return MI32_OK;
}

int mi32_inv_device_f64(mi32_handle_t h, const double *d_a, int n, int batch, double *d_inv, int *d_status)
{
    if (!h || !d_a || !d_inv || n <= 0 || batch <= 0 || d_a == d_inv) return MI32_BAD_SHAPE;
    std::lock_guard<std::mutex> lk(h->mu);
    MI32_HIP(hipSetDevice(h->device));
    const int algo = resolve_algo_f64(h, n);
    if (algo == MI32_ALGO_RESIDENT || algo == MI32_ALGO_WORKGROUP)
        return one_launch_device(h, d_a, n, batch, d_inv, d_status, DetOut{nullptr, nullptr});
    const bool blocked = algo == MI32_ALGO_BLOCKED;
    const bool nopivot = blocked && !h->pivoting;
    const Blocked64Plan bp = plan_blocked64(h, n);
    const NoPivot64Plan npp = plan_nopivot64(h, n);
    const SweepPlan sp = make_sweep_plan(n);
    int rc = ensure_ws(h, nopivot ? nopivot64_workspace_bytes(npp, batch)
                          : blocked ? blocked64_workspace_bytes(bp, batch)
                                    : sweep_workspace_bytes(sp, batch, sizeof(double)));
    if (rc != MI32_OK) return rc;
    rc = status_buffer(h, d_status, batch, &d_status);
    if (rc != MI32_OK) return rc;
    const hipError_t e = nopivot ? nopivot64_invert(npp, d_a, d_inv, batch, d_status, h->ws, h->stream, h->prof)
                         : blocked ? blocked64_invert(bp, d_a, d_inv, batch, d_status, h->ws, h->stream, h->prof)
                                   : sweep_invert(sp, d_a, d_inv, batch, d_status, h->ws, h->stream, h->prof, h->pivoting);
    if (e != hipSuccess) return fail(e, "kernel launch");
    return MI32_OK;
}

// ---- variable-size batches ---------------------------------------------------------------------------------------
// The kernel class of an order: 0 ... 3 the register-resident instances (8 / 16 / 32 / 64 lanes), 4 ... 7 the
// workgroup-resident ones (40 / 48 / 56 / 64 rows per thread); resident_lanes and workgroup_rows_per_thread stay the
// single source of the boundaries.  -1: no instance takes the order.
static int vbatch_class(int n)
{
    switch (resident_lanes(n)) {
        case 8: return 0;
        case 16: return 1;
        case 32: return 2;
        case 64: return 3;
        default: break;
    }
    switch (workgroup_rows_per_thread(n)) {
        case 40: return 4;
        case 48: return 5;
        case 56: return 6;
        case 64: return 7;
        default: return -1;
    }
}
static const int kVbatchLanes[4] = {8, 16, 32, 64};
static const int kVbatchRows[4] = {40, 48, 56, 64};

// The counting sort behind mi32_vbatch_bin, O(batch) and stable; order_begin (may be null; int[kWorkgroupMaxOrder + 2]):
// the members of order n are perm[order_begin[n] .. order_begin[n + 1]).  perm and class_begin may be null too.
static int vbatch_sort(const int *orders, int batch, int *perm, int *class_begin, int *order_begin)
{
    if (!orders || batch <= 0) return MI32_BAD_SHAPE;
    int start[kWorkgroupMaxOrder + 2] = {};
    for (int b = 0; b < batch; ++b) {
        const int n = orders[b];
        if (n < 1 || n > kWorkgroupMaxOrder) return MI32_BAD_SHAPE;
        ++start[n + 1];
    }
    int cls[kVbatchClasses + 1] = {};
    for (int n = 1; n <= kWorkgroupMaxOrder; ++n) {
        cls[vbatch_class(n) + 1] += start[n + 1];  // the members of order n (every order 1 ... 128 has a class)
        start[n + 1] += start[n];                  // start[n]: where the members of order n begin
    }
    for (int k = 0; k < kVbatchClasses; ++k) cls[k + 1] += cls[k];
    if (class_begin)
        for (int k = 0; k <= kVbatchClasses; ++k) class_begin[k] = cls[k];
    if (order_begin)
        for (int n = 0; n <= kWorkgroupMaxOrder + 1; ++n) order_begin[n] = start[n];
    if (perm)
        for (int b = 0; b < batch; ++b) perm[start[orders[b]]++] = b;
    return MI32_OK;
}

int mi32_vbatch_bin(const int *orders, int batch, int *perm, int *class_begin)
{
    if (!perm || !class_begin) return MI32_BAD_SHAPE;
    return vbatch_sort(orders, batch, perm, class_begin, nullptr);
}

int mi32_vbatch_create(mi32_handle_t h, const int *orders, int batch, mi32_vbatch_t *out)
{
    if (!out) return MI32_BAD_SHAPE;
    *out = nullptr;
    if (!h || !orders || batch <= 0) return MI32_BAD_SHAPE;
    std::vector<int> perm((size_t)batch);
    mi32_vbatch *p = new (std::nothrow) mi32_vbatch();
    if (!p) return MI32_RUNTIME_ERROR;
    const int rc = vbatch_sort(orders, batch, perm.data(), p->class_begin, p->order_begin);
    if (rc != MI32_OK) {
        delete p;
        return rc;
    }
    p->device = h->device;
    p->batch = batch;
    const size_t bytes = (size_t)batch * sizeof(int);
    hipError_t e = hipSetDevice(h->device);
    if (e == hipSuccess) e = hipMalloc((void **)&p->d_orders, bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&p->d_members, bytes);
    // synchronous copies from pageable memory: the host arrays may go away when this returns
    if (e == hipSuccess) e = hipMemcpy(p->d_orders, orders, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p->d_members, perm.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)mi32_vbatch_destroy(p);
        return fail(e, "mi32_vbatch_create");
    }
    *out = p;
    return MI32_OK;
}

int mi32_vbatch_destroy(mi32_vbatch_t p)
{
    if (!p) return MI32_OK;
    (void)hipSetDevice(p->device);
    // hipFree synchronises with the device: calls that still read the plan finish first
    if (p->d_orders) (void)hipFree(p->d_orders);
    if (p->d_members) (void)hipFree(p->d_members);
    delete p;
    return MI32_OK;
}

int mi32_vbatch_info(mi32_vbatch_t p, int *batch, int *class_begin)
{
    if (!p) return MI32_BAD_SHAPE;
    if (batch) *batch = p->batch;
    if (class_begin)
        for (int k = 0; k <= kVbatchClasses; ++k) class_begin[k] = p->class_begin[k];
    return MI32_OK;
}

}  // extern "C"

// the inverse with the determinant on the one-launch paths, whatever the context's algorithm (see the header); the
// arguments are checked before the context is touched
template <typename T>
static int inv_det_device(mi32_context *h, const T *d_a, int n, int batch, T *d_inv, int *d_status, double *d_det_mant,
                          int *d_det_exp)
{
    if (!h || !d_a || n <= 0 || n > kWorkgroupMaxOrder || batch <= 0 || d_a == d_inv || !d_det_mant || !d_det_exp)
        return MI32_BAD_SHAPE;
    std::lock_guard<std::mutex> lk(h->mu);
    MI32_HIP(hipSetDevice(h->device));
    return one_launch_device(h, d_a, n, batch, d_inv, d_status, DetOut{d_det_mant, d_det_exp});
}

// DET: the det kernels, d_inv may be null
template <typename T, bool DET>
static int inv_device_vbatched(mi32_context *h, const mi32_vbatch *p, const T *const *d_a, const int *d_lda,
                               T *const *d_inv, const int *d_ldinv, int *d_status, double *d_det_mant = nullptr,
                               int *d_det_exp = nullptr)
{
    if (!h || !p || !d_a || (!DET && !d_inv) || (DET && (!d_det_mant || !d_det_exp))) return MI32_BAD_SHAPE;
    if (p->device != h->device) return MI32_BAD_SHAPE;
    std::lock_guard<std::mutex> lk(h->mu);
    MI32_HIP(hipSetDevice(h->device));
    const int rc = status_buffer(h, d_status, p->batch, &d_status);
    if (rc != MI32_OK) return rc;
    MI32_HIP(hipMemsetAsync(d_status, 0, sizeof(int) * (size_t)p->batch, h->stream));  // MI32_OK
    const VbatchArgs<T> v{p->d_orders, p->d_members, d_a, d_inv, d_lda, d_ldinv, d_status};
    const DetOut det = DET ? DetOut{d_det_mant, d_det_exp} : DetOut{nullptr, nullptr};
    for (int k = 0; k < kVbatchClasses; ++k) {
        const int first = p->class_begin[k], count = p->class_begin[k + 1] - first;
        if (count == 0) continue;  // a class without members is not launched
        const hipError_t e =
            k < 4 ? resident_vinvert(kVbatchLanes[k], v, det, first, count, h->stream, h->prof, h->pivoting)
                  : workgroup_vinvert(kVbatchRows[k - 4], v, det, first, count, h->stream, h->prof, h->pivoting);
        if (e != hipSuccess) return fail(e, "kernel launch");
    }
    return MI32_OK;
}

// ---- A X = B for a variable-size batch ------------------------------------------------------------------------------
// Every member is treated as one_launch_solve treats a uniform batch of its order: the nrhs columns in chunks of
// solve_chunk_cols(n), full ones first, a chunk of width n + cols <= kResidentMaxOrder on the register-resident kernel
// (resident_lanes of the width), a wider one on the workgroup-resident kernel.  How an order's chunks run:
struct VsolveChunks {
    int cols;            // columns of a full chunk (of the only chunk, when nrhs fits one)
    long long chunks;    // ceil(nrhs / cap)
    int first_instance;  // the kernel of the full chunks, last_instance: of the remainder (the same when there is none)
    int last_instance;   // an instance: lanes per member (8 ... 64), or -(rows per thread) for the workgroup kernel
    bool operator==(const VsolveChunks &o) const
    {
        return cols == o.cols && chunks == o.chunks && first_instance == o.first_instance && last_instance == o.last_instance;
    }
};
static int vsolve_instance(int n, int cols)
{
    return n + cols <= kResidentMaxOrder ? resident_lanes(n + cols) : -workgroup_solve_rows_per_thread(n);
}
static VsolveChunks vsolve_chunks(int n, int nrhs)
{
    const int cap = solve_chunk_cols(n);
    VsolveChunks c;
    c.cols = nrhs < cap ? nrhs : cap;
    c.chunks = ((long long)nrhs + cap - 1) / cap;
    c.first_instance = vsolve_instance(n, c.cols);
    c.last_instance = vsolve_instance(n, (int)(nrhs - (c.chunks - 1) * cap));
    return c;
}
// The launches of a call, in the order they are enqueued: f(first, count, col0, cols, lanes, rows_per_thread) -> bool
// (false ends the walk) for every chunk of every maximal run of consecutive sorted members whose chunk sequences agree
// -- two orders' sequences agree when c.cols, the number of chunks and the two instances do: col0 and cols of every
// chunk follow from these.  order_begin as in mi32_vbatch (no member of order 128: the caller's business).  The one
// place the rule lives: mi32_vbatch_solve_launches reports this list and mi32_solve_device_vbatched* walks it.
template <typename F>
static void vsolve_walk(const int *order_begin, int nrhs, F f)
{
    int n = 1;
    while (n < kWorkgroupMaxOrder) {
        if (order_begin[n + 1] == order_begin[n]) {  // no member of this order
            ++n;
            continue;
        }
        const VsolveChunks c = vsolve_chunks(n, nrhs);
        int end = n + 1;  // the run takes the orders n ... end - 1
        while (end < kWorkgroupMaxOrder && (order_begin[end + 1] == order_begin[end] || vsolve_chunks(end, nrhs) == c)) ++end;
        // (orders without members at the run's end belong to no launch: the range below does not see them)
        const int first = order_begin[n], count = order_begin[end] - first;
        for (long long k = 0; k < c.chunks; ++k) {
            const long long col0 = k * c.cols;
            const int cols = (int)(nrhs - col0 < c.cols ? nrhs - col0 : c.cols);
            const int inst = k + 1 < c.chunks ? c.first_instance : c.last_instance;
            if (!f(first, count, (int)col0, cols, inst > 0 ? inst : 0, inst > 0 ? 0 : -inst)) return;
        }
        n = end;
    }
}

// the arguments are checked before the context is touched
template <typename T>
static int solve_device_vbatched(mi32_context *h, const mi32_vbatch *p, const T *const *d_a, const int *d_lda,
                                 const T *const *d_b, const int *d_ldb, int nrhs, T *const *d_x, const int *d_ldx,
                                 int *d_status)
{
    if (!h || !p || !d_a || !d_b || !d_x || nrhs <= 0) return MI32_BAD_SHAPE;
    if (p->device != h->device) return MI32_BAD_SHAPE;
    // order 128 has no spare column
    if (p->order_begin[kWorkgroupMaxOrder + 1] != p->order_begin[kWorkgroupMaxOrder]) return MI32_BAD_SHAPE;
    std::lock_guard<std::mutex> lk(h->mu);
    MI32_HIP(hipSetDevice(h->device));
    const int rc = status_buffer(h, d_status, p->batch, &d_status);
    if (rc != MI32_OK) return rc;
    // zeroed once: a launch only ever raises a member's flag
    hipError_t e = hipMemsetAsync(d_status, 0, sizeof(int) * (size_t)p->batch, h->stream);  // MI32_OK
    if (e == hipSuccess)
        vsolve_walk(p->order_begin, nrhs, [&](int first, int count, int col0, int cols, int lanes, int rows) {
            const VsolveArgs<T> v{p->d_orders, p->d_members, d_a, d_b, d_x, d_lda, d_ldb, d_ldx, d_status, nrhs, col0, cols};
            e = lanes ? resident_vsolve(lanes, v, first, count, h->stream, h->prof, h->pivoting)
                      : workgroup_vsolve(rows, v, first, count, h->stream, h->prof, h->pivoting);
            return e == hipSuccess;
        });
    if (e != hipSuccess) return fail(e, "kernel launch");
    return MI32_OK;
}

extern "C" {

int mi32_vbatch_solve_launches(const int *orders, int batch, int nrhs, int *launches, int capacity, int *count)
{
    if (!orders || !count || batch <= 0 || nrhs <= 0 || capacity < 0 || (capacity > 0 && !launches)) return MI32_BAD_SHAPE;
    int order_begin[kWorkgroupMaxOrder + 2];
    if (vbatch_sort(orders, batch, nullptr, nullptr, order_begin) != MI32_OK) return MI32_BAD_SHAPE;
    if (order_begin[kWorkgroupMaxOrder + 1] != order_begin[kWorkgroupMaxOrder]) return MI32_BAD_SHAPE;  // an order 128
    long long total = 0;
    vsolve_walk(order_begin, nrhs, [&](int first, int cnt, int col0, int cols, int lanes, int rows) {
        if (total < capacity) {
            int *l = launches + 6 * total;
            l[0] = first, l[1] = cnt, l[2] = col0, l[3] = cols, l[4] = lanes, l[5] = rows;
        }
        ++total;
        return true;
    });
    if (total > 0x7fffffffLL) return MI32_BAD_SHAPE;
    *count = (int)total;
    return MI32_OK;
}

int mi32_solve_device_vbatched(mi32_handle_t h, mi32_vbatch_t p, const float *const *d_a, const int *d_lda,
                               const float *const *d_b, const int *d_ldb, int nrhs, float *const *d_x, const int *d_ldx,
                               int *d_status)
{
    return solve_device_vbatched(h, p, d_a, d_lda, d_b, d_ldb, nrhs, d_x, d_ldx, d_status);
}

int mi32_solve_device_vbatched_f64(mi32_handle_t h, mi32_vbatch_t p, const double *const *d_a, const int *d_lda,
                                   const double *const *d_b, const int *d_ldb, int nrhs, double *const *d_x,
                                   const int *d_ldx, int *d_status)
{
    return solve_device_vbatched(h, p, d_a, d_lda, d_b, d_ldb, nrhs, d_x, d_ldx, d_status);
}

int mi32_inv_device_vbatched(mi32_handle_t h, mi32_vbatch_t p, const float *const *d_a, const int *d_lda,
                             float *const *d_inv, const int *d_ldinv, int *d_status)
{
    return inv_device_vbatched<float, false>(h, p, d_a, d_lda, d_inv, d_ldinv, d_status);
}

int mi32_inv_device_vbatched_f64(mi32_handle_t h, mi32_vbatch_t p, const double *const *d_a, const int *d_lda,
                                 double *const *d_inv, const int *d_ldinv, int *d_status)
{
    return inv_device_vbatched<double, false>(h, p, d_a, d_lda, d_inv, d_ldinv, d_status);
}

int mi32_inv_det_device(mi32_handle_t h, const float *d_a, int n, int batch, float *d_inv, int *d_status,
                        double *d_det_mant, int *d_det_exp)
{
    return inv_det_device(h, d_a, n, batch, d_inv, d_status, d_det_mant, d_det_exp);
}

int mi32_inv_det_device_f64(mi32_handle_t h, const double *d_a, int n, int batch, double *d_inv, int *d_status,
                            double *d_det_mant, int *d_det_exp)
{
    return inv_det_device(h, d_a, n, batch, d_inv, d_status, d_det_mant, d_det_exp);
}

int mi32_solve_device(mi32_handle_t h, const float *d_a, int n, int batch, const float *d_b, int nrhs, float *d_x,
                      int *d_status)
{
    return solve_device(h, d_a, n, batch, d_b, nrhs, d_x, d_status);
}

int mi32_solve_device_f64(mi32_handle_t h, const double *d_a, int n, int batch, const double *d_b, int nrhs, double *d_x,
                          int *d_status)
{
    return solve_device(h, d_a, n, batch, d_b, nrhs, d_x, d_status);
}

int mi32_inv_det_device_vbatched(mi32_handle_t h, mi32_vbatch_t p, const float *const *d_a, const int *d_lda,
                                 float *const *d_inv, const int *d_ldinv, int *d_status, double *d_det_mant,
                                 int *d_det_exp)
{
    return inv_device_vbatched<float, true>(h, p, d_a, d_lda, d_inv, d_ldinv, d_status, d_det_mant, d_det_exp);
}

int mi32_inv_det_device_vbatched_f64(mi32_handle_t h, mi32_vbatch_t p, const double *const *d_a, const int *d_lda,
                                     double *const *d_inv, const int *d_ldinv, int *d_status, double *d_det_mant,
                                     int *d_det_exp)
{
    return inv_device_vbatched<double, true>(h, p, d_a, d_lda, d_inv, d_ldinv, d_status, d_det_mant, d_det_exp);
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
    h->prof->collect(ms_per_class, launches_per_class);
    return MI32_OK;
}

int mi32_residual_device(mi32_handle_t h, const float *d_a, const float *d_x, int n, int batch, double *d_out)
{
    if (!h || !d_a || !d_x || !d_out || n <= 0 || batch <= 0) return MI32_BAD_SHAPE;
    std::lock_guard<std::mutex> lk(h->mu);
    MI32_HIP(hipSetDevice(h->device));
    int rc = ensure_ws(h, ws_bytes_for(h, n, batch, resolve_algo(h, n)));
    if (rc != MI32_OK) return rc;
    hipError_t e = residual_launch(d_a, d_x, n, batch, d_out, h->ws, h->stream);
    if (e != hipSuccess) return fail(e, "residual launch");
    return MI32_OK;
}

}  // extern "C"

// ---- host-pointer entry points on the default context ---------------------------
static mi32_context *g_default = nullptr;
static std::mutex g_default_mu;

static int default_context(mi32_context **out)
{
    std::lock_guard<std::mutex> lk(g_default_mu);
    if (!g_default) {
        mi32_handle_t h = nullptr;
        int rc = mi32_create(&h, env_int("MI32_DEVICE", 0));
        if (rc != MI32_OK) return rc;
        g_default = h;
    }
    *out = g_default;
    return MI32_OK;
}

static int ensure_io(mi32_context *h, size_t floats, size_t ints)
{
    if (floats > h->io_floats) {
        if (h->d_in) MI32_HIP(hipFree(h->d_in));
        if (h->d_out) MI32_HIP(hipFree(h->d_out));
        h->d_in = h->d_out = nullptr;
        h->io_floats = 0;
        MI32_HIP(hipMalloc((void **)&h->d_in, floats * sizeof(float)));
        MI32_HIP(hipMalloc((void **)&h->d_out, floats * sizeof(float)));
        h->io_floats = floats;
    }
    if (ints > h->status_ints) {
        if (h->d_status) MI32_HIP(hipFree(h->d_status));
        h->d_status = nullptr;
        h->status_ints = 0;
        MI32_HIP(hipMalloc((void **)&h->d_status, ints * sizeof(int)));
        h->status_ints = ints;
    }
    return MI32_OK;
}

// dev <- host (to_device) or host <- dev; synchronous.  Large transfers go through the pinned ring of HostCopier
// (MI32_HOST_COPY=0 keeps the runtime's pageable path), small ones through one hipMemcpyAsync.
static int host_copy(mi32_context *h, void *dev, void *host, size_t bytes, bool to_device)
{
    if (bytes >= HostCopier::kMinBytes && env_int("MI32_HOST_COPY", 1) != 0) {
        MI32_HIP(h->copier.init(h->device));
        MI32_HIP(hipStreamSynchronize(h->stream));  // the lanes' streams are not ordered with the context's stream
        MI32_HIP(h->copier.run(dev, host, bytes, to_device));
        return MI32_OK;
    }
    if (to_device) MI32_HIP(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, h->stream));
    else MI32_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, h->stream));
    MI32_HIP(hipStreamSynchronize(h->stream));
    return MI32_OK;
}

// The reference's ten timing slots (FP32_bench.cpp:256-443) from the profiler's per-class milliseconds and the host
// clock stamps of a host-pointer call (tq0: before the context, t0: after it, t1: H2D done, t2: compute done, t3: D2H done).
static void fill_times10(double *times10, const double *ms, std::chrono::steady_clock::time_point tq0,
                         std::chrono::steady_clock::time_point t0, std::chrono::steady_clock::time_point t1,
                         std::chrono::steady_clock::time_point t2, std::chrono::steady_clock::time_point t3)
{
    auto sec = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
        return std::chrono::duration<double>(b - a).count();
    };
    times10[0] = sec(tq0, t0);
    times10[1] = sec(t0, t1);
    times10[2] = 0.0;  // one ahead-of-time compiled code object: nothing is built at run time
    times10[3] = ms[KC_INIT] * 1e-3;
    // the panel kernel IS maxPivot + finalMaxPivot + pivotElements + fixRow (+ fixColumn on the panel's own columns); the
    // fused step launches of the sweep path are accounted to the column slot, where the reference spends its time
    times10[4] = ms[KC_PANEL] * 1e-3;
    times10[5] = 0.0;  // fixRow has no launch of its own
    times10[6] = (ms[KC_SWEEP_STEP] + ms[KC_UPDATE_IN] + ms[KC_UPDATE_OUT] + ms[KC_TRANSPOSE]) * 1e-3;
    times10[7] = sec(t1, t2);
    times10[8] = ms[KC_FINISH] * 1e-3 + sec(t2, t3);
    times10[9] = sec(tq0, t3);
}

// The host-pointer path.  times10 (may be NULL): the reference's timing vector, FP32_bench.cpp:256-443 /
// res_struct.h:4-6 -- [0] queue/context, [1] buffers (+ the H2D copy the reference's CL_MEM_COPY_HOST_PTR does),
// [2] program build, [3] makeAugmented, [4] pivot, [5] row, [6] column, [7] compute, [8] getInverted (+ D2H),
// [9] total; seconds.  The per-phase slots come from HIP events on the launch stream (mi32_set_profiling).
// Pre-faulting of a large host buffer on several threads, WITHOUT writing to it: madvise(MADV_POPULATE_WRITE) makes
// the kernel install writable pages (zero pages for fresh memory, the present contents otherwise) -- the buffer's
// bytes, and any C++ object that lives or will live there, are never touched by us.  The kernel hands out pages one
// fault at a time: 64 MiB cost ~12 ms on one thread of the MI355X host, ~2 ms on eight.  Used (a) on the result
// vector's reserved storage before it is value-initialised and (b) on the caller's output buffer while the device
// works -- which therefore keeps its contents until the copy back (mat_inv_32_c.h: "written only on MI32_OK /
// MI32_SINGULAR").  Where the kernel does not know the advice the pages are faulted by the copy itself, as before.
static void parallel_populate(void *p, size_t bytes, bool may_rewrite = false)
{
    const size_t kPage = 4096, kMin = (size_t)8 << 20;
    if (bytes < kMin) return;
    const uintptr_t lo = ((uintptr_t)p + kPage - 1) & ~(uintptr_t)(kPage - 1);
    const uintptr_t hi = ((uintptr_t)p + bytes) & ~(uintptr_t)(kPage - 1);
    if (hi <= lo) return;
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt > 8 ? 8 : (nt < 1 ? 1 : nt);
    const size_t span = hi - lo;
    const size_t chunk = ((span / nt) + kPage - 1) & ~(kPage - 1);
    // may_rewrite (the caller's output buffer, ours to write for the duration of the call): where the kernel does not
    // know the advice (Linux < 5.14) every page's first byte is read and written back unchanged instead
    auto populate = [may_rewrite](uintptr_t a, size_t len) {
        int rc = -1;
#ifdef MADV_POPULATE_WRITE
        rc = madvise(reinterpret_cast<void *>(a), len, MADV_POPULATE_WRITE);
#endif
        if (rc != 0 && may_rewrite) {
            for (size_t off = 0; off < len; off += 4096) {
                volatile char *q = reinterpret_cast<volatile char *>(a + off);
                const char v = *q;
                *q = v;
            }
        }
    };
    std::vector<std::thread> th;
    for (unsigned i = 1; i < nt; ++i) {
        const size_t off = (size_t)i * chunk;
        if (off >= span) break;
        const size_t len = (off + chunk <= span) ? chunk : span - off;
        try { th.emplace_back(populate, lo + off, len); } catch (...) { populate(lo + off, len); }
    }
    populate(lo, chunk < span ? chunk : span);
    for (auto &t : th) t.join();
}

// Error returns of the host-pointer paths leave the context as they found it.
struct ProfilingGuard {
    mi32_context *h = nullptr;
    ~ProfilingGuard() { if (h) (void)mi32_set_profiling(h, 0); }
};

// the device entry point per element type
static int inv_device(mi32_context *h, const float *d_a, int n, int batch, float *d_inv, int *d_status)
{
    return mi32_inv_device(h, d_a, n, batch, d_inv, d_status);
}
static int inv_device(mi32_context *h, const double *d_a, int n, int batch, double *d_inv, int *d_status)
{
    return mi32_inv_device_f64(h, d_a, n, batch, d_inv, d_status);
}

// `late_out`: where the result goes is only asked for once the kernels are queued -- the std::vector entry points
// allocate and first-touch their 4 N^2 result bytes (64 MiB of page faults at N = 4096, ~8 ms) while the device works
typedef void *(*LateOut)(void *ctx);
// One host-pointer inversion on context h; the caller holds the lock that guards h's staging buffers.
// pivoting: the variant of this one call (the context's own setting is restored afterwards).
// total_s / compute_s: the reference's two numbers ("Tempo Totale Impiegato" / "Tempo Computazione", mat_inv_32.cpp:385-386).
template <typename T>
static int host_invert_on(mi32_context *h, std::chrono::steady_clock::time_point tq0, const T *a, int n, int batch,
                          T *inv, int *status, double *times10, bool pivoting, LateOut late_out, void *late_ctx,
                          double *total_s, double *compute_s)
{
    const auto t0 = std::chrono::steady_clock::now();
    MI32_HIP(hipSetDevice(h->device));
    const size_t elems = (size_t)batch * n * n;
    int rc = ensure_io(h, elems * (sizeof(T) / sizeof(float)), (size_t)batch);  // staging capacity in 4-byte units
    if (rc != MI32_OK) return rc;
    ProfilingGuard prof_guard;  // profiling is switched off again on every way out
    if (times10) {
        if (std::is_same<T, float>::value) {
            rc = mi32_reserve(h, n, batch);  // fp32: workspace allocation belongs to the "buffers" slot
            if (rc != MI32_OK) return rc;
        }
        rc = mi32_set_profiling(h, 1);
        if (rc != MI32_OK) return rc;
        prof_guard.h = h;
        double ms[KC_COUNT]; long long cnt[KC_COUNT];
        (void)mi32_get_profile(h, ms, cnt, KC_COUNT);  // drop what an earlier call left
    }
    T *d_in = reinterpret_cast<T *>(h->d_in), *d_out = reinterpret_cast<T *>(h->d_out);
    rc = host_copy(h, d_in, const_cast<T *>(a), elems * sizeof(T), true);
    if (rc != MI32_OK) return rc;
    const auto t1 = std::chrono::steady_clock::now();
    {
        const bool saved = h->pivoting;  // host-pointer contexts are only used under their caller's lock
        h->pivoting = pivoting;
        rc = inv_device(h, d_in, n, batch, d_out, h->d_status);
        h->pivoting = saved;
    }
    if (rc != MI32_OK) return rc;
    if (late_out) {
        inv = static_cast<T *>(late_out(late_ctx));
        if (!inv) { (void)hipStreamSynchronize(h->stream); return MI32_RUNTIME_ERROR; }
    } else {
        parallel_populate(inv, elems * sizeof(T), true);  // the device is busy for the next milliseconds
    }
    MI32_HIP(hipStreamSynchronize(h->stream));
    const auto t2 = std::chrono::steady_clock::now();
    std::vector<int> st((size_t)batch);
    MI32_HIP(hipMemcpyAsync(st.data(), h->d_status, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    rc = host_copy(h, d_out, inv, elems * sizeof(T), false);
    if (rc != MI32_OK) return rc;
    MI32_HIP(hipStreamSynchronize(h->stream));
    const auto t3 = std::chrono::steady_clock::now();
    if (total_s) *total_s = std::chrono::duration<double>(t3 - t0).count();
    if (compute_s) *compute_s = std::chrono::duration<double>(t2 - t1).count();
    if (times10) {
        double ms[KC_COUNT]; long long cnt[KC_COUNT];
        rc = mi32_get_profile(h, ms, cnt, KC_COUNT);
        if (rc != MI32_OK) return rc;
        fill_times10(times10, ms, tq0, t0, t1, t2, t3);
    }
    int worst = MI32_OK;
    for (int b = 0; b < batch; ++b) {
        if (status) status[b] = st[(size_t)b];
        if (st[(size_t)b] > worst) worst = st[(size_t)b];
    }
    if (worst == MI32_RUNTIME_ERROR)  // the only status-borne runtime error (mi32_blocked.hip, fp32 shared panels)
        g_last_error = "a workgroup of a shared panel timed out waiting for its partners (the device was not ours "
                       "alone); the affected inverse is NaN-filled -- retry, or set MI32_MULTI_PANEL=0";
    return worst;
}

static void print_reference_timing_lines()
{
    if (env_int("MI32_VERBOSE", 0)) {
        // the reference's two stdout lines (mat_inv_32.cpp:385-386)
        std::printf("Tempo Totale Impiegato: %g seconds\nTempo Computazione: %g seconds\n", g_last_total,
                    g_last_compute);
        std::fflush(stdout);
    }
}

// One host-pointer inversion on the default context.  The fp32 calls print the reference's timing lines.
template <typename T>
static int host_invert(const T *a, int n, int batch, T *inv, int *status, double *times10, bool pivoting = true,
                       LateOut late_out = nullptr, void *late_ctx = nullptr)
{
    if (!a || (!inv && !late_out) || n <= 0 || batch <= 0) return MI32_BAD_SHAPE;
    const auto tq0 = std::chrono::steady_clock::now();
    mi32_context *h = nullptr;
    int rc = default_context(&h);  // the reference's platform / device / context / queue bring-up (cached here)
    if (rc != MI32_OK) return rc;
    std::lock_guard<std::mutex> lk(g_host_call_mu);  // one host-pointer call at a time: the staging buffers are shared
    rc = host_invert_on(h, tq0, a, n, batch, inv, status, times10, pivoting, late_out, late_ctx, &g_last_total,
                        &g_last_compute);
    if (std::is_same<T, float>::value && (rc == MI32_OK || rc == MI32_SINGULAR || rc == MI32_RUNTIME_ERROR))
        print_reference_timing_lines();
    return rc;
}

// the reference's shape guards, mat_inv_32.cpp:206-215 (integer division included); matrix_inversion_FP64.cpp
// has the same two
static bool bad_order(size_t a_len, int n) { return n <= 0 || (int)(a_len / (size_t)n) != n; }

extern "C" {

// ---- the batch over several GPUs (what replaces the reference's platforms[0] / devices[0],
//      mat_inv_32.cpp:239-244) -------------------------------------------------------------------------
// One context and one host thread per GPU; GPU g owns the matrices [g * ceil(B / G), min(B, (g + 1) * ceil(B / G)))
// and copies ITS OWN shard host -> device, inverts it and copies it back: no data-path exchange between the GPUs,
// the worst status word is the return value.  The contexts are created on first use and kept.
// MI32_MULTI_OVERSUBSCRIBE=1 (tests, single-GPU hosts): logical GPU g runs on device g % (visible devices), each with
// a context of its own -- the threading, the ragged shards and the status reduction run exactly as on a real node.
namespace {
struct MultiSlot {
    mi32_context *h = nullptr;
    std::mutex mu;  // guards h's staging buffers, like g_host_call_mu guards the default context's
};
std::mutex g_multi_mu;                 // guards the table
std::vector<MultiSlot *> g_multi;      // logical GPU -> slot (never shrinks; slots are never freed)
}  // namespace

// GPU g of G owns the matrices [g * ceil(B / G), min(B, (g + 1) * ceil(B / G))) (possibly none)
extern "C" int mi32_shard_range(int batch, int ngpus, int g, int *lo, int *hi)
{
    if (batch < 0 || ngpus <= 0 || g < 0 || g >= ngpus || !lo || !hi) return MI32_BAD_SHAPE;
    const int per = (batch + ngpus - 1) / ngpus;
    const long long l = (long long)g * per;
    *lo = l < batch ? (int)l : batch;
    *hi = (l + per < batch) ? (int)(l + per) : batch;
    return MI32_OK;
}

extern "C" int mi32_matrix_inv_32_batched_multi(const float *a, int n, int batch, float *inv, int *status, int ngpus)
{
    if (!a || !inv || n <= 0 || batch <= 0) return MI32_BAD_SHAPE;
    const auto tq0 = std::chrono::steady_clock::now();
    int visible = 0;
    MI32_HIP(hipGetDeviceCount(&visible));
    if (visible <= 0) {
        g_last_error = "no HIP device visible";
        return MI32_RUNTIME_ERROR;
    }
    const bool oversub = env_int("MI32_MULTI_OVERSUBSCRIBE", 0) != 0;
    if (ngpus <= 0) ngpus = visible;
    if (ngpus > visible && !oversub) {
        g_last_error = "mi32_matrix_inv_32_batched_multi: more GPUs asked for than are visible";
        return MI32_BAD_SHAPE;
    }
    if (ngpus > batch) ngpus = batch;  // at least one matrix per GPU
    std::vector<MultiSlot *> slots((size_t)ngpus, nullptr);
    {
        std::lock_guard<std::mutex> lk(g_multi_mu);
        while ((int)g_multi.size() < ngpus) g_multi.push_back(new (std::nothrow) MultiSlot());
        for (int g = 0; g < ngpus; ++g) {
            if (!g_multi[(size_t)g]) return MI32_RUNTIME_ERROR;
            slots[(size_t)g] = g_multi[(size_t)g];
        }
    }
    std::vector<int> rcs((size_t)ngpus, MI32_OK);
    std::vector<std::string> errs((size_t)ngpus);
    std::vector<double> tot((size_t)ngpus, 0.0), cmp((size_t)ngpus, 0.0);
    const size_t mat = (size_t)n * n;
    auto work = [&](int g) {
        int lo = 0, hi = 0;
        (void)mi32_shard_range(batch, ngpus, g, &lo, &hi);
        if (lo >= hi) return;  // ragged tail: this GPU has nothing
        MultiSlot *sl = slots[(size_t)g];
        std::lock_guard<std::mutex> lk(sl->mu);
        int rc = MI32_OK;
        if (!sl->h) {
            mi32_handle_t nh = nullptr;
            rc = mi32_create(&nh, g % visible);
            if (rc == MI32_OK) sl->h = nh;
        }
        if (rc == MI32_OK)
            rc = host_invert_on(sl->h, tq0, a + (size_t)lo * mat, n, hi - lo, inv + (size_t)lo * mat,
                                status ? status + lo : nullptr, nullptr, true, nullptr, nullptr, &tot[(size_t)g],
                                &cmp[(size_t)g]);
        rcs[(size_t)g] = rc;
        if (rc != MI32_OK) errs[(size_t)g] = g_last_error;  // thread-local: carried to the caller's thread below
    };
    std::vector<std::thread> th;
    for (int g = 1; g < ngpus; ++g) {
        try { th.emplace_back(work, g); } catch (...) { work(g); }
    }
    work(0);
    for (auto &t : th) t.join();
    int worst = MI32_OK;
    double t_tot = 0.0, t_cmp = 0.0;
    for (int g = 0; g < ngpus; ++g) {
        const int rc = rcs[(size_t)g];
        if (rc == MI32_BAD_SHAPE) return MI32_BAD_SHAPE;
        if (rc > worst) { worst = rc; if (!errs[(size_t)g].empty()) g_last_error = errs[(size_t)g]; }
        if (tot[(size_t)g] > t_tot) t_tot = tot[(size_t)g];
        if (cmp[(size_t)g] > t_cmp) t_cmp = cmp[(size_t)g];
    }
    {
        std::lock_guard<std::mutex> lk(g_host_call_mu);
        g_last_total = t_tot;
        g_last_compute = t_cmp;
        print_reference_timing_lines();
    }
    return worst;
}

int mi32_matrix_inv_32_batched(const float *a, int n, int batch, float *inv, int *status)
{
    return host_invert(a, n, batch, inv, status, nullptr);
}

int mi32_bench_32(const float *a_rowmajor, size_t a_len, int n, float *inv_rowmajor, double *times10)
{
    if (!times10 || bad_order(a_len, n)) return MI32_BAD_SHAPE;
    return host_invert(a_rowmajor, n, 1, inv_rowmajor, nullptr, times10);
}

int mi32_matrix_inv_32(const float *a_rowmajor, size_t a_len, int n, float *inv_rowmajor)
{
    if (bad_order(a_len, n)) return MI32_BAD_SHAPE;
    return host_invert(a_rowmajor, n, 1, inv_rowmajor, nullptr, nullptr);
}

int mi32_matrix_inv_64(const double *a_rowmajor, size_t a_len, int n, double *inv_rowmajor)
{
    if (bad_order(a_len, n)) return MI32_BAD_SHAPE;
    return host_invert(a_rowmajor, n, 1, inv_rowmajor, nullptr, nullptr);
}

int mi32_matrix_inversion_no_pivots(const double *a_rowmajor, size_t a_len, int n, double *inv_rowmajor)
{
    if (bad_order(a_len, n)) return MI32_BAD_SHAPE;
    return host_invert(a_rowmajor, n, 1, inv_rowmajor, nullptr, nullptr, false);
}

int mi32_bench_64(const double *a_rowmajor, size_t a_len, int n, double *inv_rowmajor, double *times10, int pivoting)
{
    if (!times10 || bad_order(a_len, n)) return MI32_BAD_SHAPE;
    return host_invert(a_rowmajor, n, 1, inv_rowmajor, nullptr, times10, pivoting != 0);
}

// matrix_multiply of the reference (matrix_multiply.cpp:15-212): C = A * B in double on the device, returns
// sqrt(N) - ||C||_F -- the scalar the experiment driver writes per size (main_file.cpp:80-81).
int mi32_matrix_multiply_64(const double *a, const double *b, size_t len, double *errore)
{
    if (!a || !b || !errore || len == 0) return MI32_BAD_SHAPE;
    const int n = (int)std::llround(std::sqrt((double)len));  // the reference takes the order as sqrt(size), :44
    if (n <= 0 || (size_t)n * n != len) return MI32_BAD_SHAPE;
    mi32_context *h = nullptr;
    int rc = default_context(&h);
    if (rc != MI32_OK) return rc;
    std::lock_guard<std::mutex> lk(g_host_call_mu);
    MI32_HIP(hipSetDevice(h->device));
    rc = ensure_io(h, 2 * len, 1);
    if (rc != MI32_OK) return rc;
    {
        std::lock_guard<std::mutex> lk2(h->mu);
        rc = ensure_ws(h, residual_workspace_bytes(n, 1) + 64);
    }
    if (rc != MI32_OK) return rc;
    double *da = reinterpret_cast<double *>(h->d_in), *db = reinterpret_cast<double *>(h->d_out);
    rc = host_copy(h, da, const_cast<double *>(a), len * sizeof(double), true);
    if (rc != MI32_OK) return rc;
    rc = host_copy(h, db, const_cast<double *>(b), len * sizeof(double), true);
    if (rc != MI32_OK) return rc;
    double *d_out = reinterpret_cast<double *>((char *)h->ws + residual_workspace_bytes(n, 1));
    hipError_t e = frobenius_launch_f64(da, db, n, d_out, h->ws, h->stream);
    if (e != hipSuccess) return fail(e, "matrix_multiply launch");
    MI32_HIP(hipMemcpyAsync(errore, d_out, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    MI32_HIP(hipStreamSynchronize(h->stream));
    return MI32_OK;
}

int mi32_last_timing(double *total_seconds, double *compute_seconds)
{
    std::lock_guard<std::mutex> lk(g_host_call_mu);
    if (total_seconds) *total_seconds = g_last_total;
    if (compute_seconds) *compute_seconds = g_last_compute;
    return MI32_OK;
}

}  // extern "C"

// ---- the reference's C++ entry points, unchanged signatures ------------------------------------------------

// The std::vector drop-ins: {} for a bad shape (mat_inv_32.cpp:206-215) and for a failure.  README.md:54 "In case of
// invalid matrix an empty vector is returned", and the experiment twins do so for a singular input (their
// exact-identity checks, matrix_inversion_FP32.cpp:814-835, matrix_inversion_FP64.cpp:846-867,
// matrix_inversion_no_pivots.cpp:670).  MI32_SINGULAR_KEEP=1 returns the inf/NaN result instead, as the shipped
// library does.
template <typename T>
static std::vector<T> invert_to_vector(const std::vector<T> &matrix_vector, int matrix_order, bool pivoting,
                                       const char *name)
{
    if (bad_order(matrix_vector.size(), matrix_order)) return {};
    // the result vector comes into being (value-initialised, every page touched) while the device works
    std::vector<T> result;
    struct Ctx { std::vector<T> *v; size_t n; } ctx = {&result, (size_t)matrix_order * matrix_order};
    const int rc = host_invert<T>(matrix_vector.data(), matrix_order, 1, nullptr, nullptr, nullptr, pivoting,
                                  [](void *c) -> void * {
                                      Ctx *x = static_cast<Ctx *>(c);
                                      try {
                                          x->v->reserve(x->n);  // pages first (several threads), then the value-initialisation
                                          parallel_populate(x->v->data(), x->n * sizeof(T));
                                          x->v->resize(x->n);
                                      } catch (...) { return nullptr; }
                                      return x->v->data();
                                  }, &ctx);
    if (rc == MI32_OK) return result;
    if (rc == MI32_SINGULAR && env_int("MI32_SINGULAR_KEEP", 0)) return result;
    if (rc == MI32_RUNTIME_ERROR) std::fprintf(stderr, "%s: %s\n", name, mi32_last_error());
    return {};
}

// The benchmark twins (FP32_bench.cpp:11): the inverse and the ten timing slots, an empty Res where the reference
// returns one (bad shape, :212-217; error paths, :456).
template <typename T>
static Res bench_to_res(const std::vector<T> &matrix_vector, int matrix_order, bool pivoting, std::vector<T> Res::*inverse)
{
    Res res;
    if (bad_order(matrix_vector.size(), matrix_order)) return res;
    std::vector<T> inv((size_t)matrix_order * matrix_order, T(0));
    std::vector<double> times(10, 0.0);
    if (host_invert(matrix_vector.data(), matrix_order, 1, inv.data(), nullptr, times.data(), pivoting) != MI32_OK)
        return res;
    res.*inverse = std::move(inv);
    res.times = std::move(times);
    return res;
}

// Matlab/mat_inv_32.h:4
std::vector<float> matrix_inv_32(std::vector<float> matrix_vector, int matrix_order)
{
    return invert_to_vector(matrix_vector, matrix_order, true, "matrix_inv_32");
}

// the experiment twin of matrix_inv_32 (headers.h:7, matrix_inversion_FP32.cpp:11): same call shape
std::vector<float> matrix_inversion_FP32(std::vector<float> matrix_vector, int matrix_order)
{
    return matrix_inv_32(static_cast<std::vector<float> &&>(matrix_vector), matrix_order);
}

// matrix_inversion/headers.h:9
std::vector<double> matrix_inversion_FP64(std::vector<double> matrix_vector, int matrix_order)
{
    return invert_to_vector(matrix_vector, matrix_order, true, "matrix_inversion_FP64");
}

// matrix_inversion/headers.h:11: the diagonal entry is every step's pivot
std::vector<double> matrix_inversion_no_pivots(std::vector<double> matrix_vector, int matrix_order)
{
    return invert_to_vector(matrix_vector, matrix_order, false, "matrix_inversion_no_pivots");
}

// matrix_inversion/headers.h:13-16
Res FP32_bench(std::vector<float> matrix_vector, int matrix_order)
{
    return bench_to_res(matrix_vector, matrix_order, true, &Res::inversa32);
}
Res FP64_bench(std::vector<double> matrix_vector, int matrix_order)
{
    return bench_to_res(matrix_vector, matrix_order, true, &Res::inversa64);
}
Res no_pivots_bench(std::vector<double> matrix_vector, int matrix_order)
{
    return bench_to_res(matrix_vector, matrix_order, false, &Res::inversa64);
}

// headers.h:5, matrix_multiply.cpp:15: sqrt(N) - ||A * B||_F, N = sqrt(size)
double matrix_multiply(std::vector<double> matriceA, std::vector<double> matriceB)
{
    double errore = std::nan("");
    if (matriceA.size() != matriceB.size()) return errore;
    const int rc = mi32_matrix_multiply_64(matriceA.data(), matriceB.data(), matriceA.size(), &errore);
    if (rc == MI32_RUNTIME_ERROR) std::fprintf(stderr, "matrix_multiply: %s\n", mi32_last_error());
    return errore;
}
