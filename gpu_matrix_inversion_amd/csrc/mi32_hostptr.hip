// mi32_hostptr.hip -- the host-pointer entry points of libmat_inv_32.so on the default context, the batch over several
// GPUs, and the C++ drop-ins of include/mat_inv_32.h, mat_inv_64.h and mat_inv_bench.h.
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <new>
#include <thread>
#include <type_traits>
#include <vector>

#include <sys/mman.h>

#include "mat_inv_32.h"
#include "mat_inv_64.h"
#include "mat_inv_bench.h"
#include "mi32_context.h"

using namespace mi32;
using Clock = std::chrono::steady_clock;

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
    ~HostCopier()  // also after an init that failed half way
    {
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
    // This lane's chunks are t, t + kLanes, ...; its k-th goes through pinned buffer k & 1, whose event marks the end
    // of the DMA.  To the device: fill the buffer once the DMA that last read it is done, then start this chunk's.
    // From the device: start the next chunk's DMA into the other buffer, then wait for this chunk's and empty it.
    hipError_t lane_copy(int t)
    {
        const size_t nchunks = (j_bytes + kChunk - 1) / kChunk;
        const size_t mine = (size_t)t < nchunks ? (nchunks - t + kLanes - 1) / kLanes : 0;
        char *dev = (char *)j_dev, *host = (char *)j_host;
        auto offset = [&](size_t k) { return (t + k * kLanes) * kChunk; };
        auto length = [&](size_t k) { return j_bytes - offset(k) < kChunk ? j_bytes - offset(k) : kChunk; };
        auto start_dma = [&](size_t k) {
            char *d = dev + offset(k), *p = pin[t][k & 1];
            hipError_t e = j_to_device ? hipMemcpyAsync(d, p, length(k), hipMemcpyHostToDevice, stream[t])
                                       : hipMemcpyAsync(p, d, length(k), hipMemcpyDeviceToHost, stream[t]);
            if (e == hipSuccess) e = hipEventRecord(ev[t][k & 1], stream[t]);
            return e;
        };
        hipError_t e = hipSuccess;
        if (!j_to_device && mine > 0) e = start_dma(0);
        for (size_t k = 0; k < mine && e == hipSuccess; ++k) {
            if (j_to_device) {
                if (k >= 2) e = hipEventSynchronize(ev[t][k & 1]);
                if (e != hipSuccess) break;
                std::memcpy(pin[t][k & 1], host + offset(k), length(k));
                e = start_dma(k);
            } else {
                if (k + 1 < mine) e = start_dma(k + 1);
                if (e == hipSuccess) e = hipEventSynchronize(ev[t][k & 1]);
                if (e != hipSuccess) break;
                std::memcpy(host + offset(k), pin[t][k & 1], length(k));
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

void host_copier_destroy(HostCopier *c) { delete c; }

// A context of the host-pointer entry points, made on first use and kept.  mu guards its staging buffers: one
// host-pointer call at a time per context.
namespace {
struct HostSlot {
    mi32_context *h = nullptr;
    std::mutex mu;
    int context(int device) { return h ? MI32_OK : mi32_create(&h, device); }  // the caller holds mu
};
// The default context serves every host-pointer entry point (fp32 and fp64 alike) but the batch over several GPUs:
// ONE mutex serialises them all, and guards the two timing words below.
HostSlot g_default;
double g_last_total = 0.0, g_last_compute = 0.0;
// the batch over several GPUs: logical GPU -> slot (never shrinks; slots are never freed)
std::mutex g_multi_mu;  // guards the table
std::vector<HostSlot *> g_multi;
}  // namespace

// staging of a host-pointer call: input and output of io_bytes each, one status word per matrix
static int ensure_io(mi32_context *h, size_t io_bytes, size_t ints)
{
    for (DeviceBuffer *b : {&h->d_in, &h->d_out}) MI32_TRY(b->ensure(h, io_bytes));
    return h->d_status.ensure(h, ints * sizeof(int));
}

// dev <- host (to_device) or host <- dev; synchronous.  Large transfers go through the pinned ring of HostCopier
// (MI32_HOST_COPY=0 keeps the runtime's pageable path), small ones through one hipMemcpyAsync.
static int host_copy(mi32_context *h, void *dev, void *host, size_t bytes, bool to_device)
{
    if (bytes >= HostCopier::kMinBytes && env_int("MI32_HOST_COPY", 1) != 0) {
        if (!h->copier && !(h->copier = new (std::nothrow) HostCopier())) return MI32_RUNTIME_ERROR;
        MI32_HIP(h->copier->init(h->device));
        MI32_HIP(hipStreamSynchronize(h->stream));  // the lanes' streams are not ordered with the context's stream
        MI32_HIP(h->copier->run(dev, host, bytes, to_device));
        return MI32_OK;
    }
    if (to_device) MI32_HIP(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, h->stream));
    else MI32_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, h->stream));
    MI32_HIP(hipStreamSynchronize(h->stream));
    return MI32_OK;
}

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

// `late_out`: where the result goes is only asked for once the kernels are queued -- the std::vector entry points
// allocate and first-touch their 4 N^2 result bytes (64 MiB of page faults at N = 4096, ~8 ms) while the device works
template <typename T>
using LateOut = std::function<T *()>;

// One host-pointer inversion: what the caller asks for, and the host clock stamps of the call.
template <typename T>
struct HostJob {
    const T *a;
    int n, batch;
    T *inv;                       // null with late_out
    int *status = nullptr;        // may be null
    double *times10 = nullptr;    // may be null: the reference's timing vector, see fill_times10
    bool pivoting = true;         // the variant of this one call, whatever the context's setting
    LateOut<T> late_out = nullptr;
    // the reference's two numbers ("Tempo Totale Impiegato" / "Tempo Computazione", mat_inv_32.cpp:385-386), written
    // once the result has arrived
    double *total_s = nullptr, *compute_s = nullptr;
    // tq0: before the context, t0: after it, t1: H2D done, t2: compute done, t3: D2H done
    Clock::time_point tq0, t0, t1, t2, t3;
};
static double seconds(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double>(b - a).count(); }

// The reference's ten timing slots (FP32_bench.cpp:256-443 / res_struct.h:4-6) from the profiler's per-class
// milliseconds and the clock stamps of the call -- [0] queue/context, [1] buffers (+ the H2D copy the reference's
// CL_MEM_COPY_HOST_PTR does), [2] program build, [3] makeAugmented, [4] pivot, [5] row, [6] column, [7] compute,
// [8] getInverted (+ D2H), [9] total; seconds.  The per-phase slots come from HIP events on the launch stream
// (mi32_set_profiling).
template <typename T>
static void fill_times10(const HostJob<T> &j, const double *ms)
{
    double *times10 = j.times10;
    times10[0] = seconds(j.tq0, j.t0);
    times10[1] = seconds(j.t0, j.t1);
    times10[2] = 0.0;  // one ahead-of-time compiled code object: nothing is built at run time
    times10[3] = ms[KC_INIT] * 1e-3;
    // the panel kernel IS maxPivot + finalMaxPivot + pivotElements + fixRow (+ fixColumn on the panel's own columns); the
    // fused step launches of the sweep path are accounted to the column slot, where the reference spends its time
    times10[4] = ms[KC_PANEL] * 1e-3;
    times10[5] = 0.0;  // fixRow has no launch of its own
    times10[6] = (ms[KC_SWEEP_STEP] + ms[KC_UPDATE_IN] + ms[KC_UPDATE_OUT] + ms[KC_TRANSPOSE]) * 1e-3;
    times10[7] = seconds(j.t1, j.t2);
    times10[8] = ms[KC_FINISH] * 1e-3 + seconds(j.t2, j.t3);
    times10[9] = seconds(j.tq0, j.t3);
}

// The host-pointer path: job j (j.tq0 set) on context h; the caller holds the lock that guards h's staging buffers.
template <typename T>
static int host_invert_on(mi32_context *h, HostJob<T> &j)
{
    j.t0 = Clock::now();
    MI32_HIP(hipSetDevice(h->device));
    const int n = j.n, batch = j.batch;
    const size_t elems = (size_t)batch * n * n;
    MI32_TRY(ensure_io(h, elems * sizeof(T), (size_t)batch));
    ProfilingGuard prof_guard;  // profiling is switched off again on every way out
    if (j.times10) {
        // fp32: workspace allocation belongs to the "buffers" slot
        if (std::is_same<T, float>::value) MI32_TRY(mi32_reserve(h, n, batch));
        MI32_TRY(mi32_set_profiling(h, 1));
        prof_guard.h = h;
        double ms[KC_COUNT]; long long cnt[KC_COUNT];
        (void)mi32_get_profile(h, ms, cnt, KC_COUNT);  // drop what an earlier call left
    }
    T *d_in = static_cast<T *>(h->d_in.ptr), *d_out = static_cast<T *>(h->d_out.ptr);
    int *d_status = static_cast<int *>(h->d_status.ptr);
    MI32_TRY(host_copy(h, d_in, const_cast<T *>(j.a), elems * sizeof(T), true));
    j.t1 = Clock::now();
    {
        std::lock_guard<std::mutex> lk(h->mu);
        Settings s = h->set;
        s.pivoting = j.pivoting;
        MI32_TRY(inv_device(h, s, d_in, n, batch, d_out, d_status));
    }
    T *inv = j.inv;
    if (j.late_out) {
        inv = j.late_out();
        if (!inv) { (void)hipStreamSynchronize(h->stream); return MI32_RUNTIME_ERROR; }
    } else {
        parallel_populate(inv, elems * sizeof(T), true);  // the device is busy for the next milliseconds
    }
    MI32_HIP(hipStreamSynchronize(h->stream));
    j.t2 = Clock::now();
    std::vector<int> st((size_t)batch);
    MI32_HIP(hipMemcpyAsync(st.data(), d_status, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    MI32_TRY(host_copy(h, d_out, inv, elems * sizeof(T), false));
    MI32_HIP(hipStreamSynchronize(h->stream));
    j.t3 = Clock::now();
    if (j.total_s) *j.total_s = seconds(j.t0, j.t3);
    if (j.compute_s) *j.compute_s = seconds(j.t1, j.t2);
    if (j.times10) {
        double ms[KC_COUNT]; long long cnt[KC_COUNT];
        MI32_TRY(mi32_get_profile(h, ms, cnt, KC_COUNT));
        fill_times10(j, ms);
    }
    int worst = MI32_OK;
    for (int b = 0; b < batch; ++b) {
        if (j.status) j.status[b] = st[(size_t)b];
        if (st[(size_t)b] > worst) worst = st[(size_t)b];
    }
    if (worst == MI32_RUNTIME_ERROR)  // the only status-borne runtime error (mi32_blocked.hip, fp32 shared panels)
        g_last_error = "a workgroup of a shared panel timed out waiting for its partners (the device was not ours "
                       "alone); the affected inverse is NaN-filled -- retry, or set MI32_MULTI_PANEL=0";
    return worst;
}

// the caller holds g_default.mu
static void print_reference_timing_lines()
{
    if (!env_int("MI32_VERBOSE", 0)) return;
    // the reference's two stdout lines (mat_inv_32.cpp:385-386)
    std::printf("Tempo Totale Impiegato: %g seconds\nTempo Computazione: %g seconds\n", g_last_total, g_last_compute);
    std::fflush(stdout);
}

// One host-pointer inversion on the default context.  The fp32 calls print the reference's timing lines.
template <typename T>
static int host_invert(HostJob<T> j)
{
    if (!j.a || (!j.inv && !j.late_out) || j.n <= 0 || j.batch <= 0) return MI32_BAD_SHAPE;
    j.total_s = &g_last_total;
    j.compute_s = &g_last_compute;
    j.tq0 = Clock::now();
    std::lock_guard<std::mutex> lk(g_default.mu);
    // the reference's platform / device / context / queue bring-up (cached here)
    MI32_TRY(g_default.context(env_int("MI32_DEVICE", 0)));
    const int rc = host_invert_on(g_default.h, j);
    if (std::is_same<T, float>::value && (rc == MI32_OK || rc == MI32_SINGULAR || rc == MI32_RUNTIME_ERROR))
        print_reference_timing_lines();
    return rc;
}

// the reference's shape guards, mat_inv_32.cpp:206-215 (integer division included); matrix_inversion_FP64.cpp
// has the same two
static bool bad_order(size_t a_len, int n) { return n <= 0 || (int)(a_len / (size_t)n) != n; }

// ---- the batch over several GPUs (what replaces the reference's platforms[0] / devices[0],
//      mat_inv_32.cpp:239-244) -------------------------------------------------------------------------
// One context and one host thread per GPU; GPU g owns the matrices of mi32_shard_range(batch, ngpus, g)
// and copies ITS OWN shard host -> device, inverts it and copies it back: no data-path exchange between the GPUs,
// the worst status word is the return value.  The contexts are created on first use and kept.
// MI32_MULTI_OVERSUBSCRIBE=1 (tests, single-GPU hosts): logical GPU g runs on device g % (visible devices), each with
// a context of its own -- the threading, the ragged shards and the status reduction run exactly as on a real node.
extern "C" {

int mi32_matrix_inv_32_batched_multi(const float *a, int n, int batch, float *inv, int *status, int ngpus)
{
    if (!a || !inv || n <= 0 || batch <= 0) return MI32_BAD_SHAPE;
    const auto tq0 = Clock::now();
    int visible = 0;
    MI32_TRY(visible_devices(&visible));
    const bool oversub = env_int("MI32_MULTI_OVERSUBSCRIBE", 0) != 0;
    if (ngpus <= 0) ngpus = visible;
    if (ngpus > visible && !oversub) {
        g_last_error = "mi32_matrix_inv_32_batched_multi: more GPUs asked for than are visible";
        return MI32_BAD_SHAPE;
    }
    if (ngpus > batch) ngpus = batch;  // at least one matrix per GPU
    std::vector<HostSlot *> slots((size_t)ngpus, nullptr);
    {
        std::lock_guard<std::mutex> lk(g_multi_mu);
        while ((int)g_multi.size() < ngpus) g_multi.push_back(new (std::nothrow) HostSlot());
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
        HostSlot *sl = slots[(size_t)g];
        std::lock_guard<std::mutex> lk(sl->mu);
        int rc = sl->context(g % visible);
        if (rc == MI32_OK) {
            HostJob<float> j{a + (size_t)lo * mat, n, hi - lo, inv + (size_t)lo * mat, status ? status + lo : nullptr};
            j.total_s = &tot[(size_t)g];
            j.compute_s = &cmp[(size_t)g];
            j.tq0 = tq0;
            rc = host_invert_on(sl->h, j);
        }
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
        std::lock_guard<std::mutex> lk(g_default.mu);
        g_last_total = t_tot;
        g_last_compute = t_cmp;
        print_reference_timing_lines();
    }
    return worst;
}

int mi32_matrix_inv_32_batched(const float *a, int n, int batch, float *inv, int *status)
{
    return host_invert(HostJob<float>{a, n, batch, inv, status});
}

int mi32_bench_32(const float *a_rowmajor, size_t a_len, int n, float *inv_rowmajor, double *times10)
{
    if (!times10 || bad_order(a_len, n)) return MI32_BAD_SHAPE;
    return host_invert(HostJob<float>{a_rowmajor, n, 1, inv_rowmajor, nullptr, times10});
}

int mi32_matrix_inv_32(const float *a_rowmajor, size_t a_len, int n, float *inv_rowmajor)
{
    if (bad_order(a_len, n)) return MI32_BAD_SHAPE;
    return host_invert(HostJob<float>{a_rowmajor, n, 1, inv_rowmajor});
}

int mi32_matrix_inv_64(const double *a_rowmajor, size_t a_len, int n, double *inv_rowmajor)
{
    if (bad_order(a_len, n)) return MI32_BAD_SHAPE;
    return host_invert(HostJob<double>{a_rowmajor, n, 1, inv_rowmajor});
}

int mi32_matrix_inversion_no_pivots(const double *a_rowmajor, size_t a_len, int n, double *inv_rowmajor)
{
    if (bad_order(a_len, n)) return MI32_BAD_SHAPE;
    return host_invert(HostJob<double>{a_rowmajor, n, 1, inv_rowmajor, nullptr, nullptr, false});
}

int mi32_bench_64(const double *a_rowmajor, size_t a_len, int n, double *inv_rowmajor, double *times10, int pivoting)
{
    if (!times10 || bad_order(a_len, n)) return MI32_BAD_SHAPE;
    return host_invert(HostJob<double>{a_rowmajor, n, 1, inv_rowmajor, nullptr, times10, pivoting != 0});
}

// matrix_multiply of the reference (matrix_multiply.cpp:15-212): C = A * B in double on the device, returns
// sqrt(N) - ||C||_F -- the scalar the experiment driver writes per size (main_file.cpp:80-81).
int mi32_matrix_multiply_64(const double *a, const double *b, size_t len, double *errore)
{
    if (!a || !b || !errore || len == 0) return MI32_BAD_SHAPE;
    const int n = (int)std::llround(std::sqrt((double)len));  // the reference takes the order as sqrt(size), :44
    if (n <= 0 || (size_t)n * n != len) return MI32_BAD_SHAPE;
    std::lock_guard<std::mutex> lk(g_default.mu);
    MI32_TRY(g_default.context(env_int("MI32_DEVICE", 0)));
    mi32_context *h = g_default.h;
    MI32_HIP(hipSetDevice(h->device));
    MI32_TRY(ensure_io(h, len * sizeof(double), 1));
    {
        std::lock_guard<std::mutex> lk2(h->mu);
        MI32_TRY(h->ws.ensure(h, residual_workspace_bytes(n, 1) + 64));
    }
    double *da = static_cast<double *>(h->d_in.ptr), *db = static_cast<double *>(h->d_out.ptr);
    MI32_TRY(host_copy(h, da, const_cast<double *>(a), len * sizeof(double), true));
    MI32_TRY(host_copy(h, db, const_cast<double *>(b), len * sizeof(double), true));
    double *d_out = reinterpret_cast<double *>((char *)h->ws.ptr + residual_workspace_bytes(n, 1));
    MI32_TRY(hip_status(frobenius_launch_f64(da, db, n, d_out, h->ws.ptr, h->stream), "matrix_multiply launch"));
    MI32_HIP(hipMemcpyAsync(errore, d_out, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    MI32_HIP(hipStreamSynchronize(h->stream));
    return MI32_OK;
}

int mi32_last_timing(double *total_seconds, double *compute_seconds)
{
    std::lock_guard<std::mutex> lk(g_default.mu);
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
    const size_t elems = (size_t)matrix_order * matrix_order;
    const LateOut<T> make_result = [&]() -> T * {
        try {
            result.reserve(elems);  // pages first (several threads), then the value-initialisation
            parallel_populate(result.data(), elems * sizeof(T));
            result.resize(elems);
        } catch (...) { return nullptr; }
        return result.data();
    };
    const int rc =
        host_invert(HostJob<T>{matrix_vector.data(), matrix_order, 1, nullptr, nullptr, nullptr, pivoting, make_result});
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
    const HostJob<T> job{matrix_vector.data(), matrix_order, 1, inv.data(), nullptr, times.data(), pivoting};
    if (host_invert(job) != MI32_OK) return res;
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
