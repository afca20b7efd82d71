// mi32_context.h -- what the host units of libmat_inv_32.so share: the context, the settings launch planning reads,
// the grow-only device buffer, error reporting, and the declarations that cross unit boundaries.
//   mi32_plan.hip     launch planning, pure host code: no HIP runtime call, no context; a dense call is planned once,
//                     as a DenseRoute
//   mi32_context.hip  context life cycle, setters, workspace, profiler
//   mi32_device.hip   the device-pointer entry points; one inv_device<T> enqueues every DenseRoute, with or without the
//                     determinant
//   mi32_hostptr.hip  the host-pointer entry points and the C++ drop-ins of the reference's headers
#pragma once
#include <cstdlib>
#include <functional>
#include <mutex>
#include <string>

#include "mi32_internal.h"

struct HostCopier;  // mi32_hostptr.hip

// internal to the library: none of this is an exported symbol
#pragma GCC visibility push(hidden)

// ---- errors ---------------------------------------------------------------------------------------------------------
extern thread_local std::string g_last_error;  // mi32_last_error(); defined in mi32_context.hip
// MI32_OK for hipSuccess; else sets g_last_error ("what: HIP's text") and returns MI32_RUNTIME_ERROR
int hip_status(hipError_t e, const char *what);
// return from the calling function unless the library call / the HIP call succeeded
#define MI32_TRY(call)                    \
    do {                                  \
        const int rc__ = (call);          \
        if (rc__ != MI32_OK) return rc__; \
    } while (0)
#define MI32_HIP(call) MI32_TRY(hip_status((call), #call))

inline int env_int(const char *name, int dflt)
{
    const char *s = std::getenv(name);
    return (s && *s) ? std::atoi(s) : dflt;
}

// ---- settings ---------------------------------------------------------------------------------------------------------
// What launch planning reads of a context (the mi32_set_* calls write it); a call without a context plans with the
// defaults.  0 / AUTO: the environment's value, then the built-in choice (see mi32_plan.hip, the one reader of each knob).
struct Settings {
    int algo = MI32_ALGO_AUTO;
    bool pivoting = true;  // false: the reference's no-pivot variant (the diagonal entry is every step's pivot)
    int panel_w = 0;
    int block_w = 0;
    bool lookahead = true;  // false: no second stream, neither for the look-ahead half nor for a split batch
};

// ---- grow-only device memory --------------------------------------------------------------------------------------------
// The workspace, the context's own status words and the staging of the host-pointer calls.  ensure() returns at once
// while the block is large enough; to grow it waits for every stream of the context, frees and allocates anew (the
// contents are lost).
struct DeviceBuffer {
    void *ptr = nullptr;
    size_t bytes = 0;
    int ensure(mi32_context *h, size_t want);
    void release();
};

void host_copier_destroy(HostCopier *c);

// ---- the diagnostic guard mode of the workspace (off unless a test called mi32_debug_ws_guard) -------------------------
// One carve a call makes: whose it is, where it starts in its buffer, and its regions in order (offsets from `base`).
struct WsCarve {
    enum Owner { INVERSE = 0, DET = 1, RESIDUAL = 2 };
    int owner;
    int part;     // 0 / 1 for the halves of a split batch
    size_t base;  // bytes into the buffer: the workspace, or (DET) the det memory
    size_t bytes;
    mi32::WsRegions regions;
};
// A red zone armed by the last guarded call on a context: bytes [off, off + bytes) of its buffer hold `pattern` in
// every 32-bit word.  region: index into the carve's regions of the region in front of the zone, -1 for the leading one
// (which is named after the first region).
struct WsZone {
    int owner, part, region;
    const char *name;
    size_t off, bytes;
    uint32_t pattern;
};
// the poison of the value regions and of the zones behind them: a quiet NaN as a float, and two of it as a double
static constexpr uint32_t kWsPoison = 0x7FF8DEADu;
// What the tests-only entry points mi32_debug_ws_layout and mi32_debug_ws_check fill (like mi32_debug_dense_route they
// are not part of include/mat_inv_32_c.h; tests/workspace_cases.py mirrors the two structs).
struct mi32_debug_ws_region {
    int owner, part, kind, reserved;  // WsCarve::Owner, 0 / 1, mi32::WsKind
    size_t offset, bytes;             // offset: from the start of the buffer (the det memory for owner 1, else the workspace)
    char name[16];
};
struct mi32_debug_ws_report {
    int checked, damaged;  // zones compared with their pattern / that differ from it
    // the first damaged zone (all zero and an empty name while damaged == 0): its index among the zones of the call, its
    // carve, the region it lies behind (the first region for a leading zone)
    int zone, owner, part, reserved;
    long long offset;      // of the first changed byte from that region's end; from its start, negative, in a leading zone
    size_t bytes;          // changed bytes in that zone
    char name[16];
};

struct mi32_context {
    int device = 0;
    Settings set;
    HostCopier *copier = nullptr;  // made by the first host-pointer call large enough to use it
    mi32::Profiler *prof = nullptr;  // an EventProfiler (mi32_context.hip) while profiling is on
    hipEvent_t switch_event = nullptr;
    hipStream_t aux_stream = nullptr;   // look-ahead half of the rank-bw updates (lowest priority)
    hipStream_t split_stream = nullptr; // second half of a split batch (same priority as the main stream)
    hipEvent_t la_events[8] = {};
    int cu_count = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    DeviceBuffer ws;
    // staging for the host-pointer entry points
    DeviceBuffer d_in, d_out, d_status;
    // status words of device-resident calls that pass no status buffer: the kernels always have one to flag
    // a bad pivot or a lost panel partner in (a given-up matrix is then skipped and comes out as NaN)
    DeviceBuffer d_istatus;
    // det calls above order 128 (mi32_inv_det_any_device*): the recorded pivots, the parity and input-flag words
    DeviceBuffer det;
    std::vector<WsZone> zones;  // guard mode: what the last call armed (mi32_debug_ws_check)
    std::mutex mu;
};
inline Settings settings_of(const mi32_context *h) { return h ? h->set : Settings(); }

int visible_devices(int *count);  // MI32_RUNTIME_ERROR when there is none
int sync_all_streams(mi32_context *h);
// the status buffer a device-resident call runs with: the caller's, or the context's own
int status_buffer(mi32_context *h, int *d_status, int batch, int **out);
// the same, zeroed on the stream (MI32_OK): for the kernels that only ever raise a member's flag
int zeroed_status_buffer(mi32_context *h, int *d_status, int batch, int **out);

// ---- launch planning (mi32_plan.hip) --------------------------------------------------------------------------------------
int resolve_algo(const Settings &s, int n, size_t elem_bytes);
bool blocked_supported(int n);  // fp32: the register-resident panel holds at most 16384 (padded) rows
mi32::BlockedRoute plan_route(const Settings &s, int n, int batch, bool aux_stream, bool split_stream);
// with what the context offers; a null handle plans as a fresh context does
inline mi32::BlockedRoute route_of(const mi32_context *h, const Settings &s, int n, int batch)
{
    return plan_route(s, n, batch, !h || h->aux_stream, !h || h->split_stream);
}
// How one dense call (a uniform batch at device pointers) runs, decided once: the path, the one plan object that path
// carves and launches with, the workspace the call ensures, and what a det call must know of the path's pivot list.
// dense_route composes resolve_algo, plan_route, block_w64 and the make_*_plan functions and holds no rule of its own;
// mi32_inv_device*, mi32_inv_det_any_device*, mi32_workspace_bytes, mi32_reserve and the mi32_resolve_* queries all
// read this one description.
struct DenseRoute {
    enum Path { RESIDENT, WORKGROUP, SWEEP, BLOCKED32, BLOCKED64, NOPIVOT64, WIDE } path;
    union {  // the member `path` names; none on the one-launch paths
        mi32::SweepPlan sweep;
        mi32::BlockedRoute blocked;
        mi32::Blocked64Plan blocked64;
        mi32::NoPivot64Plan nopivot64;
    };
    // The path's *_workspace_bytes of the plan above.  fp32: at least the residual check's share; BLOCKED32: the whole
    // batch, or the two halves of a split one (the same number of bytes unless the guard mode adds red zones).
    size_t ws_bytes;
    int det_steps;  // entries of a member's pivot list: the padded step count (0: the one-launch kernels keep no list)
    int det_first;  // the first real step: BLOCKED32 and NOPIVOT64 pad in front of the matrix, BLOCKED64 behind it
    bool one_launch() const { return path == RESIDENT || path == WORKGROUP || path == WIDE; }
};
// h: the streams a context offers (null: a fresh context's); they reach no field but the blocked fp32 route's look-ahead
// and parts
DenseRoute dense_route(const mi32_context *h, const Settings &s, int n, int batch, size_t elem_bytes);
// The carves a call on this route makes, by the size-only passes of the carves themselves: the path's (both parts of a
// split batch; none on the one-launch paths) and, with det, the det memory's.
std::vector<WsCarve> dense_carves(const DenseRoute &d, int batch, size_t elem_bytes, bool det);
WsCarve residual_carve_of(int n, int batch);
// Guard mode only (g_ws_guard != 0), after the buffers were ensured: waits for the context's streams, fills every value
// region and every zone behind one with kWsPoison and every other zone with zero, on the main stream, waits for that,
// and remembers the zones.  The index and record regions are left as they are.
int guard_arm(mi32_context *h, const std::vector<WsCarve> &carves);
void lookahead_geometry(int cus, int n, int *workgroups, bool *exclusive);

// An instance of the one-launch kernels: register-resident with `lanes` per member (8 ... 64), or workgroup-resident
// with `rows_per_thread` (40 ... 64); the other field is 0.
struct KernelInstance {
    int lanes, rows_per_thread;
    bool operator==(const KernelInstance &o) const { return lanes == o.lanes && rows_per_thread == o.rows_per_thread; }
};
// The kernel classes of a variable-size batch, in launch order: class k takes the orders whose resident_lanes /
// workgroup_rows_per_thread are kVbatchClass[k]'s.
static constexpr int kVbatchClasses = 8;
extern const KernelInstance kVbatchClass[kVbatchClasses];

// A variable-size batch plan (mi32_vbatch_create): immutable after creation.  The orders and the sorted member list
// are the only device memory it owns, 8 bytes per member.
struct mi32_vbatch {
    int device = 0;
    int batch = 0;
    int class_begin[kVbatchClasses + 1] = {};  // class k takes d_members[class_begin[k] .. class_begin[k + 1])
    // the members of order n are d_members[order_begin[n] .. order_begin[n + 1]), n = 1 ... 128 (host only: the solve's
    // launches follow the width n + columns, not the order's class)
    int order_begin[mi32::kWorkgroupMaxOrder + 2] = {};
    int *d_orders = nullptr;   // int[batch], the caller's member order
    int *d_members = nullptr;  // int[batch], member indices in ascending order of their orders (stable)
};
int vbatch_sort(const int *orders, int batch, int *perm, int *class_begin, int *order_begin);

// A X = B: one launch of a call, the `count` sorted members from `first` on (of a uniform batch: all of them) with the
// columns col0 ... col0 + cols - 1 of their B.  The six ints are what mi32_vbatch_solve_launches reports per launch.
struct SolveLaunch {
    int first, count, col0, cols;
    KernelInstance kernel;
};
using SolveLaunchFn = std::function<bool(const SolveLaunch &)>;  // false ends the walk
int solve_chunk_cols(int n);  // the widest chunk of columns beside an order; 0: the order has no spare column
// the launches of a uniform batch of order n, then of a plan's members (order_begin as in mi32_vbatch), in the order
// they are enqueued; solve_chunk_cols(n) > 0 / vsolve_has_columns(order_begin) is the caller's business
void solve_walk(int n, int batch, int nrhs, const SolveLaunchFn &f);
void vsolve_walk(const int *order_begin, int nrhs, const SolveLaunchFn &f);
bool vsolve_has_columns(const int *order_begin);  // no member of an order without a spare column

// ---- device-pointer calls (mi32_device.hip) ---------------------------------------------------------------------------
// One inversion with the settings given, whatever the context's own are: the DenseRoute of the call, enqueued.  det:
// where the determinants go (empty: none); d_inv may be null only with one.  The caller holds h->mu and has checked the
// arguments.  T = float or double (instantiated in mi32_device.hip).
template <typename T>
int inv_device(mi32_context *h, Settings s, const T *d_a, int n, int batch, T *d_inv, int *d_status,
               mi32::DetOut det = {nullptr, nullptr});

#pragma GCC visibility pop
