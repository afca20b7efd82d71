// mi32_plan.hip -- launch planning of libmat_inv_32.so: which algorithm, which blocking, how much workspace, which
// kernel instance for which members and columns.  Pure host code: functions of the settings, the environment and the
// shape, no HIP runtime call and no context -- the mi32_resolve_* entry points answer with what a call would do.
// A dense call is planned once: dense_route composes the rules below into the DenseRoute (mi32_context.h) that the
// device entry, the workspace queries and mi32_resolve_blocking_f64 all read.
#include <cstring>

#include "mi32_apply.h"
#include "mi32_context.h"
#include "mi32_det_large.h"

using namespace mi32;

// Blocked from a measured cross-over on MI355X: fp32 32 rows, fp64 (windowed steps + rank-bw updates on the fp64
// matrix cores) 256 rows; the no-pivot variants 512 rows both (fp32: the W x W diagonal block is its whole "panel";
// fp64: a blocked path of its own, mi32_nopivot64.hip).  MI32_ALGO_SWEEP keeps the unblocked sweep.
int resolve_algo(const Settings &s, int n, size_t elem_bytes)
{
    const bool f32 = elem_bytes == sizeof(float);
    int algo = s.algo != MI32_ALGO_AUTO ? s.algo : env_int("MI32_ALGO", MI32_ALGO_AUTO);
    // the register-resident path holds orders up to 64; above, RESIDENT resolves to what AUTO resolves to
    if (algo == MI32_ALGO_RESIDENT && n <= kResidentMaxOrder) return algo;
    // MI32_ALGO_WORKGROUP up to 128 rows: the register-resident path takes the orders it holds, so that one setting
    // serves orders on both sides of 64; above 128 it resolves to what AUTO resolves to
    if (algo == MI32_ALGO_WORKGROUP && n <= kWorkgroupMaxOrder)
        return n <= kResidentMaxOrder ? MI32_ALGO_RESIDENT : MI32_ALGO_WORKGROUP;
    // MI32_ALGO_WIDE up to 256 rows in fp32: the two paths above take the orders they hold, so that one setting serves
    // every small order; above 256, and in fp64 above 128, it resolves to what AUTO resolves to
    if (algo == MI32_ALGO_WIDE && n <= (f32 ? kWideMaxOrder : kWorkgroupMaxOrder))
        return n <= kResidentMaxOrder ? MI32_ALGO_RESIDENT : n <= kWorkgroupMaxOrder ? MI32_ALGO_WORKGROUP : MI32_ALGO_WIDE;
    const int cross = !s.pivoting ? 512 : f32 ? 32 : 256;
    if (algo != MI32_ALGO_SWEEP && algo != MI32_ALGO_BLOCKED) algo = (n >= cross) ? MI32_ALGO_BLOCKED : MI32_ALGO_SWEEP;
    if (f32 && algo == MI32_ALGO_BLOCKED && !blocked_supported(n)) algo = MI32_ALGO_SWEEP;  // panel would not fit in registers
    return algo;
}

// (the update tiles address a matrix with 32-bit byte offsets from its base, so a working copy must stay below 4 GiB:
// mi32_blocked.hip asserts it for this bound)
bool blocked_supported(int n) { return n > 0 && ((n + 127) & ~127) <= 16384; }

// A knob whose every set value counts, the empty string included: atoi of it (MI32_MULTI_PANEL, MI32_LOOKAHEAD_MIN;
// env_int reads the empty string as unset).
static bool env_atoi(const char *name, int *value)
{
    const char *e = std::getenv(name);
    if (e) *value = std::atoi(e);
    return e != nullptr;
}

// THE route of a blocked fp32 call: every decision of the path, each rule once.  aux_stream / split_stream: what the
// context offers (a call without one plans as a fresh context does, with both).
BlockedRoute plan_route(const Settings &s, int n, int batch, bool aux_stream, bool split_stream)
{
    BlockedRoute r = {};
    const double elems = (double)batch * (double)n * (double)n;
    // ---- geometry
    r.n = n;
    r.np = (n + 127) & ~127;
    // Row stride: np + 64 floats (256 B): keeps rows 256-B aligned and avoids a power-of-two stride.
    r.ld = r.np + 64;
    r.pivoting = s.pivoting;
    int nt = (r.np >= 2048) ? 1024 : 512;
    int rpt = 1;
    while (rpt * nt < r.np) rpt *= 2;
    if (rpt > 8 && nt == 512) {  // no 512-thread instance holds more than 8 rows per lane: use 1024
        nt = 1024;
        rpt = 1;
        while (rpt * nt < r.np) rpt *= 2;
    }
    r.nthreads_panel = nt;
    r.rpt = rpt;
    int w = s.panel_w ? s.panel_w : env_int("MI32_PANEL_W", 0);
    if (w <= 0) w = 16;  // 32 is selectable where it fits, but measured slower (4.6 vs 4.2 ms at 2048^2)
    r.w = w = (w >= 32) ? 32 : (w >= 16) ? 16 : (w >= 8 ? 8 : 4);
    int bw = s.block_w ? s.block_w : env_int("MI32_BLOCK_W", 0);
    if (bw == 0) {
        // A single matrix is bound by the pivot chain and bw = 256 gives the rank-bw update its best
        // arithmetic intensity.  A batch that fills the GPU is bound by the HBM traffic of the in-block
        // updates (np x bw re-written per sub-panel): bw = 128 halves it (measured 64 x 2048^2:
        // 23.0 ms vs 24.7 ms; single 4096^2: 11.4 ms vs 11.2 ms).
        bw = (batch >= 8 && elems >= 64.0 * 1024.0 * 1024.0) ? 128 : 256;
        // (Rounds 1-2 ran N > 14336 with bw = 512 for the rank-bw update's sake: 120 instead of 114 TFLOP/s.  With the
        // pivot-row strips of round 3 an in-block update tile costs more and there are twice as many per sub-panel at
        // 512: 16384^2 122 ms at 256, 126 at 384, 140 at 512; 12288^2 65.5 vs 75.9; 8192^2 33.9 vs 38.0.)
    }
    if (bw <= 0) bw = 256;
    bw = (bw + 127) & ~127;
    if (bw > kMaxBW) bw = kMaxBW;
    if (bw > r.np) bw = r.np;
    r.bw = bw;
    r.nblk = (r.np + bw - 1) / bw;
    // ---- shared panels need every workgroup of a panel resident at once and a whole CU each; with the look-ahead
    // kernel holding all but 16 (32 below 8192 rows) CUs that is safe for a few matrices (MI32_MULTI_PANEL=0 turns
    // them off).  The no-pivot variant has no panel search to share: it ignores the flag, but a batch it is set for
    // is never split.
    bool multi_panel = nt == 1024 && r.np > kPanelGroupRows && batch * kMaxPanelGroups <= 16;
    int knob;
    if (env_atoi("MI32_MULTI_PANEL", &knob)) multi_panel = multi_panel && knob != 0;
    r.shared_panels = multi_panel && s.pivoting;
    // ---- per outer block
    for (int b = 0; b < r.nblk && b < 128; ++b) {
        int bnt, brpt;
        panel_geometry(r, r.np - b * bw, bnt, brpt);
        int wmax = ((bnt == 1024) ? 64 : 128) / brpt;  // floats of slab per thread
        if (wmax > kMaxW) wmax = kMaxW;
        int wb = w < wmax ? w : wmax;                  // wmax < 4 (np > 16384) is rejected by blocked_supported()
        wb = (wb >= 32) ? 32 : (wb >= 16) ? 16 : (wb >= 8 ? 8 : 4);
        // (the no-pivot variant has no register-resident panel whose rows would limit the width)
        r.wblk[b] = s.pivoting ? (unsigned char)wb : 16;
    }
    // Fused mode pays while the panel workgroup holds at most 2 rows per lane (measured: 2048^2 3.23 -> 3.06 ms,
    // 1024^2 1.40 -> 1.27 ms); with more rows the prologue (rows x W x W fmaf on ONE CU) costs what the update launch
    // did (4096^2: 8.9 -> 9.5 ms).  The first block with at most kFusedRows rows:
    r.first_fused = !s.pivoting ? r.nblk : r.np <= kFusedRows ? 0 : (r.np - kFusedRows + bw - 1) / bw;
    // ---- look-ahead: it pays when the GPU is otherwise idle during the panel phase: a single large matrix
    // (measured in round 1: 8192^2 51 -> 45 ms, 16384^2 399 -> 330 ms, 4096^2 11.2 -> 11.0 ms, 2048^2 4.2 -> 4.4 ms; with
    // the half on CUs of its own, round 2: 3584^2 7.39 -> 7.00 ms, 3072^2 5.79 -> 5.63, 2560^2 4.32 -> 4.34, 2048^2 3.01 -> 3.14)
    // Round 3 (reference-order arithmetic: the pivot rows' strip per block sits between the block's last panel and its
    // rank-bw update, and rides in the panel launches only WITHOUT the second stream), with / without:
    // 4096^2 10.23 / 10.09, 4352^2 11.50 / 11.66, 5120^2 15.02 / 15.79, 8192^2 34.0 / 37.1 -> on above 4096 padded rows.
    int la_min = 4096 + 1;
    if (env_atoi("MI32_LOOKAHEAD_MIN", &knob)) la_min = knob > 2048 ? knob : 2048;
    r.lookahead = s.lookahead && aux_stream && batch == 1 && r.np >= la_min;
    // ---- parts.  A GPU-filling batch is run as two halves on the context's two streams: the MFMA-bound rank-bw
    // launches of one half overlap the latency / HBM-bound sub-panel launches of the other (64 x 2048^2: 18.5 -> 17.4 ms;
    // three or four parts lose; round 3: 8 x 4096^2 23.6 -> 22.1 ms, 4 x 4096^2 15.7 -> 15.0: from four matrices on).
    // Both halves use the blocking of the whole batch, so a matrix's result does not depend on the split;
    // mi32_set_lookahead(h, 0) turns the second stream off altogether.  Plans with the shared-panel flag are not split:
    // a panel's workgroups need whole CUs at the same time, which the other half's rank-bw grid would keep from them
    // for the length of its launch.
    const bool split = split_stream && s.lookahead && batch >= 4 && elems >= 64.0 * 1024.0 * 1024.0 &&
                       env_int("MI32_BATCH_SPLIT", 1) != 0 && !multi_panel;
    r.parts = split ? 2 : 1;
    r.part_batch[0] = split ? (batch + 1) / 2 : batch;
    r.part_batch[1] = batch - r.part_batch[0];
    // The strip(t) tiles follow each block sub-panel by sub-panel in the columns outside it -- unless the look-ahead
    // is on: those columns are then still being written by the previous block's second-stream update while the
    // block's panels run (the next block's columns too: half (A) of the previous block covered THIS block's), and
    // the block's strips run in one launch at its end (gj_block_strip_kernel).  So do GPU-filling batches: there the
    // strip(t) tiles (256-thread groups, one global round trip per 32 earlier steps) cost more than the one launch
    // per block (measured 64 x 2048^2: 23.0 vs 21.7 ms).  Each part counts its own tiles.
    for (int i = 0; i < r.parts; ++i) r.part_strips_at_end[i] = r.lookahead || r.part_batch[i] * ((r.np + 63) / 64) > 256;
    return r;
}

static int block_w64(const Settings &s) { return s.block_w ? s.block_w : env_int("MI32_BLOCK_W64", 0); }

// THE description of a dense call.  Only the plan of the path that runs is built: a one-launch or sweep call plans no
// blocked route, a blocked fp32 call plans its route once and sizes its workspace from that same object.
DenseRoute dense_route(const mi32_context *h, const Settings &s, int n, int batch, size_t elem_bytes)
{
    const bool f32 = elem_bytes == sizeof(float);
    const int algo = resolve_algo(s, n, elem_bytes);
    DenseRoute d;
    d.ws_bytes = 0;  // the one-launch paths keep no working copy
    d.det_steps = d.det_first = 0;
    if (algo == MI32_ALGO_RESIDENT || algo == MI32_ALGO_WORKGROUP || algo == MI32_ALGO_WIDE) {
        d.path = algo == MI32_ALGO_RESIDENT ? DenseRoute::RESIDENT : algo == MI32_ALGO_WORKGROUP ? DenseRoute::WORKGROUP : DenseRoute::WIDE;
    } else if (algo == MI32_ALGO_SWEEP) {
        d.path = DenseRoute::SWEEP;
        d.sweep = make_sweep_plan(n);
        d.ws_bytes = sweep_workspace_bytes(d.sweep, batch, elem_bytes);
        d.det_steps = n;
    } else if (f32) {
        d.path = DenseRoute::BLOCKED32;
        // blocked_carve reads np, ld and bw only, and plan_route derives none of the three from the streams offered
        // (those reach `lookahead` and the parts): the route the call runs also sizes the workspace of any context
        const BlockedRoute &r = d.blocked = route_of(h, s, n, batch);
        // A split batch carves one workspace per half, the second where the first ends.  Every region is a whole number
        // of 256-byte units per member, so the two halves need exactly what the whole batch needs -- a context that
        // never splits reserves the same -- until the guard mode gives each carve its own red zones.
        const size_t whole = blocked_workspace_bytes(r, batch);
        const size_t halves = r.parts == 2 ? blocked_workspace_bytes(r, r.part_batch[0]) + blocked_workspace_bytes(r, r.part_batch[1]) : 0;
        d.ws_bytes = whole > halves ? whole : halves;
        d.det_steps = r.np;
        d.det_first = r.np - n;  // the identity padding comes first on this path: its steps are skipped by index
    } else if (s.pivoting) {
        d.path = DenseRoute::BLOCKED64;
        d.blocked64 = make_blocked64_plan(n, block_w64(s));
        d.ws_bytes = blocked64_workspace_bytes(d.blocked64, batch);
        d.det_steps = d.blocked64.np;
    } else {
        d.path = DenseRoute::NOPIVOT64;
        d.nopivot64 = make_nopivot64_plan(n, block_w64(s));
        d.ws_bytes = nopivot64_workspace_bytes(d.nopivot64, batch);
        d.det_steps = d.nopivot64.np;
        d.det_first = d.nopivot64.np - n;  // the identity padding comes first here too
    }
    if (f32) {  // mi32_residual_device checks an fp32 result in the same workspace
        const size_t res = residual_workspace_bytes(n, batch);
        if (res > d.ws_bytes) d.ws_bytes = res;
    }
    return d;
}

// ---- the workspace layout, for the diagnostic guard mode ------------------------------------------------------------------
std::atomic<size_t> mi32::g_ws_guard{0};

std::vector<WsCarve> dense_carves(const DenseRoute &d, int batch, size_t elem_bytes, bool det)
{
    std::vector<WsCarve> out;
    const auto add = [&](int owner, int part, size_t base, auto size_pass) {
        out.push_back(WsCarve{owner, part, base, 0, {}});
        out.back().bytes = size_pass(&out.back().regions);
    };
    switch (d.path) {
        case DenseRoute::SWEEP:
            add(WsCarve::INVERSE, 0, 0, [&](WsRegions *r) { return sweep_workspace_bytes(d.sweep, batch, elem_bytes, r); });
            break;
        case DenseRoute::BLOCKED32:
            // the second part's carve starts where the first part's ends (blocked_invert_split, mi32_device.hip)
            for (int part = 0; part < d.blocked.parts; ++part)
                add(WsCarve::INVERSE, part, part ? out[0].bytes : 0,
                    [&](WsRegions *r) { return blocked_workspace_bytes(d.blocked, d.blocked.part_batch[part], r); });
            break;
        case DenseRoute::BLOCKED64:
            add(WsCarve::INVERSE, 0, 0, [&](WsRegions *r) { return blocked64_workspace_bytes(d.blocked64, batch, r); });
            break;
        case DenseRoute::NOPIVOT64:
            add(WsCarve::INVERSE, 0, 0, [&](WsRegions *r) { return nopivot64_workspace_bytes(d.nopivot64, batch, r); });
            break;
        case DenseRoute::RESIDENT:
        case DenseRoute::WORKGROUP:
        case DenseRoute::WIDE: return out;  // the one-launch kernels carve nothing and keep no pivot list
    }
    if (det) add(WsCarve::DET, 0, 0, [&](WsRegions *r) { return det_bytes(d.det_steps, batch, elem_bytes, r); });
    return out;
}

WsCarve residual_carve_of(int n, int batch)
{
    WsCarve c{WsCarve::RESIDUAL, 0, 0, 0, {}};
    c.bytes = residual_workspace_bytes(n, batch, &c.regions);
    return c;
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
void lookahead_geometry(int cus, int n, int *workgroups, bool *exclusive)
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

// ---- variable-size batches ---------------------------------------------------------------------------------------
// 0 ... 3 the register-resident instances, 4 ... 7 the workgroup-resident ones
const KernelInstance kVbatchClass[kVbatchClasses] = {{8, 0}, {16, 0}, {32, 0}, {64, 0}, {0, 40}, {0, 48}, {0, 56}, {0, 64}};

// The kernel class of an order; resident_lanes and workgroup_rows_per_thread stay the single source of the
// boundaries.  -1: no instance takes the order.
static int vbatch_class(int n)
{
    const KernelInstance inst{resident_lanes(n), workgroup_rows_per_thread(n)};
    for (int k = 0; k < kVbatchClasses; ++k)
        if (kVbatchClass[k] == inst) return k;
    return -1;
}

// The counting sort behind mi32_vbatch_bin, O(batch) and stable; order_begin (may be null; int[kWorkgroupMaxOrder + 2]):
// the members of order n are perm[order_begin[n] .. order_begin[n + 1]).  perm and class_begin may be null too.
int vbatch_sort(const int *orders, int batch, int *perm, int *class_begin, int *order_begin)
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

// ---- A X = B on the one-launch paths ----------------------------------------------------------------------------------
// A call's nrhs columns are cut into chunks of at most solve_chunk_cols(n): what is left of one 64-lane group beside an
// order up to 32, of the workgroup's 128 columns above (0: no order of these kernels, or no spare column).  Full chunks
// first; every launch repeats the elimination of A.
int solve_chunk_cols(int n)
{
    return n < 1 || n >= kWorkgroupMaxOrder ? 0 : n <= 32 ? kResidentMaxOrder - n : kWorkgroupMaxOrder - n;
}
// THE rule, chunk width -> kernel: a chunk whose width n + cols fits a 64-lane group runs on the register-resident
// kernel (resident_lanes of the width), a wider one on the workgroup-resident kernel.
static KernelInstance solve_instance(int n, int cols)
{
    if (n + cols <= kResidentMaxOrder) return {resident_lanes(n + cols), 0};
    return {0, workgroup_solve_rows_per_thread(n)};
}
// How an order's chunks run.  Two orders' chunk sequences agree when these agree: col0 and cols of every chunk follow.
struct SolveChunks {
    int cols;              // columns of a full chunk (of the only chunk, when nrhs fits one)
    long long chunks;      // ceil(nrhs / cap)
    KernelInstance first;  // the kernel of the full chunks
    KernelInstance last;   // of the remainder (the same when there is none)
    bool operator==(const SolveChunks &o) const
    {
        return cols == o.cols && chunks == o.chunks && first == o.first && last == o.last;
    }
};
static SolveChunks solve_chunks(int n, int nrhs)
{
    const int cap = solve_chunk_cols(n);
    SolveChunks c;
    c.cols = nrhs < cap ? nrhs : cap;
    c.chunks = ((long long)nrhs + cap - 1) / cap;
    c.first = solve_instance(n, c.cols);
    c.last = solve_instance(n, (int)(nrhs - (c.chunks - 1) * cap));
    return c;
}
// one launch per chunk for the `count` members from `first` on; false: f ended the walk
static bool walk_chunks(const SolveChunks &c, int nrhs, int first, int count, const SolveLaunchFn &f)
{
    for (long long k = 0; k < c.chunks; ++k) {
        const long long col0 = k * c.cols;
        const int cols = (int)(nrhs - col0 < c.cols ? nrhs - col0 : c.cols);
        if (!f(SolveLaunch{first, count, (int)col0, cols, k + 1 < c.chunks ? c.first : c.last})) return false;
    }
    return true;
}

void solve_walk(int n, int batch, int nrhs, const SolveLaunchFn &f) { (void)walk_chunks(solve_chunks(n, nrhs), nrhs, 0, batch, f); }

// Every member is treated as a uniform batch of its order is; one run of launches for every maximal run of consecutive
// sorted members whose chunk sequences agree.  The one place the rule lives: mi32_vbatch_solve_launches reports this
// list and mi32_solve_device_vbatched* walks it.
void vsolve_walk(const int *order_begin, int nrhs, const SolveLaunchFn &f)
{
    int n = 1;
    while (n < kWorkgroupMaxOrder) {
        if (order_begin[n + 1] == order_begin[n]) {  // no member of this order
            ++n;
            continue;
        }
        const SolveChunks c = solve_chunks(n, nrhs);
        int end = n + 1;  // the run takes the orders n ... end - 1
        while (end < kWorkgroupMaxOrder && (order_begin[end + 1] == order_begin[end] || solve_chunks(end, nrhs) == c)) ++end;
        // (orders without members at the run's end belong to no launch: the range below does not see them)
        if (!walk_chunks(c, nrhs, order_begin[n], order_begin[end] - order_begin[n], f)) return;
        n = end;
    }
}

// an order 128 has no spare column
bool vsolve_has_columns(const int *order_begin)
{
    return order_begin[kWorkgroupMaxOrder + 1] == order_begin[kWorkgroupMaxOrder];
}

// ---- Z = X R for a variable-size batch -----------------------------------------------------------------------------------
// One launch per lane class that has members; the columns are walked inside the kernel.  mi32_vbatch_apply_launches
// reports this list and mi32_apply_device_vbatched* walks it.
void mi32::apply_walk(const int *class_begin, size_t elem_bytes, const ApplyLaunchFn &f)
{
    static_assert(kVbatchClasses == 8 && kApplyClasses == 5, "the plan's classes 4 ... 7 share the 128-thread kernel");
    for (int k = 0; k < kApplyClasses; ++k) {
        const int first = class_begin[k], end = class_begin[k + 1 < kApplyClasses ? k + 1 : kVbatchClasses];
        if (end == first) continue;  // a class without members is not launched
        if (!f(ApplyLaunch{first, end - first, kApplyLanes[k], apply_chunk_cols(elem_bytes)})) return;
    }
}

extern "C" {

size_t mi32_workspace_bytes(int n, int batch, int algo)
{
    if (n <= 0 || batch <= 0) return 0;
    Settings s;
    s.algo = algo;
    return dense_route(nullptr, s, n, batch, sizeof(float)).ws_bytes;
}

int mi32_resolve_algo(mi32_handle_t h, int n, int /*batch*/) { return resolve_algo(settings_of(h), n, sizeof(float)); }

int mi32_resolve_blocking(mi32_handle_t h, int n, int batch, int *panel_width, int *block_width)
{
    if (n <= 0 || batch <= 0) return MI32_BAD_SHAPE;
    const BlockedRoute p = route_of(h, settings_of(h), n, batch);
    if (panel_width) *panel_width = p.w;
    if (block_width) *block_width = p.bw;
    return MI32_OK;
}

int mi32_resolve_panel_widths(mi32_handle_t h, int n, int batch, int *widths, int capacity, int *nblocks)
{
    if (n <= 0 || batch <= 0 || capacity < 0 || (capacity > 0 && !widths)) return MI32_BAD_SHAPE;
    // (the widths of the pivoting plan whatever the handle's pivoting: the no-pivot variant runs 16 in every block)
    Settings s = settings_of(h);
    s.pivoting = true;
    const BlockedRoute p = route_of(h, s, n, batch);
    if (nblocks) *nblocks = p.nblk;
    for (int b = 0; b < p.nblk && b < capacity && b < 128; ++b) widths[b] = p.wblk[b];
    return MI32_OK;
}

int mi32_resolve_route(mi32_handle_t h, int n, int batch, mi32_route_t *route, int *panel_groups, int capacity)
{
    if (n <= 0 || batch <= 0 || !blocked_supported(n) || !route || capacity < 0 || (capacity > 0 && !panel_groups))
        return MI32_BAD_SHAPE;
    const BlockedRoute r = route_of(h, settings_of(h), n, batch);
    *route = mi32_route_t{r.np, r.bw, r.nblk, r.shared_panels, r.lookahead, r.parts,
                          {r.part_batch[0], r.part_batch[1]},
                          {r.part_strips_at_end[0], r.part_strips_at_end[1]}, r.first_fused};
    for (int b = 0; panel_groups && b < r.nblk && b < capacity; ++b) panel_groups[b] = r.panel_groups(r.np - b * r.bw);
    return MI32_OK;
}

// tests only: the gj_subpanel_kernel instance that runs panel s of outer block blk of this shape, as blocked_invert
// itself derives it (panel_instance): out[0 .. 5] = threads, rows per lane, columns, fused, workgroups per panel,
// triangular steps.
int mi32_debug_panel_instance(mi32_handle_t h, int n, int batch, int blk, int s, int *out)
{
    if (n <= 0 || batch <= 0 || !blocked_supported(n) || !out) return MI32_BAD_SHAPE;
    Settings st = settings_of(h);
    st.pivoting = true;
    const BlockedRoute r = route_of(h, st, n, batch);
    if (blk < 0 || blk >= r.nblk || s < 0 || (blk * r.bw + (s + 1) * r.wblk[blk]) > r.np) return MI32_BAD_SHAPE;
    const PanelInstance pi = panel_instance(r, blk, s);
    out[0] = pi.nt; out[1] = pi.rpt; out[2] = pi.w; out[3] = pi.fused; out[4] = pi.groups; out[5] = pi.tri;
    return MI32_OK;
}

int mi32_resolve_blocking_f64(mi32_handle_t h, int n, int *block_width)
{
    if (n <= 0 || !block_width) return MI32_BAD_SHAPE;
    const DenseRoute d = dense_route(h, settings_of(h), n, 1, sizeof(double));  // (no fp64 decision reads the batch)
    *block_width = d.path == DenseRoute::BLOCKED64 ? d.blocked64.bw : d.path == DenseRoute::NOPIVOT64 ? d.nopivot64.bw : 0;
    return MI32_OK;
}

// tests only: the DenseRoute of this shape on this context (null: a fresh one's), out[0 .. 4] = path (the order of
// DenseRoute::Path), pivot-list entries, first real step, padded order and block width of the path's plan (0, 0 where it
// has none or, on the sweep, pads nothing); *ws_bytes (may be null): the workspace of the call.
int mi32_debug_dense_route(mi32_handle_t h, int n, int batch, int elem_bytes, int *out, size_t *ws_bytes)
{
    if (n <= 0 || batch <= 0 || (elem_bytes != 4 && elem_bytes != 8) || !out) return MI32_BAD_SHAPE;
    const DenseRoute d = dense_route(h, settings_of(h), n, batch, (size_t)elem_bytes);
    out[0] = d.path; out[1] = d.det_steps; out[2] = d.det_first;
    out[3] = d.path == DenseRoute::BLOCKED32 ? d.blocked.np : d.path == DenseRoute::BLOCKED64 ? d.blocked64.np
             : d.path == DenseRoute::NOPIVOT64 ? d.nopivot64.np : 0;
    out[4] = d.path == DenseRoute::BLOCKED32 ? d.blocked.bw : d.path == DenseRoute::BLOCKED64 ? d.blocked64.bw
             : d.path == DenseRoute::NOPIVOT64 ? d.nopivot64.bw : 0;
    if (ws_bytes) *ws_bytes = d.ws_bytes;
    return MI32_OK;
}

// tests only: the guard size G of the workspace's diagnostic guard mode, rounded up to a multiple of 256; 0 switches
// the mode off.  Process-wide: every size query and every carve from now on reads it.
int mi32_debug_ws_guard(size_t bytes)
{
    g_ws_guard.store(align256(bytes));
    return MI32_OK;
}

// tests only: the regions of the carves the dense calls of this shape make on this context (null: a fresh one's), in
// carve order: the inversion's (owner 0; both parts of a split batch; none on the one-launch routes), the det memory's
// of mi32_inv_det_any_device* (owner 1; none on the one-launch routes) and, for fp32, the residual verifier's (owner 2).
// offset: bytes from the start of the buffer, which is the det memory for owner 1 and the workspace otherwise.  Up to
// `capacity` entries are written; *count is the number there are.
int mi32_debug_ws_layout(mi32_handle_t h, int n, int batch, int elem_bytes, mi32_debug_ws_region *regions, int capacity,
                         int *count)
{
    if (n <= 0 || batch <= 0 || (elem_bytes != 4 && elem_bytes != 8) || !count || capacity < 0 || (capacity > 0 && !regions))
        return MI32_BAD_SHAPE;
    const DenseRoute d = dense_route(h, settings_of(h), n, batch, (size_t)elem_bytes);
    std::vector<WsCarve> carves = dense_carves(d, batch, (size_t)elem_bytes, true);
    if (elem_bytes == 4) carves.push_back(residual_carve_of(n, batch));
    int total = 0;
    for (const WsCarve &c : carves)
        for (const WsRegion &r : c.regions) {
            if (total < capacity) {
                mi32_debug_ws_region &o = regions[total];
                o = mi32_debug_ws_region{c.owner, c.part, r.kind, 0, c.base + r.off, r.bytes, {}};
                std::strncpy(o.name, r.name, sizeof(o.name) - 1);
            }
            ++total;
        }
    *count = total;
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

int mi32_resolve_wide(mi32_handle_t /*h*/, int n, int elem_bytes, int *threads_per_matrix, int *rows_per_thread, int *max_order)
{
    if (n <= 0 || (elem_bytes != 4 && elem_bytes != 8)) return MI32_BAD_SHAPE;
    const bool f32 = elem_bytes == 4;  // no fp64 instance: the register file holds no 256 x 256 fp64 matrix
    if (threads_per_matrix) *threads_per_matrix = f32 ? wide_threads(n) : 0;
    if (rows_per_thread) *rows_per_thread = f32 ? wide_rows_per_thread(n) : 0;
    if (max_order) *max_order = kWideMaxOrder;
    return MI32_OK;
}

int mi32_resolve_solve(mi32_handle_t /*h*/, int n, int nrhs, int elem_bytes, int *chunk_cols, int *launches, int *lanes,
                       int *rows_per_thread)
{
    const int cap = solve_chunk_cols(n);
    if (cap == 0 || nrhs <= 0 || (elem_bytes != 4 && elem_bytes != 8) || !chunk_cols || !launches || !lanes ||
        !rows_per_thread)
        return MI32_BAD_SHAPE;
    const SolveChunks c = solve_chunks(n, nrhs);
    *chunk_cols = cap;
    *launches = (int)c.chunks;
    *lanes = c.first.lanes;  // the first chunk's kernel
    *rows_per_thread = c.first.rows_per_thread;
    return MI32_OK;
}

const char *mi32_dominant_kernel(int algo)
{
    return algo == MI32_ALGO_WIDE ? "gj_wide_kernel"
           : algo == MI32_ALGO_WORKGROUP ? "gj_workgroup_kernel"
           : algo == MI32_ALGO_RESIDENT ? "gj_resident_kernel"
           : algo == MI32_ALGO_SWEEP  ? "gj_sweep_step_kernel"
                                      : "gj_rank_bw2_kernel";
}

int mi32_vbatch_bin(const int *orders, int batch, int *perm, int *class_begin)
{
    if (!perm || !class_begin) return MI32_BAD_SHAPE;
    return vbatch_sort(orders, batch, perm, class_begin, nullptr);
}

int mi32_vbatch_solve_launches(const int *orders, int batch, int nrhs, int *launches, int capacity, int *count)
{
    if (!orders || !count || batch <= 0 || nrhs <= 0 || capacity < 0 || (capacity > 0 && !launches)) return MI32_BAD_SHAPE;
    int order_begin[kWorkgroupMaxOrder + 2];
    if (vbatch_sort(orders, batch, nullptr, nullptr, order_begin) != MI32_OK) return MI32_BAD_SHAPE;
    if (!vsolve_has_columns(order_begin)) return MI32_BAD_SHAPE;
    long long total = 0;
    vsolve_walk(order_begin, nrhs, [&](const SolveLaunch &s) {
        if (total < capacity) {
            int *l = launches + 6 * total;
            l[0] = s.first, l[1] = s.count, l[2] = s.col0, l[3] = s.cols, l[4] = s.kernel.lanes, l[5] = s.kernel.rows_per_thread;
        }
        ++total;
        return true;
    });
    if (total > 0x7fffffffLL) return MI32_BAD_SHAPE;
    *count = (int)total;
    return MI32_OK;
}

int mi32_vbatch_apply_launches(const int *orders, int batch, int nrhs, int elem_bytes, int *launches, int capacity,
                               int *count)
{
    if (!orders || !count || batch <= 0 || nrhs <= 0 || (elem_bytes != 4 && elem_bytes != 8) || capacity < 0 ||
        (capacity > 0 && !launches))
        return MI32_BAD_SHAPE;
    int class_begin[kVbatchClasses + 1];
    if (vbatch_sort(orders, batch, nullptr, class_begin, nullptr) != MI32_OK) return MI32_BAD_SHAPE;
    int total = 0;
    apply_walk(class_begin, (size_t)elem_bytes, [&](const ApplyLaunch &a) {
        if (total < capacity) {
            int *l = launches + 4 * total;
            l[0] = a.first, l[1] = a.count, l[2] = a.lanes, l[3] = a.cols;
        }
        ++total;
        return true;
    });
    *count = total;
    return MI32_OK;
}

// GPU g of G owns the matrices [g * ceil(B / G), min(B, (g + 1) * ceil(B / G))) (possibly none)
int mi32_shard_range(int batch, int ngpus, int g, int *lo, int *hi)
{
    if (batch < 0 || ngpus <= 0 || g < 0 || g >= ngpus || !lo || !hi) return MI32_BAD_SHAPE;
    const int per = (batch + ngpus - 1) / ngpus;
    const long long l = (long long)g * per;
    *lo = l < batch ? (int)l : batch;
    *hi = (l + per < batch) ? (int)(l + per) : batch;
    return MI32_OK;
}

}  // extern "C"
