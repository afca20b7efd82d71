// mi32_internal.h -- shared declarations of libmat_inv_32.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <type_traits>
#include <vector>

#include "mat_inv_32_c.h"

namespace mi32 {

// ---- pivot records ----------------------------------------------------------
// One 64-bit key per candidate: (bits of |a| << 32) | ~row.  |a| >= 0, so its
// IEEE bit pattern orders like the value; the inverted row index makes an
// unsigned max pick the LOWEST row among equal maxima (the reference's scan
// keeps the first maximum, mat_inv_32.cpp:121-127).  NaN candidates and "no
// candidate" are key 0, which loses against every real candidate.
__device__ __forceinline__ unsigned long long pivot_key(float a, int row)
{
    const float v = __builtin_fabsf(a);
    if (!(v == v)) return 0ull;
    return ((unsigned long long)__float_as_uint(v) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)row);
}
__device__ __forceinline__ int pivot_key_row(unsigned long long key, int fallback_row)
{
    return key == 0ull ? fallback_row : (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
}
// the pivot that flags its matrix MI32_SINGULAR on every path: zero, NaN or infinite
template <typename T>
__device__ __forceinline__ bool pivot_unusable(T piv) { return piv == T(0) || piv - piv != T(0); }

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long k)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(k, off, 64);
        k = o > k ? o : k;
    }
    return k;
}

// Blocked fp32 plans with shared panels only: true when matrix b was given up (see SubpanelArgs::guard in
// mi32_blocked_internal.h; guard may be null).  Wave-uniform.
__device__ __forceinline__ bool matrix_given_up(const int *guard, int b)
{
    return guard != nullptr && __builtin_amdgcn_readfirstlane(guard[b]) == MI32_RUNTIME_ERROR;
}

// ---- optional per-kernel-class timing (HIP events on the launch stream) -------------
// Off by default.  When a context enables it, every launch is bracketed by two
// events recorded on the stream the kernel is launched on; the classes mirror the
// reference's per-phase timing slots (FP32_bench.cpp:256-443: makeAug, pivot, row,
// column, getInverted).
enum KernelClass {
    KC_INIT = 0,       // makeAugmented counterpart
    KC_SWEEP_STEP = 1, // fused pivot step of the sweep path
    KC_PANEL = 2,      // register-resident panel steps of the blocked path
    KC_UPDATE_IN = 3,  // rank-w update inside a block
    KC_UPDATE_OUT = 4, // rank-bw update of the rest of the matrix (fp32 MFMA)
    KC_FINISH = 5,     // getInverted counterpart (column un-permutation)
    KC_TRANSPOSE = 6,  // multiplier transposition in front of a rank-bw update (A operand, k-major)
    KC_COUNT = 7
};
struct Profiler {
    virtual void begin(int kclass, hipStream_t s) = 0;
    virtual void end(int kclass, hipStream_t s) = 0;
    virtual ~Profiler() {}
};
struct ProfScope {
    Profiler *p; int k; hipStream_t s;
    ProfScope(Profiler *p_, int k_, hipStream_t s_) : p(p_), k(k_), s(s_) { if (p) p->begin(k, s); }
    ~ProfScope() { if (p) p->end(k, s); }
};

// ---- workspace carving ----------------------------------------------------------
// Every workspace region starts on a 256-byte boundary.
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
// What a region holds.  The diagnostic guard mode ("Ordering and workspace contract") poisons the VALUES
// regions and leaves the other two as they are: a poisoned index would turn a stale-map read into a wild address.
enum WsKind {
    WS_VALUES = 0,   // float or double working data
    WS_INDICES = 1,  // row maps (int)
    WS_RECORDS = 2   // arg-max records, exchange granules, flags, parity
};
struct WsRegion {
    const char *name;  // a string literal
    size_t off, bytes;
    int kind;
};
typedef std::vector<WsRegion> WsRegions;
// The guard size G in bytes, a multiple of 256; 0: the mode is off (always, unless a test called mi32_debug_ws_guard).
// Process-wide, and read by WsCarver alone: the size-only pass and the address pass of a carve cannot disagree.
extern std::atomic<size_t> g_ws_guard;  // mi32_plan.hip
// Bump allocator over one workspace.  Without a base pointer it only adds up the region sizes (the
// *_workspace_bytes functions); with one it also hands out each region's address.  With a guard size G, one red zone
// of G bytes lies in front of the first region and one behind every region.  `log` (may be null) takes the regions in
// carve order.
struct WsCarver {
    char *base;
    size_t guard;
    size_t off;
    WsRegions *log;
    explicit WsCarver(void *b, WsRegions *l = nullptr)
        : base((char *)b), guard(g_ws_guard.load(std::memory_order_relaxed)), off(guard), log(l) {}
    template <typename P>
    P *take(size_t bytes, WsKind kind, const char *name)
    {
        P *p = base ? (P *)(base + off) : nullptr;
        if (log) log->push_back(WsRegion{name, off, bytes, (int)kind});
        off += bytes + guard;
        return p;
    }
};

// ---- launch plumbing ----------------------------------------------------------
struct SweepPlan {
    int n;        // matrix order
    int ld;       // leading dimension of the working copies (n rounded up to 4)
    int tr;       // rows per workgroup of the step kernel
    int row_tiles;
    int col_tiles;
};

// ---- the blocked fp32 path's route -------------------------------------------------------------------------------------
static constexpr int kMaxBW = 512;  // widest outer block (rows of the transposed panel Gk)
static constexpr int kMaxW = 32;    // widest sub-panel (columns kept in registers)
// A panel of more than kPanelGroupRows candidate rows is shared by up to kMaxPanelGroups workgroups (one CU
// each, <= 4 rows per lane at 1024 threads) that exchange every step's local winner through global memory.
static constexpr int kMaxPanelGroups = 4;
static constexpr int kPanelGroupRows = 4096;
// Fused launches exist for the panel geometries of at most kFusedRows rows (see "Fused mode" in blocked_invert).
static constexpr int kFusedRows = 2048;

// How one blocked fp32 call runs.  Every decision of the path is taken once, by plan_route (mi32_plan.hip), from the
// settings, the shape and the streams the context offers; blocked_invert and the launchers read it and decide nothing.
struct BlockedRoute {
    // ---- geometry
    int n;     // matrix order
    int np;    // padded order (multiple of 128), identity padding
    int ld;    // row stride of the working copies in floats (np + 64)
    int w;     // widest sub-panel allowed (what the caller asked for; 16 by default)
    int bw;    // outer block width
    int nblk;
    int nthreads_panel;
    int rpt;   // rows per thread in the panel kernel when it holds all np rows
    bool pivoting;  // false: the reference's no-pivot variant (the diagonal entry is every step's pivot)
    // ---- per outer block
    // Sub-panel width.  The panel kernel keeps (rows at or below the block) x width floats in registers, so the first
    // blocks of a large matrix use narrow sub-panels and the width grows as the elimination retires rows (16384 rows:
    // 4, 8192: 8, 4096 and fewer: 16).  Without pivoting there is no register-resident panel: 16 in every block.
    unsigned char wblk[128];
    // Blocks from this one on run panel(s) || update(s-1) as one launch (nblk: none does; pivoting only).
    int first_fused;
    bool fused(int blk) const { return blk >= first_fused; }
    // More than kPanelGroupRows candidate rows: the panel is shared by up to kMaxPanelGroups workgroups instead of
    // narrowing the sub-panels (pivoting and small batches only: all of a panel's workgroups must be resident at the
    // same time).  Every launch then skips a matrix whose panel lost a partner.
    bool shared_panels;
    // workgroups of a panel that holds `rows` rows (it changes inside a block: 8320 rows, 3 -> 2 at 8192)
    int panel_groups(int rows) const { return shared_panels ? (rows + kPanelGroupRows - 1) / kPanelGroupRows : 1; }
    // the rank-bw update of a block is cut in two and all but the next block's columns run on the second stream
    bool lookahead;
    // ---- parts: the whole batch on the main stream, or ceil(batch / 2) there and the rest on the split stream.  Both
    // halves run with the blocking and the panels of the whole batch; a half never has the look-ahead.
    int parts;
    int part_batch[2];
    // true: the block's strips in one launch at its end; false: they ride in the panel launches (decided per part)
    bool part_strips_at_end[2];
};

// Thread geometry of a panel launch that holds `nrows` rows: NT threads hold the rows x w columns in registers, rpt
// rows each (1024 threads leave <= 128 VGPRs per lane, i.e. rpt * w <= 64 floats of slab) -- the smallest that fits
// (fewer waves and fewer rows per lane both shorten a pivot step).
inline void panel_geometry(const BlockedRoute &r, int nrows, int &nt, int &rpt)
{
    rpt = 1;
    if (r.panel_groups(nrows) > 1) {  // shared by ceil(nrows / 4096) workgroups of 1024 x 4 rows
        nt = 1024;
        rpt = 4;
        return;
    }
    if (nrows <= 256) nt = 256;
    else if (nrows <= 512) nt = 512;
    else {
        nt = r.nthreads_panel;
        while (rpt * nt < nrows) rpt *= 2;
        // 2049 ... 3072 rows at 1024 threads: three rows per lane (a fourth, dead row costs every pivot step its issue)
        if (nt == 1024 && rpt == 4 && 3 * nt >= nrows) rpt = 3;
    }
}

// Which panel instance runs TRIANGULAR pivot steps (mi32_panel.h, panel_step): step R updates the columns c > R only and
// the panel writes no G_s -- the column-tile-0 update tiles compute it from the multipliers and the normalised pivot
// rows (SubpanelArgs::u_tri), and one wave of the panel completes the pivot rows left of their pivots after the last
// step (tri_left_rows: ~3 us).  That pays where the panel's own FMAs and its G_s store cost more, and it is on for the
// one instance it was measured on: the unfused one-workgroup panel of 1024 threads x 4 rows per lane x 16 columns
// (3073 ... 4096 rows; 31.5 -> 28.0 us per launch).  At one to three rows per lane the same change cost 0.2 ... 3 us per
// launch; the other geometries with four and more rows per lane have not been timed.
// Never the multi-workgroup panels: their exchange granules carry no multiplier history.
constexpr bool panel_tri(int nt, int rpt, int w, bool multi, bool fused)
{
    return !multi && !fused && nt == 1024 && rpt == 4 && w == 16;
}

// The kernel instance that runs panel(s) of outer block blk with pivoting: what blocked_invert and dispatch_subpanel
// make of the route (thread geometry by the rows the panel holds; fused when an update rides in its launch, which the
// first panel of a fused block has none of).
struct PanelInstance {
    int nt, rpt, w, groups;
    bool fused, tri;
};
inline PanelInstance panel_instance(const BlockedRoute &r, int blk, int s)
{
    PanelInstance pi;
    pi.w = r.wblk[blk];
    pi.fused = r.fused(blk) && s > 0;
    const int c0 = blk * r.bw + s * pi.w;
    const int rows = r.np - (pi.fused ? c0 - pi.w : c0);  // a fused panel holds the pivot rows of s-1 once more
    pi.groups = r.panel_groups(rows);
    panel_geometry(r, rows, pi.nt, pi.rpt);
    pi.tri = panel_tri(pi.nt, pi.rpt, pi.w, pi.groups > 1, pi.fused);
    return pi;
}

// Above kWorkgroupMaxOrder (mi32_inv_det_any_device*, mi32_det_large.h) the pivots are spread over launches: what a det
// call hands to a sweep / blocked route, which records every step's pivot there.  Empty: a plain call, which enqueues
// exactly the launches it always did.
struct DetRec {
    void *piv = nullptr;    // element type of the route; matrix b's pivot of (padded) step r at piv[b * pstride + r]
    size_t pstride = 0;     // elements per matrix, >= the route's padded order
    int *parity = nullptr;  // int[batch], zeroed on the stream before the route runs; bit 0: an odd number of exchanges
    bool on() const { return piv != nullptr; }
};

SweepPlan make_sweep_plan(int n);

// The size-only pass of each path's carve; regions (may be null) takes the carve's regions in order.
size_t sweep_workspace_bytes(const SweepPlan &p, int batch, size_t elem_bytes, WsRegions *regions = nullptr);
// of `batch` members (a whole call, or one part)
size_t blocked_workspace_bytes(const BlockedRoute &r, int batch, WsRegions *regions = nullptr);

// Enqueue a whole inversion on `stream`.  ws: workspace of at least the size
// reported above, 256-byte aligned.
// T = float, or double: the fp64 twin (matrix_inversion_FP64 of the reference), same launches on doubles.
// pivoting = false: the reference's no-pivot variant (matrix_inversion_no_pivots.cpp:10), the diagonal entry is the pivot
template <typename T>
hipError_t sweep_invert(const SweepPlan &p, const T *d_a, T *d_inv, int batch, int *d_status, void *ws,
                        hipStream_t stream, Profiler *prof, bool pivoting = true, const DetRec &det = DetRec());
// fp64 blocked path (mi32_blocked64.hip): windowed sweep steps + rank-bw updates on the fp64 matrix cores
struct Blocked64Plan {
    int n, np, ld;  // matrix order, padded order (multiple of 64, identity padding), row stride in doubles
    int bw;         // outer block width (multiple of 64, <= 256)
    int tr;         // rows per workgroup of the step kernel (8 or 32)
    int row_tiles;  // workgroups per step launch = arg-max records per column
};
Blocked64Plan make_blocked64_plan(int n, int bw);
size_t blocked64_workspace_bytes(const Blocked64Plan &p, int batch, WsRegions *regions = nullptr);
hipError_t blocked64_invert(const Blocked64Plan &p, const double *d_a, double *d_inv, int batch, int *d_status, void *ws,
                            hipStream_t stream, Profiler *prof, const DetRec &det = DetRec());
// makeAugmented counterpart of the fp64 blocked paths: w0 <- diag(A, I) with pad = 0 (the pivoted path) or diag(I, A)
// with pad = np - n (the no-pivot path: rows and columns [pad, np) hold the matrix); np x np, row stride ld, wstride
// doubles per matrix; orig <- the identity, status[b] <- MI32_SINGULAR for a non-finite input entry (status may be null)
void launch_b64_init(const double *d_a, int n, int np, int ld, size_t wstride, double *w0, int *orig, int batch,
                     int *status, hipStream_t stream, int pad);
// fp64 no-pivot path (mi32_nopivot64.hip): the reference's order element by element, per block of bw steps the
// diagonal block on one workgroup, the block columns / pivot-row strips of every other row / column, and one
// rank-bw update on the fp64 matrix cores
struct NoPivot64Plan {
    int n, np, ld;  // matrix order, padded order (multiple of bw, identity padding), row stride in doubles
    int bw;         // block width: 64 (default) or 128
};
NoPivot64Plan make_nopivot64_plan(int n, int bw);
size_t nopivot64_workspace_bytes(const NoPivot64Plan &p, int batch, WsRegions *regions = nullptr);
hipError_t nopivot64_invert(const NoPivot64Plan &p, const double *d_a, double *d_inv, int batch, int *d_status, void *ws,
                            hipStream_t stream, Profiler *prof, const DetRec &det = DetRec());

// register-resident path (mi32_resident.hip): orders up to kResidentMaxOrder, one launch, no workspace.  A group of
// resident_lanes(n) lanes (8 / 16 / 32 / 64; 0 when the order is out of range) holds one matrix; d_status must not
// be null.  Bit-identical to the sweep path.
static constexpr int kResidentMaxOrder = 64;
int resident_lanes(int n);

// workgroup-resident path (mi32_workgroup.hip): orders kResidentMaxOrder + 1 ... kWorkgroupMaxOrder, one launch, no
// workspace.  One workgroup of 256 threads holds one matrix in registers, workgroup_rows_per_thread(n) rows per thread
// (40 / 48 / 56 / 64; 0 when the order is out of range); d_status must not be null.  Bit-identical to the sweep path.
static constexpr int kWorkgroupMaxOrder = 128;
int workgroup_rows_per_thread(int n);

// wide workgroup-resident path (mi32_wide.hip): fp32 orders kWorkgroupMaxOrder + 1 ... kWideMaxOrder, one launch, no
// workspace.  One workgroup of wide_threads(n) threads (768 / 1024: 4 slabs of 192 / 256 column lanes) holds one matrix
// in registers, wide_rows_per_thread(n) rows per thread (40 / 48 / 56 / 64; both 0 when the order is out of range);
// d_status must not be null.  Bit-identical to the sweep path.
static constexpr int kWideMaxOrder = 256;
int wide_rows_per_thread(int n);
int wide_threads(int n);

// f(value, pivot), both as compile-time constants (std::integral_constant): the one place where a run-time pair picks
// a kernel instance of the one-launch batch paths.  false: `value` is none of Vs, and f was not called.
template <int... Vs, typename F>
static bool pick_instance(int value, bool pivoting, F f)
{
    const auto pick = [&](auto c) {
        if (value != decltype(c)::value) return false;
        if (pivoting) f(c, std::true_type{});
        else f(c, std::false_type{});
        return true;
    };
    return (pick(std::integral_constant<int, Vs>{}) || ...);
}
// the instances of slab_member (mi32_slab.h) on both paths above, by their rows per thread
template <typename F>
static bool slab_instance(int rows_per_thread, bool pivoting, F f)
{
    return pick_instance<40, 48, 56, 64>(rows_per_thread, pivoting, f);
}

// variable-size batches (mi32_vbatch_*): members of any orders 1 ... kWorkgroupMaxOrder, each at its own pointer and
// leading dimensions, on the two paths above.  Everything here is device memory.  `members` is the plan's list of
// member indices sorted by order; a launch takes the `count` members from `first` on, which all belong to one kernel
// instance (lanes per matrix / rows per thread), and looks everything else up by the member index.
template <typename T>
struct VbatchArgs {
    const int *orders;   // int[batch], in the caller's member order
    const int *members;  // int[batch], the member indices in ascending order of their orders (stable)
    const T *const *a;   // member pointers, row-major, rows lda[b] elements apart
    T *const *inv;
    const int *lda;      // null: orders[b]
    const int *ldinv;    // null: orders[b]
    int *status;         // int[batch], zeroed by the host before the launches
};

// ---- the determinant beside the inverse (mi32_inv_det_device*) ------------------------------------------------------
// The pivot steps of the two paths above already hold every pivot value and every row exchange, and elimination with
// partial pivoting gives det A = (-1)^swaps * prod pivots.  The det kernels (gj_*_det_kernel / gj_*_det_vkernel) are the
// same bodies with a compile-time switch; the elimination arithmetic is untouched.  The determinant is a pair like
// frexp's, det = m * 2^e with |m| in [0.5, 1), built by a fixed recurrence of IEEE double operations.  It starts at
// (1.0, 0); after step r has its pivot `piv` and knows whether row r and the pivot row differ (`swap`), while the member
// is not flagged:
//     (pm, pe) = frexp((double)piv);  if (swap) m = -m;  (m, k) = frexp(m * pm);  e += pe + k;
// The step that flags the member ends the accumulation: (+0.0, 0) for an exactly zero pivot with pivoting on (the rest
// of the column is exactly zero), (NaN, 0) for every other flag and for a non-finite input entry.
struct DetAcc {
    double m;
    int e;
    bool flagged;  // the member is flagged (by its input or an earlier step): the pair is final
};
// before the first step; input_bad: some entry of the member's input is not finite (the whole member's, not this lane's)
__device__ __forceinline__ DetAcc det_start(const bool input_bad)
{
    return DetAcc{input_bad ? __builtin_nan("") : 1.0, 0, input_bad};
}
// The recurrence.  UNIFORM: every lane of the wave holds the same
// member, so the accumulator is moved to scalar registers between steps -- it costs no vector register where the
// elimination needs them all (fp64, 64 lanes, pivoting: 256).
template <typename T, bool PIVOT, bool UNIFORM>
__device__ __forceinline__ void det_accumulate(DetAcc &d, const T piv, const bool swap)
{
    const bool piv_bad = piv == T(0) || piv - piv != T(0);
    const double pd = (double)piv;  // exact
    const double pm = __builtin_amdgcn_frexp_mant(pd);
    const int pe = __builtin_amdgcn_frexp_exp(pd);
    const double prod = (swap ? -d.m : d.m) * pm;  // in +-[0.25, 1): never under- or overflows
    const double ok_m = __builtin_amdgcn_frexp_mant(prod);
    const int ok_e = d.e + pe + __builtin_amdgcn_frexp_exp(prod);
    const double bad_m = (PIVOT && piv == T(0)) ? 0.0 : __builtin_nan("");
    double m = d.flagged ? d.m : piv_bad ? bad_m : ok_m;
    int e = d.flagged ? d.e : piv_bad ? 0 : ok_e;
    if constexpr (UNIFORM) {
        m = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(m)),
                             __builtin_amdgcn_readfirstlane(__double2loint(m)));
        e = __builtin_amdgcn_readfirstlane(e);
    }
    d.m = m;
    d.e = e;
    d.flagged = d.flagged || piv_bad;
}
// where the determinants go: member b's pair to mant[b], exp[b].  Empty (both null): no determinant, the plain kernels
// run; with one the det kernels run and the inverse's pointer(s) may be null (determinant only).
struct DetOut {
    double *mant;
    int *exp;
    bool empty() const { return !mant && !exp; }
    bool valid() const { return !mant == !exp; }  // exactly one null member is no DetOut
};
// the det kernels' argument: VbatchArgs plus the determinant arrays (double[batch], int[batch], the caller's member
// order); v.inv may be null: only status and determinant are written then
template <typename T>
struct VbatchDetArgs {
    VbatchArgs<T> v;
    double *det_mant;
    int *det_exp;
};

// ---- the launchers of the two one-launch paths -----------------------------------------------------------------------
// Per path a uniform batch and a slice of a variable-size plan (lanes / rows_per_thread: the slice's kernel class).  The
// status words are zeroed by the host before the launch; hipErrorInvalidValue for an order or class without an instance,
// a DetOut with exactly one null member, or a null inverse without a DetOut.
template <typename T>
hipError_t resident_invert(const T *d_a, T *d_inv, int n, int batch, int *d_status, DetOut det, hipStream_t stream,
                           Profiler *prof, bool pivoting);
template <typename T>
hipError_t resident_vinvert(int lanes, const VbatchArgs<T> &v, DetOut det, int first, int count, hipStream_t stream,
                            Profiler *prof, bool pivoting);
template <typename T>
hipError_t workgroup_invert(const T *d_a, T *d_inv, int n, int batch, int *d_status, DetOut det, hipStream_t stream,
                            Profiler *prof, bool pivoting);
template <typename T>
hipError_t workgroup_vinvert(int rows_per_thread, const VbatchArgs<T> &v, DetOut det, int first, int count,
                             hipStream_t stream, Profiler *prof, bool pivoting);
// the wide path: a uniform fp32 batch only
hipError_t wide_invert(const float *d_a, float *d_inv, int n, int batch, int *d_status, DetOut det, hipStream_t stream,
                       Profiler *prof, bool pivoting);

// ---- A X = B on the two paths above, without the inverse (mi32_solve_device*) ----------------------------------------
// A lane (register-resident) or column (workgroup-resident) j >= n of a member holds zeros, is read by no step and never
// stores: the solve kernels (gj_resident_solve_kernel / gj_workgroup_solve_kernel) put a column of B there, and the
// unchanged pivot step performs Gauss-Jordan on the augmented column -- the row exchange, prn = b[p] / piv, b[i] =
// fma(-f, prn, b[i]) unless f == 0, b[r] = prn.  One launch takes the `cols` columns of B from `col0` on; n + cols is
// the launch's WIDTH: at most kResidentMaxOrder for the register-resident kernel (resident_lanes(n + cols) lanes per
// member), at most kWorkgroupMaxOrder for the workgroup-resident one.  The lanes / columns < n store nothing.
template <typename T>
struct SolveArgs {
    const T *a;   // (batch, n, n) contiguous
    const T *b;   // (batch, n, nrhs) contiguous
    T *x;         // (batch, n, nrhs) contiguous; may be b: a member's loads all precede its stores
    int *status;  // int[batch], zeroed by the host before the first launch of the call
    int n, batch, nrhs;
    int col0, cols;  // this launch's columns of B and X
};
// rows per thread of the workgroup-resident solve kernel: 40 up to order 80 (an order <= 64 whose width exceeds 64
// lanes included), then as workgroup_rows_per_thread; 0 outside 1 ... kWorkgroupMaxOrder - 1
int workgroup_solve_rows_per_thread(int n);
// hipErrorInvalidValue for a width without an instance, no columns, or a null pointer
template <typename T>
hipError_t resident_solve(const SolveArgs<T> &s, hipStream_t stream, Profiler *prof, bool pivoting);
template <typename T>
hipError_t workgroup_solve(const SolveArgs<T> &s, hipStream_t stream, Profiler *prof, bool pivoting);

// ---- A X = B for a variable-size batch (mi32_solve_device_vbatched*) -------------------------------------------------
// The solve kernels' variable-size twins (gj_resident_solve_vkernel / gj_workgroup_solve_vkernel; each pair shares its
// member body, resident_solve_member of mi32_resident.hip and slab_member of mi32_slab.h): a launch takes the
// `count` members from `first` on of the plan's sorted list, which all run the columns col0 ... col0 + cols - 1 of their
// B on one kernel instance (lanes per member by the width n + cols, or rows per thread by the order), and looks up the
// member's order, pointers and leading dimensions by the member index.  Everything here is device memory.
template <typename T>
struct VsolveArgs {
    const int *orders;   // int[batch], in the caller's member order
    const int *members;  // int[batch], the member indices in ascending order of their orders (stable)
    const T *const *a;   // member pointers, row-major: A is n x n, rows lda[b] elements apart
    const T *const *b;   // B is n x nrhs, rows ldb[b] elements apart
    T *const *x;         // X is n x nrhs, rows ldx[b] elements apart; x[b] may be b[b] with ldx[b] == ldb[b]
    const int *lda;      // null: orders[b]
    const int *ldb;      // null: nrhs
    const int *ldx;      // null: nrhs
    int *status;         // int[batch], zeroed by the host before the first launch of the call
    int nrhs;
    int col0, cols;      // this launch's columns of B and X
};
// hipErrorInvalidValue for a class without an instance, an empty or negative range, no columns, or a null pointer
template <typename T>
hipError_t resident_vsolve(int lanes, const VsolveArgs<T> &v, int first, int count, hipStream_t stream, Profiler *prof,
                           bool pivoting);
template <typename T>
hipError_t workgroup_vsolve(int rows_per_thread, const VsolveArgs<T> &v, int first, int count, hipStream_t stream,
                            Profiler *prof, bool pivoting);

// The resources a blocked inversion is enqueued with (what to do with them is the route's business): `aux` carries the
// look-ahead half of each rank-bw update; events[0 .. n/2) mark "second-stream work done", events[n/2 .. n) "panel
// phase done"
struct BlockedExec {
    hipStream_t stream = nullptr;
    hipStream_t aux = nullptr;
    hipEvent_t *events = nullptr;
    int n_events = 0;
    int aux_workgroups = 0;  // grid of the persistent look-ahead kernel: CUs minus the ones kept free
    bool aux_exclusive = false;  // its workgroups take a whole CU's LDS: nothing of the main stream shares their CUs
    Profiler *prof = nullptr;
};
// enqueues part `part` of the route: its r.part_batch[part] members at d_a / d_inv / d_status, in the workspace ws
// det (a det call only): the pivots of the part's members; d_inv may then be null (determinant only)
hipError_t blocked_invert(const BlockedRoute &r, int part, const float *d_a, float *d_inv, int *d_status, void *ws,
                          const BlockedExec &ex, const DetRec &det = DetRec());
// getInvertedMatrix counterpart (mat_inv_32.cpp:195-203), shared by the three paths (mi32_sweep.hip).  Working
// column c holds inverse column orig[c].  orig and invp hold np entries per matrix, np apart.
// invp <- the inverse of orig; a matrix whose guard word is MI32_RUNTIME_ERROR is skipped (guard may be null).
void launch_invert_perm(const int *orig, int *invp, int np, int batch, const int *guard, hipStream_t stream);
// launch_invert_perm, then out (n x n per matrix) <- the working copy w (row stride ld, wstride elements per matrix)
// with its columns gathered through invp
// (T = float or double)
template <typename T>
void launch_unpermute(const T *w, int ld, size_t wstride, const int *orig, int *invp, int np, int n, int batch, T *out,
                      hipStream_t stream);
hipError_t residual_launch(const float *d_a, const float *d_x, int n, int batch, double *d_out, void *ws,
                           hipStream_t stream);
size_t residual_workspace_bytes(int n, int batch, WsRegions *regions = nullptr);
hipError_t frobenius_launch_f64(const double *d_a, const double *d_b, int n, double *d_out, void *ws, hipStream_t stream);

}  // namespace mi32
