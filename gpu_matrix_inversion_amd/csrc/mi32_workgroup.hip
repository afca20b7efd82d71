// mi32_workgroup.hip -- the workgroup-resident path for large batches of matrices of order 65 ... 128, gfx950.
//
// One launch per call: one workgroup of 256 threads owns one matrix from the load to the un-permuted inverse.  One
// global read and one global write per element, no workspace, the matrix index is blockIdx.x alone (64-bit offsets).
//
// Layout: the matrix lives in the workgroup's REGISTERS.  Thread (slab h, column j) -- j = threadIdx.x & 127,
// h = threadIdx.x >> 7, so a slab is two whole waves -- holds the register slots h * RPT ... h * RPT + RPT - 1 of
// column j; RPT = 40 / 48 / 56 / 64 gives 80 / 96 / 112 / 128 padded rows.  A slot >= n is NaN in every column (a NaN
// never wins a pivot search, and a row only ever changes itself unless it is the pivot row); a column >= n holds
// zeros, is published by no step r < n and never stores.
//
// Labels instead of swaps: slot s holds the logical row label[s] (the identity at the start).  pivotElements exchanges
// two labels and moves no data; the search considers slots with label >= r and breaks ties by the label; the store
// writes slot s to row label[s].  The column permutation of the sweep (working column c holds inverse column orig[c],
// orig[r] <-> orig[p] per step) is the inverse of the label permutation (label[s]: r <-> p by value), so column j
// stores to column slot_of[j], the slot whose label is j, and no second table is carried.
//
// LDS carries only the per-step exchange: the published column r (the multiplier column and the search's input) and the
// normalised pivot row, both double-buffered by the parity of the step, so that a step needs two barriers.  Per step r,
// in the arithmetic of gj_sweep_step_kernel / resident_step (hence the same bits as the CPU oracle):
//   a. the two threads of column r publish their slots and then zero them (the implicit identity column's entries)
//   b. barrier; EVERY wave searches the published column redundantly: lane l builds the PivotRec<T> of slots l and
//      l + 64 from its copy of their labels, one wave reduction; the labels live in two registers per lane of every
//      wave (kept identical by construction) and reach LDS once, for the store
//   c. the slab that holds the pivot slot picks its entry with a wave-uniform switch (scalar branches, no run-time
//      register index), divides ONCE per column, prn = a[p][j] / piv (column r: 1 / piv), and publishes prn
//   d. barrier; every slot takes its multiplier f = published column entry by ds_read_b128 at compile-time offsets (all
//      lanes read one address: a broadcast) and a[i] = fma(-f, prn, a[i]), skipped when f == 0; the pivot slot
//      is then overwritten with prn by a second wave-uniform switch
//   e. a zero / NaN / infinite pivot, or a non-finite input entry, flags the member MI32_SINGULAR
//
// gj_workgroup_vkernel is the same body for a variable-size batch (mi32_inv_device_vbatched): the workgroup looks up
// its member's order, pointers and leading dimensions from blockIdx.x.
#include <type_traits>

#include "mi32_internal.h"
#include "mi32_sweep_common.h"

namespace mi32 {

static constexpr int kWorkgroupThreads = 256;
static constexpr int kWorkgroupColumns = 128;  // column lanes per slab; also the most padded rows (2 x 64)

int workgroup_rows_per_thread(int n)
{
    return n <= kResidentMaxOrder || n > kWorkgroupMaxOrder ? 0 : n <= 80 ? 40 : n <= 96 ? 48 : n <= 112 ? 56 : 64;
}

int workgroup_solve_rows_per_thread(int n)
{
    return n < 1 || n >= kWorkgroupMaxOrder ? 0 : n <= 80 ? 40 : workgroup_rows_per_thread(n);
}

// `X(i)` for i = 0 ... 63 as the cases of a switch; slots >= RPT are discarded at compile time
#define MI32_WG_CASES8(X, b) X(b + 0) X(b + 1) X(b + 2) X(b + 3) X(b + 4) X(b + 5) X(b + 6) X(b + 7)
#define MI32_WG_CASES64(X)                                                                                      \
    MI32_WG_CASES8(X, 0) MI32_WG_CASES8(X, 8) MI32_WG_CASES8(X, 16) MI32_WG_CASES8(X, 24) MI32_WG_CASES8(X, 32) \
    MI32_WG_CASES8(X, 40) MI32_WG_CASES8(X, 48) MI32_WG_CASES8(X, 56)

// a[slot] for a wave-uniform slot held in a scalar register: a tree of scalar branches around one move
template <typename T, int RPT>
__device__ __forceinline__ T wg_pick(const T (&a)[RPT], int slot)
{
    T v = T(0);
#define MI32_WG_PICK(i) \
    case (i):           \
        if constexpr ((i) < RPT) v = a[(i)]; \
        break;
    switch (slot) { MI32_WG_CASES64(MI32_WG_PICK) default: break; }
#undef MI32_WG_PICK
    return v;
}
template <typename T, int RPT>
__device__ __forceinline__ void wg_put(T (&a)[RPT], int slot, T v)
{
#define MI32_WG_PUT(i) \
    case (i):          \
        if constexpr ((i) < RPT) a[(i)] = v; \
        break;
    switch (slot) { MI32_WG_CASES64(MI32_WG_PUT) default: break; }
#undef MI32_WG_PUT
}

// One member from the load to the un-permuted inverse on the whole workgroup, shared by the uniform and the
// variable-size kernel.  `in` / `out`: the member's first element, rows lda / ldo elements apart; everything but the
// thread's own column is workgroup-uniform.  Every element is in registers before the first store (the step loop's
// barriers lie between), so `out` may be `in`.  ROW_POINTER: the loads walk a pointer advanced by lda instead of forming
// row * lda + j per row (the same addresses; which of the two keeps the row masks out of the registers differs
// between the instances, see the variable-size kernel).  DET: every thread also multiplies each step's pivot into the
// determinant (det_accumulate of mi32_internal.h; the pivot and the swap predicate are workgroup-uniform, so the
// accumulator lives in scalar registers), thread 0 stores it to *det_mant / *det_exp, and a null `out` skips the
// inverse's stores.  SOLVE (A X = B, never with DET): the columns n ... n + cols - 1 hold the member's B columns `rhs`
// + 0 ... cols - 1 (rows ldb elements apart) and take the steps as any column >= n would -- they are never column r, so
// that is the row exchange, prn = b[p] / piv, the update by the published multipliers and b[r] = prn; slot s of such a
// column is row label[s] of X, stored to `out` + its column (rows ldo apart), and the columns < n store nothing.
template <typename T, int RPT, bool PIVOT, bool ROW_POINTER, bool DET, bool SOLVE = false>
__device__ __forceinline__ void workgroup_member(const T *in, T *out, const int n, const int lda, const int ldo,
                                                 int *status_word, double *det_mant = nullptr, int *det_exp = nullptr,
                                                 const T *rhs = nullptr, const int ldb = 0, const int cols = 0)
{
    static_assert(!(SOLVE && (DET || ROW_POINTER)), "the solve body loads by index and has no determinant");
    static_assert(RPT % 8 == 0 && RPT >= 40 && RPT <= 64, "rows per thread");
    constexpr int P = 2 * RPT;  // padded rows
    __shared__ __attribute__((aligned(32))) T s_col[2][kWorkgroupColumns];   // published column r, by step parity
    __shared__ __attribute__((aligned(32))) T s_prow[2][kWorkgroupColumns];  // normalised pivot row, by step parity
    __shared__ __attribute__((aligned(16))) int s_label[kWorkgroupColumns];  // slot -> logical row, for the store
    __shared__ int s_slot_of[kWorkgroupColumns];                             // logical row -> slot, for the store

    const int j = threadIdx.x & (kWorkgroupColumns - 1);
    const int h = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 7);  // wave-uniform
    const int lane = threadIdx.x & 63;
    const int slot0 = h * RPT;
    const bool mine = j < (SOLVE ? n + cols : n);
    // SOLVE: this thread's column of [A | B], its first element and row stride
    const T *colp0 = in;
    int ldc = lda;
    if constexpr (SOLVE) {
        colp0 = j < n ? in + j : mine ? rhs + (j - n) : in;  // (a column past the width reads A's first element)
        ldc = j < n ? lda : ldb;
    }

    T a[RPT];
    const T *rowp = in + ((size_t)slot0 * (size_t)lda + (size_t)j);  // this thread's entry of its slab's first row
    bool bad = false;  // boundary rule: a NaN / inf anywhere in the input is an invalid matrix
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
        const bool live = mine && slot0 + i < n;
        T v;  // loaded unconditionally (a dead slot reads the member's first element): the loads stay in flight together
        if constexpr (SOLVE) {
            v = colp0[live ? (size_t)(slot0 + i) * ldc : 0];
        } else if constexpr (ROW_POINTER) {
            v = *(live ? rowp : in);
            rowp += lda;
        } else {
            v = in[live ? (size_t)(slot0 + i) * lda + j : 0];
        }
        bad = bad || (live && v - v != T(0));
        a[i] = slot0 + i < n ? (mine ? v : T(0)) : not_a_candidate(T(0));
    }
    // this wave's copy of the labels of slots lane and lane + 64 (slots >= P exist in no register: never candidates)
    int lab0 = lane, lab1 = lane + 64;
    DetAcc det = det_start(false);
    // a non-finite input entry, seen by the thread that loaded it alone: the workgroup's accumulation never starts
    if constexpr (DET) det = det_start(__syncthreads_or(bad) != 0);

#pragma unroll 1
    for (int r = 0; r < n; ++r) {
        T *const colp = s_col[r & 1];
        T *const prowp = s_prow[r & 1];
        // a. column r: publish, then the implicit identity column takes its place
        if (j == r) {
#pragma unroll
            for (int i = 0; i < RPT; i += 4) {
                *reinterpret_cast<Vec4<T> *>(&colp[slot0 + i]) = Vec4<T>{a[i], a[i + 1], a[i + 2], a[i + 3]};
                a[i] = a[i + 1] = a[i + 2] = a[i + 3] = T(0);
            }
        }
        __syncthreads();
        // b. the pivot slot sp
        int sp = r;  // without pivoting the labels stay the identity
        bool swap = false;
        if constexpr (PIVOT) {
            const T v0 = colp[lane];
            const T v1 = lane + 64 < P ? colp[lane + 64] : not_a_candidate(T(0));  // (in bounds: 128 entries; a slot >= P is none)
            const PivotRec<T> k0 = PivotRec<T>::make(lab0 >= r ? v0 : not_a_candidate(T(0)), lab0);
            const PivotRec<T> k1 = PivotRec<T>::make(lab1 >= r ? v1 : not_a_candidate(T(0)), lab1);
            const PivotRec<T> best = wave_max_rec(PivotRec<T>::best_of(k0, k1));
            const int pl = __builtin_amdgcn_readfirstlane(best.row(r));  // the pivot's logical row; r when nothing is a candidate
            const unsigned long long m0 = __builtin_amdgcn_ballot_w64(lab0 == pl);
            const unsigned long long m1 = __builtin_amdgcn_ballot_w64(lab1 == pl);
            sp = m0 ? __builtin_ctzll(m0) : 64 + __builtin_ctzll(m1);
            swap = pl != r;
            // pivotElements: the two labels change places
            lab0 = lab0 == pl ? r : lab0 == r ? pl : lab0;
            lab1 = lab1 == pl ? r : lab1 == r ? pl : lab1;
        }
        const T piv = colp[sp];
        if constexpr (DET) det_accumulate<T, PIVOT, true>(det, piv, swap);
        bad = bad || piv == T(0) || piv - piv != T(0);  // zero, NaN or infinite pivot
        const int hp = sp >= RPT ? 1 : 0, lp = sp - hp * RPT;
        // c. fixRow in the slab that holds the pivot slot
        if (h == hp) prowp[j] = (j == r ? T(1) : wg_pick<T, RPT>(a, lp)) / piv;
        __syncthreads();
        // d. fixColumn
        const T prn = prowp[j];
#pragma unroll
        for (int i = 0; i < RPT; i += 4) {
            const Vec4<T> f = *reinterpret_cast<const Vec4<T> *>(&colp[slot0 + i]);  // the multipliers: old a[i][r]
            a[i + 0] = (f.x != T(0)) ? fma_t(-f.x, prn, a[i + 0]) : a[i + 0];
            a[i + 1] = (f.y != T(0)) ? fma_t(-f.y, prn, a[i + 1]) : a[i + 1];
            a[i + 2] = (f.z != T(0)) ? fma_t(-f.z, prn, a[i + 2]) : a[i + 2];
            a[i + 3] = (f.w != T(0)) ? fma_t(-f.w, prn, a[i + 3]) : a[i + 3];
        }
        if (h == hp) wg_put<T, RPT>(a, lp, prn);  // the pivot slot takes the normalised pivot row
    }

    int oc = j;
    if constexpr (PIVOT) {
        if (threadIdx.x < 64) {
            s_label[lane] = lab0;
            s_label[lane + 64] = lab1;
            if constexpr (!SOLVE) {
                s_slot_of[lab0] = lane;
                s_slot_of[lab1] = lane + 64;
            }
        }
        __syncthreads();
        if constexpr (!SOLVE) oc = s_slot_of[j];
    }
    if (!mine) return;
    if constexpr (SOLVE) {
        // X has no column permutation: the B column keeps its place, only the rows follow the labels
        if (j >= n) {
#pragma unroll
            for (int i = 0; i < RPT; ++i) {
                if (slot0 + i < n) {
                    const int row = PIVOT ? s_label[slot0 + i] : slot0 + i;
                    // (< n by construction, like the inverse's rows below)
                    if (row < n) out[(size_t)row * ldo + (j - n)] = a[i];
                }
            }
        }
        if (bad) *status_word = MI32_SINGULAR;
        return;
    }
    if constexpr (DET) {
        if (threadIdx.x == 0) {
            *det_mant = det.m;
            *det_exp = det.e;
        }
    }
    bool store = true;
    if constexpr (DET) store = out != nullptr;  // determinant only: status and determinant are all that is written
    if (store) {
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
            if (slot0 + i < n) {
                const int row = PIVOT ? s_label[slot0 + i] : slot0 + i;
                // (both are < n by construction: the labels of the slots < n are a permutation of 0 ... n - 1)
                if (row < n && oc < n) out[(size_t)row * ldo + oc] = a[i];
            }
        }
    }
    // the status word was zeroed (MI32_OK) by the host before this launch; every writer stores the same value
    if (bad) *status_word = MI32_SINGULAR;
}

template <typename T, int RPT, bool PIVOT>
__global__ __launch_bounds__(kWorkgroupThreads) void gj_workgroup_kernel(const T *__restrict__ in, T *__restrict__ out,
                                                                         int n, int *__restrict__ status)
{
    const size_t mat = (size_t)blockIdx.x * (size_t)n * (size_t)n;
    workgroup_member<T, RPT, PIVOT, false, false>(in + mat, out + mat, n, n, n, status + blockIdx.x);
}

// gj_workgroup_kernel with the determinant: member b's pair goes to det_mant[b], det_exp[b]; a null `out`: no inverse
template <typename T, int RPT, bool PIVOT>
__global__ __launch_bounds__(kWorkgroupThreads) void gj_workgroup_det_kernel(const T *__restrict__ in, T *__restrict__ out,
                                                                             int n, int *__restrict__ status,
                                                                             double *__restrict__ det_mant,
                                                                             int *__restrict__ det_exp)
{
    const size_t mat = (size_t)blockIdx.x * (size_t)n * (size_t)n;
    workgroup_member<T, RPT, PIVOT, false, true>(in + mat, out ? out + mat : nullptr, n, n, n, status + blockIdx.x,
                                                 det_mant + blockIdx.x, det_exp + blockIdx.x);
}

// A X = B: workgroup m of the launch takes member m and the columns col0 ... col0 + cols - 1 of its B.  B and X carry
// no __restrict__: X may be B (every element is in registers before the first store).
template <typename T, int RPT, bool PIVOT>
__global__ __launch_bounds__(kWorkgroupThreads) void gj_workgroup_solve_kernel(const SolveArgs<T> s)
{
    const size_t m = blockIdx.x;
    const size_t at = m * (size_t)s.n * (size_t)s.nrhs + (size_t)s.col0;
    workgroup_member<T, RPT, PIVOT, false, false, true>(s.a + m * (size_t)s.n * (size_t)s.n, s.x + at, s.n, s.n, s.nrhs,
                                                        s.status + m, nullptr, nullptr, s.b + at, s.nrhs, s.cols);
}

// The variable-size kernels: workgroup g of the launch takes member members[first + g] of the plan's sorted list; its
// order and leading dimensions (a null lda / ldinv: the order) are workgroup-uniform values.
struct WorkgroupSlot {
    int m, n, lda, ldo;  // the caller's member index, the member's order and leading dimensions
};
// (v by value: through a reference the kernel-argument loads are ordered differently)
template <typename T>
__device__ __forceinline__ WorkgroupSlot workgroup_slot(const VbatchArgs<T> v, const int first)
{
    WorkgroupSlot s;
    s.m = __builtin_amdgcn_readfirstlane(v.members[(size_t)first + blockIdx.x]);
    s.n = __builtin_amdgcn_readfirstlane(v.orders[s.m]);
    s.lda = v.lda ? __builtin_amdgcn_readfirstlane(v.lda[s.m]) : s.n;
    s.ldo = v.ldinv ? __builtin_amdgcn_readfirstlane(v.ldinv[s.m]) : s.n;
    return s;
}

// The member pointers carry no __restrict__: a member may be inverted in place.  ROW_POINTER = (RPT >= 56): with a
// leading dimension of its own the compiler branches around each row's 64-bit address and, at 56 and 64 rows per
// thread, spills the row masks to vector-register lanes (fp32 without pivoting: 129 / 132 registers); the row pointer
// avoids that there (101 / 118) and costs registers at 40 and 48 rows.
template <typename T, int RPT, bool PIVOT>
__global__ __launch_bounds__(kWorkgroupThreads) void gj_workgroup_vkernel(const VbatchArgs<T> v, const int first)
{
    const WorkgroupSlot s = workgroup_slot(v, first);
    workgroup_member<T, RPT, PIVOT, (RPT >= 56), false>(v.a[s.m], v.inv[s.m], s.n, s.lda, s.ldo, v.status + s.m);
}

// gj_workgroup_vkernel with the determinant, which lands at the caller's member index like the status word; d.v.inv may
// be null (determinant only)
template <typename T, int RPT, bool PIVOT>
__global__ __launch_bounds__(kWorkgroupThreads) void gj_workgroup_det_vkernel(const VbatchDetArgs<T> d, const int first)
{
    const WorkgroupSlot s = workgroup_slot(d.v, first);
    workgroup_member<T, RPT, PIVOT, (RPT >= 56), true>(d.v.a[s.m], d.v.inv ? d.v.inv[s.m] : nullptr, s.n, s.lda, s.ldo,
                                                       d.v.status + s.m, d.det_mant + s.m, d.det_exp + s.m);
}

// A X = B for a variable-size batch: workgroup g of the launch takes member members[first + g] of the plan's sorted
// list and the columns col0 ... col0 + cols - 1 of its B; the member's order and its three leading dimensions (a null
// lda: the order, a null ldb / ldx: nrhs) are workgroup-uniform values.
struct WorkgroupSolveSlot {
    int m, n, lda, ldb, ldx;
};
template <typename T>
__device__ __forceinline__ WorkgroupSolveSlot workgroup_slot(const VsolveArgs<T> v, const int first)
{
    WorkgroupSolveSlot s;
    s.m = __builtin_amdgcn_readfirstlane(v.members[(size_t)first + blockIdx.x]);
    s.n = __builtin_amdgcn_readfirstlane(v.orders[s.m]);
    s.lda = v.lda ? __builtin_amdgcn_readfirstlane(v.lda[s.m]) : s.n;
    s.ldb = v.ldb ? __builtin_amdgcn_readfirstlane(v.ldb[s.m]) : v.nrhs;
    s.ldx = v.ldx ? __builtin_amdgcn_readfirstlane(v.ldx[s.m]) : v.nrhs;
    return s;
}

// B and X carry no __restrict__: X may be B (every element is in registers before the first store)
template <typename T, int RPT, bool PIVOT>
__global__ __launch_bounds__(kWorkgroupThreads) void gj_workgroup_solve_vkernel(const VsolveArgs<T> v, const int first)
{
    const WorkgroupSolveSlot s = workgroup_slot(v, first);
    workgroup_member<T, RPT, PIVOT, false, false, true>(v.a[s.m], v.x[s.m] + v.col0, s.n, s.lda, s.ldx, v.status + s.m,
                                                        nullptr, nullptr, v.b[s.m] + v.col0, s.ldb, v.cols);
}

#undef MI32_WG_CASES8
#undef MI32_WG_CASES64

// f(rows per thread, pivot), both as compile-time constants (std::integral_constant): the one place where a run-time
// pair picks a kernel instance.  false: no instance has that many rows per thread.
template <typename F>
static bool workgroup_instance(int rows_per_thread, bool pivoting, F f)
{
    const auto pick = [&](auto rpt) {
        if (pivoting) f(rpt, std::true_type{});
        else f(rpt, std::false_type{});
        return true;
    };
    switch (rows_per_thread) {
        case 40: return pick(std::integral_constant<int, 40>{});
        case 48: return pick(std::integral_constant<int, 48>{});
        case 56: return pick(std::integral_constant<int, 56>{});
        case 64: return pick(std::integral_constant<int, 64>{});
        default: return false;
    }
}

template <typename T>
hipError_t workgroup_invert(const T *d_a, T *d_inv, int n, int batch, int *d_status, const DetOut det, hipStream_t stream,
                            Profiler *prof, bool pivoting)
{
    const int rows = workgroup_rows_per_thread(n);
    if (rows == 0 || batch <= 0 || !d_status || !det.valid() || (!d_inv && det.empty())) return hipErrorInvalidValue;
    ProfScope ps(prof, KC_PANEL, stream);  // pivot steps on a register-resident panel: the whole matrix
    workgroup_instance(rows, pivoting, [&](auto rpt, auto pivot) {
        constexpr int RPT = decltype(rpt)::value;
        constexpr bool PIVOT = decltype(pivot)::value;
        const dim3 grid((unsigned)batch);
        if (det.empty())
            hipLaunchKernelGGL((gj_workgroup_kernel<T, RPT, PIVOT>), grid, dim3(kWorkgroupThreads), 0, stream, d_a, d_inv, n,
                               d_status);
        else
            hipLaunchKernelGGL((gj_workgroup_det_kernel<T, RPT, PIVOT>), grid, dim3(kWorkgroupThreads), 0, stream, d_a,
                               d_inv, n, d_status, det.mant, det.exp);
    });
    return hipGetLastError();
}
template hipError_t workgroup_invert(const float *, float *, int, int, int *, DetOut, hipStream_t, Profiler *, bool);
template hipError_t workgroup_invert(const double *, double *, int, int, int *, DetOut, hipStream_t, Profiler *, bool);

template <typename T>
hipError_t workgroup_vinvert(int rows_per_thread, const VbatchArgs<T> &v, const DetOut det, int first, int count,
                             hipStream_t stream, Profiler *prof, bool pivoting)
{
    if (count <= 0 || first < 0 || !v.status || !det.valid() || (!v.inv && det.empty())) return hipErrorInvalidValue;
    const VbatchDetArgs<T> vd{v, det.mant, det.exp};
    ProfScope ps(prof, KC_PANEL, stream);
    const bool found = workgroup_instance(rows_per_thread, pivoting, [&](auto rpt, auto pivot) {
        constexpr int RPT = decltype(rpt)::value;
        constexpr bool PIVOT = decltype(pivot)::value;
        const dim3 grid((unsigned)count);
        if (det.empty())
            hipLaunchKernelGGL((gj_workgroup_vkernel<T, RPT, PIVOT>), grid, dim3(kWorkgroupThreads), 0, stream, v, first);
        else
            hipLaunchKernelGGL((gj_workgroup_det_vkernel<T, RPT, PIVOT>), grid, dim3(kWorkgroupThreads), 0, stream, vd,
                               first);
    });
    return found ? hipGetLastError() : hipErrorInvalidValue;
}
template hipError_t workgroup_vinvert(int, const VbatchArgs<float> &, DetOut, int, int, hipStream_t, Profiler *, bool);
template hipError_t workgroup_vinvert(int, const VbatchArgs<double> &, DetOut, int, int, hipStream_t, Profiler *, bool);

template <typename T>
hipError_t workgroup_solve(const SolveArgs<T> &s, hipStream_t stream, Profiler *prof, bool pivoting)
{
    const int rows = workgroup_solve_rows_per_thread(s.n);
    if (rows == 0 || s.batch <= 0 || s.cols < 1 || s.n + s.cols > kWorkgroupColumns || s.col0 < 0 ||
        s.col0 + s.cols > s.nrhs || !s.a || !s.b || !s.x || !s.status)
        return hipErrorInvalidValue;
    ProfScope ps(prof, KC_PANEL, stream);
    workgroup_instance(rows, pivoting, [&](auto rpt, auto pivot) {
        constexpr int RPT = decltype(rpt)::value;
        constexpr bool PIVOT = decltype(pivot)::value;
        hipLaunchKernelGGL((gj_workgroup_solve_kernel<T, RPT, PIVOT>), dim3((unsigned)s.batch), dim3(kWorkgroupThreads), 0,
                           stream, s);
    });
    return hipGetLastError();
}
template hipError_t workgroup_solve(const SolveArgs<float> &, hipStream_t, Profiler *, bool);
template hipError_t workgroup_solve(const SolveArgs<double> &, hipStream_t, Profiler *, bool);

// every member of the range has an order of this rows-per-thread class and a width n + cols of at most 128 columns:
// the caller's business, like the leading dimensions
template <typename T>
hipError_t workgroup_vsolve(int rows_per_thread, const VsolveArgs<T> &v, int first, int count, hipStream_t stream,
                            Profiler *prof, bool pivoting)
{
    if (count <= 0 || first < 0 || v.cols < 1 || v.cols >= kWorkgroupColumns || v.col0 < 0 || v.col0 + v.cols > v.nrhs ||
        !v.orders || !v.members || !v.a || !v.b || !v.x || !v.status)
        return hipErrorInvalidValue;
    ProfScope ps(prof, KC_PANEL, stream);
    const bool found = workgroup_instance(rows_per_thread, pivoting, [&](auto rpt, auto pivot) {
        constexpr int RPT = decltype(rpt)::value;
        constexpr bool PIVOT = decltype(pivot)::value;
        hipLaunchKernelGGL((gj_workgroup_solve_vkernel<T, RPT, PIVOT>), dim3((unsigned)count), dim3(kWorkgroupThreads), 0,
                           stream, v, first);
    });
    return found ? hipGetLastError() : hipErrorInvalidValue;
}
template hipError_t workgroup_vsolve(int, const VsolveArgs<float> &, int, int, hipStream_t, Profiler *, bool);
template hipError_t workgroup_vsolve(int, const VsolveArgs<double> &, int, int, hipStream_t, Profiler *, bool);

}  // namespace mi32
