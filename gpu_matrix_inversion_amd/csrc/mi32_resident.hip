// mi32_resident.hip -- the register-resident path for large batches of small matrices (n <= 64), gfx950.
//
// One launch per call: a group of L lanes (L = 8, 16, 32 or 64, the smallest that is >= n) owns one matrix from
// the first pivot search to the un-permuted inverse; a wave holds 64 / L matrices, a workgroup four waves.  One
// global read and one global write per element, no workspace, no batch index in blockIdx.y / .z (the matrix index
// is a 64-bit function of blockIdx.x alone).
//
// Layout: lane j of the group holds COLUMN j of the working matrix, a[0 .. L) in registers, the N x N in-place
// form of mi32_sweep.hip (column r holds, from step r on, the one right-half column of [A|I] that went dense at
// step r).  Padding never reaches a stored value: a row >= n is NaN in every column -- a NaN never wins a pivot
// search, and a row only ever changes itself unless it is the pivot row -- and a lane >= n holds zeros, is read by
// no step r < n and never stores.
//
// Per pivot step r, the five kernels of the reference (mat_inv_32.cpp:317-362) in the arithmetic of
// gj_sweep_step_kernel, hence the same bits as the CPU oracle:
//   1. maxPivot / finalMaxPivot: column r lives in ONE lane, so the search is a scan over that lane's registers
//      (every lane scans its own column, lane r's answer is broadcast): PivotRec<T> of mi32_sweep_common.h
//   2. pivotElements: the pivot row's entry of this lane's column is picked by a compare/select chain on p (a
//      run-time register index would go through scratch); slot p receives the old row r
//   3. fixRow: ONE IEEE division per lane and step, prn = a[p][j] / piv; column r's lane takes 1 / piv
//   4. fixColumn: row i != r takes its multiplier f = old a[i][r] from column r's lane of the group; column r's own
//      entry becomes 0 first (the implicit identity column); a[i] = fma(-f, prn, a[i]), skipped when f == 0
//   5. a zero / NaN / infinite pivot, or a non-finite input entry, flags the member MI32_SINGULAR
// The column permutation of the sweep (working column c holds inverse column orig[c]) is carried in the lanes
// (lane c holds orig[c]) and applied by the store.
//
// The loops over ROWS are fully unrolled, so every register index is a compile-time constant (no scratch).  The
// loop over pivot STEPS is unrolled for L <= 16 only: for L = 32 / 64 the unrolled body would be 1024 / 4096 row
// updates of straight-line code per instance (~75 / ~300 KB, more than an instruction cache holds, times 8
// instances), so there r is a run-time, wave-uniform value that is only ever compared with the compile-time row
// index or used as a lane index.
//
// Every kernel of the file is made of one load (resident_load), one step loop (resident_steps) and one store
// (resident_store): the inverse and determinant kernels through resident_member, the A X = B kernels through
// resident_solve_member.  The variable-size kernels (mi32_inv_device_vbatched, mi32_solve_device_vbatched) are the same
// bodies: every group looks up its member's order, pointers and leading dimensions (resident_vgroup), and the groups of
// a wave may differ in order.
#include <type_traits>

#include "mi32_internal.h"
#include "mi32_sweep_common.h"

namespace mi32 {

static constexpr int kResidentThreads = 256;

int resident_lanes(int n) { return n <= 0 || n > kResidentMaxOrder ? 0 : n <= 8 ? 8 : n <= 16 ? 16 : n <= 32 ? 32 : 64; }

// the value lane `src` of this lane's group of L holds.  L = 64: the group is the wave and every caller's src is
// wave-uniform, so this is a v_readlane into a scalar register; smaller groups go through ds_bpermute.
template <int L>
__device__ __forceinline__ int group_bcast(int v, int src)
{
    if constexpr (L == 64) return __builtin_amdgcn_readlane(v, src);
    else return __shfl(v, src, L);
}
template <int L>
__device__ __forceinline__ float group_bcast(float v, int src)
{
    return __int_as_float(group_bcast<L>(__float_as_int(v), src));
}
template <int L>
__device__ __forceinline__ double group_bcast(double v, int src)
{
    return __hiloint2double(group_bcast<L>(__double2hiint(v), src), group_bcast<L>(__double2loint(v), src));
}

// A wave-uniform row number as a vector register the compiler cannot see through.  With a run-time step the row
// tests `i >= r`, `i == r`, `i == p` of an unrolled row loop are otherwise evaluated on the scalar unit, all of them
// ahead of the loop, and their 2 L mask registers are spilled to vector-register lanes (v_writelane / v_readlane
// around every use: measured in the code object, 204 registers at L = 64).  As a vector compare each test is one
// instruction whose mask is consumed by the next.  A compile-time row number stays what it is.
template <int L>
__device__ __forceinline__ int row_number(int r)
{
    if constexpr (L > 16) asm volatile("" : "+v"(r));
    return r;
}

// One pivot step on the group's matrix.  r: the step (a compile-time constant after unrolling for L <= 16).  DET: the
// step also multiplies its pivot into the determinant `det` (det_accumulate of mi32_internal.h); every lane of the group
// holds the pivot and the swap predicate, so all of them accumulate, redundantly.
template <typename T, int L, bool PIVOT, bool DET>
__device__ __forceinline__ void resident_step(T (&a)[L], const int r, const int j, int &orig, bool &bad, DetAcc &det)
{
    // 1. the pivot row p of column r: rows >= n hold NaN and are no candidates, like the rows above r
    int p = r;
    if constexpr (PIVOT) {
        const int rv = row_number<L>(r);
        PivotRec<T> best = PivotRec<T>::none();
#pragma unroll
        for (int i = 0; i < L; ++i) {
            const T cand = (i >= rv) ? a[i] : not_a_candidate(T(0));
            best = PivotRec<T>::best_of(PivotRec<T>::make(cand, i), best);
        }
        p = group_bcast<L>(best.row(r), r);
    }
    // 2. pivotElements: this column's entry of row r, then its entry of row p (the pivot row), whose slot
    //    receives the old row r
    T ar = T(0);
    {
        const int rv = row_number<L>(r);
#pragma unroll
        for (int i = 0; i < L; ++i) ar = (i == rv) ? a[i] : ar;
    }
    T ap = ar;
    if constexpr (PIVOT) {
        const int pv = row_number<L>(p);
#pragma unroll
        for (int i = 0; i < L; ++i) {
            ap = (i == pv) ? a[i] : ap;
            a[i] = (i == pv) ? ar : a[i];
            // both selects of a row next to its compare: scheduled apart, the L masks stay live and are spilled
            if constexpr (L > 16) __builtin_amdgcn_sched_barrier(0);
        }
    }
    // 3. fixRow: the pivot is column r's entry of row p (mat_inv_32.cpp:70,129-130)
    const T piv = group_bcast<L>(ap, r);
    if constexpr (DET) det_accumulate<T, PIVOT, L == 64>(det, piv, p != r);
    bad = bad || piv == T(0) || piv - piv != T(0);  // zero, NaN or infinite pivot
    const bool is_r = (j == r);
    const T prn = (is_r ? T(1) : ap) / piv;
    // 4. fixColumn; slot r takes the normalised pivot row
    {
        const int rv = row_number<L>(r);
#pragma unroll
        for (int i = 0; i < L; ++i) {
            const T f = group_bcast<L>(a[i], r);    // the multiplier: old a[i][r]
            const T base = is_r ? T(0) : a[i];      // the implicit identity column's entry in this row
            const T upd = (f != T(0)) ? fma_t(-f, prn, base) : base;
            a[i] = (i == rv) ? prn : upd;
        }
    }
    // the column permutation: orig[r] <-> orig[p]
    if constexpr (PIVOT) {
        const int o_r = group_bcast<L>(orig, r), o_p = group_bcast<L>(orig, p);
        orig = is_r ? o_p : (j == p) ? o_r : orig;
    }
}

// The three pieces every kernel of this file is made of.  n: this GROUP's order (the same in its L lanes, 0 for a group
// that owns no member); nmax: the largest order in the wave, wave-uniform.
//
// The load: this lane's column, `col` its first element, rows ld elements apart.  A lane that is not `mine` (past the
// member's width, or in a group without a member) holds zeros and reads nothing.  Boundary rule: a NaN / inf anywhere
// in the input is an invalid member (`bad`).
template <typename T, int L>
__device__ __forceinline__ void resident_load(T (&a)[L], const T *col, const int ld, const int n, const bool mine, bool &bad)
{
#pragma unroll
    for (int i = 0; i < L; ++i) {
        if (i < n) {
            a[i] = mine ? col[(size_t)i * ld] : T(0);
            bad = bad || (a[i] - a[i] != T(0));
        } else {
            a[i] = not_a_candidate(T(0));  // a padded row stays NaN in every column and never wins a pivot search
        }
    }
}

// The step loop.  With UNIFORM_N every group of the wave has the order nmax (or none: the steps then run on zeros);
// without, a group sits out the steps past its own order -- a step on a finished group would flag it and destroy its
// result, and in a solve lane n of a finished group holds a column of B and would become a pivot column -- and every
// cross-lane operation of resident_step stays inside its group of L lanes, all of them in or all of them out.
template <typename T, int L, bool PIVOT, bool UNIFORM_N, bool DET>
__device__ __forceinline__ void resident_steps(T (&a)[L], const int n, const int nmax, const int j, int &orig, bool &bad,
                                               DetAcc &det)
{
    if constexpr (L <= 16) {
#pragma unroll
        for (int r = 0; r < L; ++r) {
            if constexpr (UNIFORM_N) {
                if (r < n) resident_step<T, L, PIVOT, DET>(a, r, j, orig, bad, det);  // n is wave-uniform: a scalar branch
            } else {
                if (r < nmax) {  // wave-uniform: no wave walks through the steps none of its groups takes
                    if (r < n) resident_step<T, L, PIVOT, DET>(a, r, j, orig, bad, det);
                }
            }
        }
    } else {
#pragma unroll 1
        for (int r = 0; r < nmax; ++r) {
            if constexpr (UNIFORM_N) resident_step<T, L, PIVOT, DET>(a, r, j, orig, bad, det);
            else if (r < n) resident_step<T, L, PIVOT, DET>(a, r, j, orig, bad, det);
        }
    }
}

// The store of this lane's rows < n to the column whose first element is `col`, rows ld elements apart.
template <typename T, int L>
__device__ __forceinline__ void resident_store(const T (&a)[L], T *col, const int ld, const int n)
{
#pragma unroll
    for (int i = 0; i < L; ++i)
        if (i < n) col[(size_t)i * ld] = a[i];
}

// One member from the load to the un-permuted inverse, shared by the uniform and the variable-size kernel.  `col`: this
// lane's column of the member, rows lda elements apart; `out`: the inverse's first element, rows ldo apart.  A group
// that owns no member neither loads nor stores.  Every element is in registers before the first store.  DET: the group's
// first lane also stores the member's determinant to *det_mant / *det_exp, and a null `out` skips the inverse's stores.
template <typename T, int L, bool PIVOT, bool UNIFORM_N, bool DET>
__device__ __forceinline__ void resident_member(const T *col, T *out, const int n, const int nmax, const int lda,
                                                const int ldo, const int j, const bool mine, int *status_word,
                                                double *det_mant = nullptr, int *det_exp = nullptr)
{
    T a[L];
    bool bad = false;
    resident_load<T, L>(a, col, lda, n, mine, bad);
    int orig = j;
    DetAcc det = det_start(false);
    if constexpr (DET) {
        // a non-finite input entry, seen by the lane of its column alone: the group's accumulation never starts
        const unsigned long long flagged = __builtin_amdgcn_ballot_w64(bad);
        const int g0 = (int)(__lane_id() & ~(unsigned)(L - 1));  // the group's first lane in the wave
        const unsigned long long group = L == 64 ? ~0ull : ((1ull << (L & 63)) - 1ull) << g0;
        det = det_start((flagged & group) != 0ull);
    }
    resident_steps<T, L, PIVOT, UNIFORM_N, DET>(a, n, nmax, j, orig, bad, det);
    if (!mine) return;
    if constexpr (DET) {
        if (j == 0) {
            *det_mant = det.m;
            *det_exp = det.e;
        }
    }
    bool store = true;
    if constexpr (DET) store = out != nullptr;  // determinant only: status and determinant are all that is written
    if (store) resident_store<T, L>(a, out + orig, ldo, n);  // the store applies the column permutation
    // the status word was zeroed (MI32_OK) by the host before this launch; every writer stores the same value
    if (bad) *status_word = MI32_SINGULAR;
}

// The uniform kernel pair's body: group b of the launch takes member b of the batch.  DET: member b's determinant goes to
// det_mant[b], det_exp[b], and a null `out` means no inverse.
template <typename T, int L, bool PIVOT, bool DET>
__device__ __forceinline__ void resident_umember(const T *in, T *out, const int n, const int batch, int *status,
                                                 double *det_mant, int *det_exp)
{
    constexpr int kGroups = kResidentThreads / L;  // matrices per workgroup
    const int j = threadIdx.x & (L - 1);
    const long long b = (long long)blockIdx.x * kGroups + threadIdx.x / L;
    // a group past the end of the batch runs the steps on zeros (the cross-lane operations are whole-wave) and
    // neither loads nor stores
    const bool mine = b < (long long)batch && j < n;
    const size_t mat = mine ? (size_t)b * (size_t)n * (size_t)n : 0;
    if constexpr (DET) {
        const size_t w = mine ? (size_t)b : 0;
        resident_member<T, L, PIVOT, true, true>(in + mat + j, out ? out + mat : nullptr, n, n, n, n, j, mine, status + w,
                                                 det_mant + w, det_exp + w);
    } else {
        resident_member<T, L, PIVOT, true, false>(in + mat + j, out + mat, n, n, n, n, j, mine, status + (mine ? b : 0));
    }
}

template <typename T, int L, bool PIVOT>
__global__ __launch_bounds__(kResidentThreads) void gj_resident_kernel(const T *__restrict__ in, T *__restrict__ out,
                                                                       int n, int batch, int *__restrict__ status)
{
    resident_umember<T, L, PIVOT, false>(in, out, n, batch, status, nullptr, nullptr);
}

// gj_resident_kernel with the determinant
template <typename T, int L, bool PIVOT>
__global__ __launch_bounds__(kResidentThreads) void gj_resident_det_kernel(const T *__restrict__ in, T *__restrict__ out,
                                                                           int n, int batch, int *__restrict__ status,
                                                                           double *__restrict__ det_mant,
                                                                           int *__restrict__ det_exp)
{
    resident_umember<T, L, PIVOT, true>(in, out, n, batch, status, det_mant, det_exp);
}

// A group's member in a variable-size launch: group g takes member members[first + g] of the plan's sorted list.  The
// list is sorted by order, so the groups of a wave almost always share one; where they do not the wave loops to its
// largest (nmax).  A group past the end of the range has no member (valid false, m = n = 0).  For L = 64 the group is
// the wave and the group index, the member index and the order are scalar values, hence so is everything a kernel
// looks up by them (pointers, leading dimensions).
struct ResidentGroup {
    bool valid;
    int m, n, nmax;
};
template <int L>
__device__ __forceinline__ ResidentGroup resident_vgroup(const int *orders, const int *members, const int first,
                                                         const int count)
{
    constexpr int kGroups = kResidentThreads / L;  // members per workgroup
    int grp = threadIdx.x / L;
    if constexpr (L == 64) grp = __builtin_amdgcn_readfirstlane(grp);  // the group is the wave
    const long long g = (long long)blockIdx.x * kGroups + grp;
    const bool valid = g < (long long)count;
    int m = valid ? members[(size_t)first + (size_t)g] : 0;
    if constexpr (L == 64) m = __builtin_amdgcn_readfirstlane(m);
    int n = valid ? orders[m] : 0;
    if constexpr (L == 64) n = __builtin_amdgcn_readfirstlane(n);
    int nmax = n;
    if constexpr (L < 64) {
#pragma unroll
        for (int off = L; off < 64; off <<= 1) {
            const int o = __shfl_xor(nmax, off, 64);
            nmax = o > nmax ? o : nmax;
        }
        nmax = __builtin_amdgcn_readfirstlane(nmax);
    }
    return {valid, m, n, nmax};
}

// The variable-size kernel pair's body: the group reads its member's pointers and leading dimensions (a null lda /
// ldinv: the order).  The member pointers carry no __restrict__: a member may be inverted in place.  The guarded step
// loop also at L = 64, where n is nmax: the uniform loop costs these instances up to 60 registers.
template <typename T, int L, bool PIVOT, bool DET>
__device__ __forceinline__ void resident_vmember(const VbatchArgs<T> &v, const int first, const int count, double *det_mant,
                                                 int *det_exp)
{
    const int j = threadIdx.x & (L - 1);
    const ResidentGroup grp = resident_vgroup<L>(v.orders, v.members, first, count);
    const int m = grp.m, n = grp.n;
    const bool mine = grp.valid && j < n;
    const T *col = nullptr;
    T *out = nullptr;
    int lda = n, ldo = n;
    if (mine) {
        col = v.a[m] + j;
        if (!DET || v.inv) out = v.inv[m];
        if (v.lda) lda = v.lda[m];
        if (v.ldinv) ldo = v.ldinv[m];
    }
    // the determinant lands at the caller's member index, like the status word
    if constexpr (DET) resident_member<T, L, PIVOT, false, true>(col, out, n, grp.nmax, lda, ldo, j, mine, v.status + m,
                                                                 det_mant + m, det_exp + m);
    else resident_member<T, L, PIVOT, false, false>(col, out, n, grp.nmax, lda, ldo, j, mine, v.status + m);
}

template <typename T, int L, bool PIVOT>
__global__ __launch_bounds__(kResidentThreads) void gj_resident_vkernel(const VbatchArgs<T> v, const int first,
                                                                        const int count)
{
    resident_vmember<T, L, PIVOT, false>(v, first, count, nullptr, nullptr);
}

// gj_resident_vkernel with the determinant; v.v.inv may be null (determinant only)
template <typename T, int L, bool PIVOT>
__global__ __launch_bounds__(kResidentThreads) void gj_resident_det_vkernel(const VbatchDetArgs<T> v, const int first,
                                                                            const int count)
{
    resident_vmember<T, L, PIVOT, true>(v.v, first, count, v.det_mant, v.det_exp);
}

// A X = B: group m of the launch takes member m; its lanes j < n hold the columns of A as above, its lanes n ... n +
// cols - 1 the columns col0 ... of the member's B, and the steps are resident_step's, unchanged: a lane >= n is never
// column r, so it takes the row exchange, prn = b[p] / piv, the update by column r's multipliers and b[r] = prn.  The
// rows are exchanged physically, so register row i of such a lane is row i of X; the lanes < n store nothing and the
// column bookkeeping (`orig`) is dead.  `col`: this lane's column of A or B, rows ld elements apart; rhs: the lane holds
// a column of B.  x_of() gives the lane's column of X and its leading dimension; it is called after the step loop, so
// that what it reads is not held in registers across the steps.  A boundary rule as above: a NaN / inf anywhere in A
// or B is an invalid member.  The uniform and the variable-size kernel share this body.
template <typename T>
struct ResidentColumn {
    T *first;  // the column's first element
    int ld;    // its rows are ld elements apart
};
template <typename T, int L, bool PIVOT, bool UNIFORM_N, typename XOf>
__device__ __forceinline__ void resident_solve_member(const T *col, const int ld, const int n, const int nmax, const int j,
                                                      const bool mine, const bool rhs, int *status_word, XOf x_of)
{
    T a[L];
    bool bad = false;
    resident_load<T, L>(a, col, ld, n, mine, bad);
    int orig = j;
    DetAcc det = det_start(false);
    resident_steps<T, L, PIVOT, UNIFORM_N, false>(a, n, nmax, j, orig, bad, det);
    if (!mine) return;
    if (rhs) {
        const ResidentColumn<T> x = x_of();
        resident_store<T, L>(a, x.first, x.ld, n);
    }
    // the status word was zeroed (MI32_OK) by the host before the call's first launch; every writer stores the same value
    if (bad) *status_word = MI32_SINGULAR;
}

// The uniform solve kernel: group m of the launch takes member m of the batch.  B and X carry no __restrict__: X may
// be B (a lane stores the column it loaded).
template <typename T, int L, bool PIVOT>
__global__ __launch_bounds__(kResidentThreads) void gj_resident_solve_kernel(const SolveArgs<T> s)
{
    constexpr int kGroups = kResidentThreads / L;  // members per workgroup
    const int j = threadIdx.x & (L - 1);
    const long long m = (long long)blockIdx.x * kGroups + threadIdx.x / L;
    const int n = s.n;
    // a group past the end of the batch, and a lane past the launch's width, run the steps on zeros
    const bool mine = m < (long long)s.batch && j < n + s.cols;
    const bool rhs = j >= n;
    const size_t member = mine ? (size_t)m : 0;
    const size_t rhs_at = member * (size_t)n * (size_t)s.nrhs + (size_t)(s.col0 + (rhs ? j - n : 0));
    const T *col = rhs ? s.b + rhs_at : s.a + (member * (size_t)n * (size_t)n + (size_t)j);
    resident_solve_member<T, L, PIVOT, true>(col, rhs ? s.nrhs : n, n, n, j, mine, rhs, s.status + member,
                                             [&] { return ResidentColumn<T>{s.x + rhs_at, s.nrhs}; });
}

// A X = B for a variable-size batch: group g of the launch takes member members[first + g] of the plan's sorted list
// and the columns col0 ... col0 + cols - 1 of its B; every member of the launch has a width n + cols of this lane class.
// The groups of a wave may differ in order, so B sits in a different lane in each, and a group sits out the steps past
// its own order: here that guard of resident_steps carries the result.  For L = 64 the group is the wave, n is nmax
// and the step loop is the uniform one: the guard, never false there, is not left for the compiler to fold, because
// whether it folds it decides the schedule of the step (unfolded: 3 % slower here).  X's pointer
// and leading dimension are looked up after the steps.  No pointer carries __restrict__: X may be B.
template <typename T, int L, bool PIVOT>
__global__ __launch_bounds__(kResidentThreads) void gj_resident_solve_vkernel(const VsolveArgs<T> v, const int first,
                                                                              const int count)
{
    const int j = threadIdx.x & (L - 1);
    const ResidentGroup grp = resident_vgroup<L>(v.orders, v.members, first, count);
    const int m = grp.m, n = grp.n;
    // a group past the end of the range, and a lane past the member's width, hold zeros and neither load nor store
    const bool mine = grp.valid && j < n + v.cols;
    const bool rhs = j >= n;
    const int xcol = v.col0 + (rhs ? j - n : 0);  // this lane's column of B and X
    const T *col = nullptr;
    int ld = 0;
    if (mine) {
        const int lda = v.lda ? v.lda[m] : n;
        const int ldb = v.ldb ? v.ldb[m] : v.nrhs;
        col = rhs ? v.b[m] + xcol : v.a[m] + j;
        ld = rhs ? ldb : lda;
    }
    resident_solve_member<T, L, PIVOT, L == 64>(col, ld, n, grp.nmax, j, mine, rhs, v.status + m, [&] {
        return ResidentColumn<T>{v.x[m] + xcol, v.ldx ? v.ldx[m] : v.nrhs};
    });
}

// The one launch helper: picks the instance by its lanes per matrix (pick_instance of mi32_internal.h) and hands
// `launch` L and PIVOT as compile-time constants and the grid for `groups` groups of L lanes (a 64-bit count: no batch
// index in blockIdx.y / .z).  hipErrorInvalidValue when `lanes` names no instance.
template <typename F>
static hipError_t resident_launch(int lanes, bool pivoting, int groups, hipStream_t stream, Profiler *prof, F launch)
{
    ProfScope ps(prof, KC_PANEL, stream);  // pivot steps on a register-resident panel: the whole matrix
    const bool found = pick_instance<8, 16, 32, 64>(lanes, pivoting, [&](auto l, auto pivot) {
        constexpr int kGroups = kResidentThreads / decltype(l)::value;
        launch(l, pivot, dim3((unsigned)(((long long)groups + kGroups - 1) / kGroups)), dim3(kResidentThreads));
    });
    return found ? hipGetLastError() : hipErrorInvalidValue;
}

template <typename T>
hipError_t resident_invert(const T *d_a, T *d_inv, int n, int batch, int *d_status, const DetOut det, hipStream_t stream,
                           Profiler *prof, bool pivoting)
{
    const int lanes = resident_lanes(n);
    if (lanes == 0 || batch <= 0 || !d_status || !det.valid() || (!d_inv && det.empty())) return hipErrorInvalidValue;
    return resident_launch(lanes, pivoting, batch, stream, prof, [&](auto l, auto pivot, dim3 grid, dim3 block) {
        constexpr int L = decltype(l)::value;
        constexpr bool PIVOT = decltype(pivot)::value;
        if (det.empty())
            hipLaunchKernelGGL((gj_resident_kernel<T, L, PIVOT>), grid, block, 0, stream, d_a, d_inv, n, batch, d_status);
        else
            hipLaunchKernelGGL((gj_resident_det_kernel<T, L, PIVOT>), grid, block, 0, stream, d_a, d_inv, n, batch, d_status,
                               det.mant, det.exp);
    });
}
template hipError_t resident_invert(const float *, float *, int, int, int *, DetOut, hipStream_t, Profiler *, bool);
template hipError_t resident_invert(const double *, double *, int, int, int *, DetOut, hipStream_t, Profiler *, bool);

template <typename T>
hipError_t resident_vinvert(int lanes, const VbatchArgs<T> &v, const DetOut det, int first, int count, hipStream_t stream,
                            Profiler *prof, bool pivoting)
{
    if (count <= 0 || first < 0 || !v.status || !det.valid() || (!v.inv && det.empty())) return hipErrorInvalidValue;
    const VbatchDetArgs<T> vd{v, det.mant, det.exp};
    return resident_launch(lanes, pivoting, count, stream, prof, [&](auto l, auto pivot, dim3 grid, dim3 block) {
        constexpr int L = decltype(l)::value;
        constexpr bool PIVOT = decltype(pivot)::value;
        if (det.empty()) hipLaunchKernelGGL((gj_resident_vkernel<T, L, PIVOT>), grid, block, 0, stream, v, first, count);
        else hipLaunchKernelGGL((gj_resident_det_vkernel<T, L, PIVOT>), grid, block, 0, stream, vd, first, count);
    });
}
template hipError_t resident_vinvert(int, const VbatchArgs<float> &, DetOut, int, int, hipStream_t, Profiler *, bool);
template hipError_t resident_vinvert(int, const VbatchArgs<double> &, DetOut, int, int, hipStream_t, Profiler *, bool);

template <typename T>
hipError_t resident_solve(const SolveArgs<T> &s, hipStream_t stream, Profiler *prof, bool pivoting)
{
    const int lanes = s.n >= 1 && s.cols >= 1 ? resident_lanes(s.n + s.cols) : 0;
    if (lanes == 0 || s.batch <= 0 || s.col0 < 0 || s.col0 + s.cols > s.nrhs || !s.a || !s.b || !s.x || !s.status)
        return hipErrorInvalidValue;
    return resident_launch(lanes, pivoting, s.batch, stream, prof, [&](auto l, auto pivot, dim3 grid, dim3 block) {
        hipLaunchKernelGGL((gj_resident_solve_kernel<T, decltype(l)::value, decltype(pivot)::value>), grid, block, 0, stream,
                           s);
    });
}
template hipError_t resident_solve(const SolveArgs<float> &, hipStream_t, Profiler *, bool);
template hipError_t resident_solve(const SolveArgs<double> &, hipStream_t, Profiler *, bool);

template <typename T>
hipError_t resident_vsolve(int lanes, const VsolveArgs<T> &v, int first, int count, hipStream_t stream, Profiler *prof,
                           bool pivoting)
{
    if (count <= 0 || first < 0 || v.cols < 1 || v.cols >= lanes || v.col0 < 0 || v.col0 + v.cols > v.nrhs || !v.orders ||
        !v.members || !v.a || !v.b || !v.x || !v.status)
        return hipErrorInvalidValue;
    return resident_launch(lanes, pivoting, count, stream, prof, [&](auto l, auto pivot, dim3 grid, dim3 block) {
        hipLaunchKernelGGL((gj_resident_solve_vkernel<T, decltype(l)::value, decltype(pivot)::value>), grid, block, 0, stream,
                           v, first, count);
    });
}
template hipError_t resident_vsolve(int, const VsolveArgs<float> &, int, int, hipStream_t, Profiler *, bool);
template hipError_t resident_vsolve(int, const VsolveArgs<double> &, int, int, hipStream_t, Profiler *, bool);

}  // namespace mi32
