// mi32_slab.h -- the slab-resident member body of the workgroup path (mi32_workgroup.hip: 2 slabs of 128 column lanes,
// orders 65 ... 128) and the wide path (mi32_wide.hip: 4 slabs of 192 / 256 column lanes, fp32 orders 129 ... 256).
// __device__ templates only; the kernels, their classes and their launchers are in the two .hip files.
//
// Layout: the matrix lives in the workgroup's REGISTERS.  The workgroup is SLABS slabs of C column lanes; thread (slab
// h, column j) -- h = threadIdx.x / C, C a multiple of 64, so a slab is whole waves and every `h == hp` branch is
// wave-uniform -- holds the register slots h * RPT ... h * RPT + RPT - 1 of column j; RPT = 40 / 48 / 56 / 64 gives
// P = SLABS * RPT padded rows.  A slot >= n is NaN in every column (a NaN never wins a pivot search, and a row only
// ever changes itself unless it is the pivot row); a column >= n holds zeros, is published by no step r < n and never
// stores.
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
//   a. the SLABS threads of column r publish their slots and then zero them (the implicit identity column's entries)
//   b. barrier; EVERY wave searches the published column redundantly: lane l builds the PivotRec<T> of slots l + 64 k,
//      k < SLABS, from its copy of their labels, one wave reduction; the labels live in SLABS registers per lane of
//      every wave (kept identical by construction) and reach LDS once, for the store
//   c. the slab that holds the pivot slot picks its entry with a wave-uniform switch (scalar branches, no run-time
//      register index), divides ONCE per column, prn = a[p][j] / piv (column r: 1 / piv), and publishes prn
//   d. barrier; every slot takes its multiplier f = published column entry by ds_read_b128 at compile-time offsets (all
//      lanes read one address: a broadcast) and a[i] = fma(-f, prn, a[i]), skipped when f == 0; the pivot slot
//      is then overwritten with prn by a second wave-uniform switch
//   e. a zero / NaN / infinite pivot, or a non-finite input entry, flags the member MI32_SINGULAR
#pragma once
#include "mi32_internal.h"
#include "mi32_sweep_common.h"

namespace mi32 {

// `X(i)` for i = 0 ... 63 as the cases of a switch; slots >= RPT are discarded at compile time
#define MI32_SLAB_CASES8(X, b) X(b + 0) X(b + 1) X(b + 2) X(b + 3) X(b + 4) X(b + 5) X(b + 6) X(b + 7)
#define MI32_SLAB_CASES64(X)                                                                                    \
    MI32_SLAB_CASES8(X, 0) MI32_SLAB_CASES8(X, 8) MI32_SLAB_CASES8(X, 16) MI32_SLAB_CASES8(X, 24)                \
    MI32_SLAB_CASES8(X, 32) MI32_SLAB_CASES8(X, 40) MI32_SLAB_CASES8(X, 48) MI32_SLAB_CASES8(X, 56)

// a[slot] for a wave-uniform slot held in a scalar register: a tree of scalar branches around one move
template <typename T, int RPT>
__device__ __forceinline__ T slab_pick(const T (&a)[RPT], int slot)
{
    T v = T(0);
#define MI32_SLAB_PICK(i) \
    case (i):             \
        if constexpr ((i) < RPT) v = a[(i)]; \
        break;
    switch (slot) { MI32_SLAB_CASES64(MI32_SLAB_PICK) default: break; }
#undef MI32_SLAB_PICK
    return v;
}
template <typename T, int RPT>
__device__ __forceinline__ void slab_put(T (&a)[RPT], int slot, T v)
{
#define MI32_SLAB_PUT(i) \
    case (i):            \
        if constexpr ((i) < RPT) a[(i)] = v; \
        break;
    switch (slot) { MI32_SLAB_CASES64(MI32_SLAB_PUT) default: break; }
#undef MI32_SLAB_PUT
}
#undef MI32_SLAB_CASES8
#undef MI32_SLAB_CASES64

// the slot whose ballot is set: the first non-empty mask from K on, the last one untested (exactly one of the masks is
// non-zero, the labels being a permutation, and __builtin_ctzll of zero is never evaluated)
template <int K, int SLABS>
__device__ __forceinline__ int slab_first_slot(const unsigned long long (&m)[SLABS])
{
    if constexpr (K == SLABS - 1) return 64 * K + __builtin_ctzll(m[K]);
    else return m[K] ? 64 * K + __builtin_ctzll(m[K]) : slab_first_slot<K + 1, SLABS>(m);
}

// One member from the load to the un-permuted inverse on the whole workgroup of SLABS * C threads.  `in` / `out`: the
// member's first element, rows lda / ldo elements apart; everything but the thread's own column is workgroup-uniform.
// Every element is in registers before the first store (the step loop's barriers lie between), so `out` may be `in`.
// ROW_POINTER: the loads walk a pointer advanced by lda instead of forming row * lda + j per row (the same addresses;
// which of the two keeps the row masks out of the registers differs between the instances, see the variable-size
// kernels).  DET: every thread also multiplies each step's pivot into the determinant (det_accumulate of
// mi32_internal.h; the pivot and the swap predicate are workgroup-uniform, so the accumulator lives in scalar
// registers), thread 0 stores it to *det_mant / *det_exp, and a null `out` skips the inverse's stores.  SOLVE (A X = B,
// never with DET): the columns n ... n + cols - 1 hold the member's B columns `rhs` + 0 ... cols - 1 (rows ldb elements
// apart) and take the steps as any column >= n would -- they are never column r, so that is the row exchange,
// prn = b[p] / piv, the update by the published multipliers and b[r] = prn; slot s of such a column is row label[s] of
// X, stored to `out` + its column (rows ldo apart), and the columns < n store nothing.
template <typename T, int SLABS, int C, int RPT, bool PIVOT, bool ROW_POINTER, bool DET, bool SOLVE = false>
__device__ __forceinline__ void slab_member(const T *in, T *out, const int n, const int lda, const int ldo,
                                            int *status_word, double *det_mant = nullptr, int *det_exp = nullptr,
                                            const T *rhs = nullptr, const int ldb = 0, const int cols = 0)
{
    static_assert(!(SOLVE && (DET || ROW_POINTER)), "the solve body loads by index and has no determinant");
    static_assert(RPT % 8 == 0 && RPT >= 40 && RPT <= 64, "rows per thread");
    static_assert((SLABS == 2 || SLABS == 4) && C % 64 == 0 && C <= 64 * SLABS, "a slab is whole waves");
    constexpr int P = SLABS * RPT;  // padded rows
    constexpr int L = 64 * SLABS;   // the most padded rows (RPT <= 64) and column lanes: the LDS arrays' length
    __shared__ __attribute__((aligned(32))) T s_col[2][L];   // published column r, by step parity
    __shared__ __attribute__((aligned(32))) T s_prow[2][L];  // normalised pivot row, by step parity
    __shared__ __attribute__((aligned(16))) int s_label[L];  // slot -> logical row, for the store
    __shared__ int s_slot_of[L];                             // logical row -> slot, for the store

    // (a power of two as mask and shift, spelled out: the compiler does not fold the general form behind readfirstlane)
    int j, h;  // h is wave-uniform
    if constexpr ((C & (C - 1)) == 0) {
        j = threadIdx.x & (C - 1);
        h = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> __builtin_ctz(C));
    } else {
        h = __builtin_amdgcn_readfirstlane((int)threadIdx.x / C);
        j = (int)threadIdx.x - h * C;
    }
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
    // this wave's copy of the labels of slots lane + 64 k (slots >= P exist in no register: never candidates); the first
    // SLABS are used.  (A list, not a loop: with a loop between the load loop and the step loop the ROW_POINTER
    // instances take up to 18 vector registers and 120 scalar spills more)
    int lab[4] = {lane, lane + 64, lane + 128, lane + 192};
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
            const T none = not_a_candidate(T(0));
            PivotRec<T> rec[SLABS];
#pragma unroll
            for (int k = 0; k < SLABS; ++k) {
                // (in bounds: L entries; a slot >= P is written by nobody and is no candidate)
                const T v = lane + 64 * k < P ? colp[lane + 64 * k] : none;
                rec[k] = PivotRec<T>::make(lab[k] >= r ? v : none, lab[k]);
            }
            // pairwise: (0, 1), (2, 3), then their winners
#pragma unroll
            for (int w = 1; w < SLABS; w *= 2) {
#pragma unroll
                for (int k = 0; k + w < SLABS; k += 2 * w) rec[k] = PivotRec<T>::best_of(rec[k], rec[k + w]);
            }
            const PivotRec<T> best = wave_max_rec(rec[0]);
            const int pl = __builtin_amdgcn_readfirstlane(best.row(r));  // the pivot's logical row; r when nothing is a candidate
            unsigned long long m[SLABS];
#pragma unroll
            for (int k = 0; k < SLABS; ++k) m[k] = __builtin_amdgcn_ballot_w64(lab[k] == pl);
            sp = slab_first_slot<0, SLABS>(m);
            swap = pl != r;
            // pivotElements: the two labels change places
#pragma unroll
            for (int k = 0; k < SLABS; ++k) lab[k] = lab[k] == pl ? r : lab[k] == r ? pl : lab[k];
        }
        const T piv = colp[sp];
        if constexpr (DET) det_accumulate<T, PIVOT, true>(det, piv, swap);
        bad = bad || piv == T(0) || piv - piv != T(0);  // zero, NaN or infinite pivot
        int hp;  // (two slabs as a comparison, spelled out like the column index above)
        if constexpr (SLABS == 2) hp = sp >= RPT ? 1 : 0;
        else hp = sp / RPT;
        const int lp = sp - hp * RPT;
        // c. fixRow in the slab that holds the pivot slot
        if (h == hp) prowp[j] = (j == r ? T(1) : slab_pick<T, RPT>(a, lp)) / piv;
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
        if (h == hp) slab_put<T, RPT>(a, lp, prn);  // the pivot slot takes the normalised pivot row
    }

    int oc = j;
    if constexpr (PIVOT) {
        if (threadIdx.x < 64) {
#pragma unroll
            for (int k = 0; k < SLABS; ++k) s_label[lane + 64 * k] = lab[k];
            if constexpr (!SOLVE) {
#pragma unroll
                for (int k = 0; k < SLABS; ++k) s_slot_of[lab[k]] = lane + 64 * k;
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

}  // namespace mi32
