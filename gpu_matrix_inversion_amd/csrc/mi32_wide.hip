// mi32_wide.hip -- the wide workgroup-resident path for large batches of fp32 matrices of order 129 ... 256, gfx950.
//
// One launch per call: one workgroup of 768 or 1024 threads owns one matrix from the load to the un-permuted inverse.
// One global read and one global write per element, no workspace, the matrix index is blockIdx.x alone (64-bit
// offsets).  fp32 only: a 256 x 256 fp64 matrix is the whole vector register file of a CU.
//
// Layout: workgroup_member's (mi32_workgroup.hip) with the slab count and the columns per slab as parameters: 4 slabs
// of C = 192 / 256 column lanes.  Thread (slab h, column j) -- h = threadIdx.x / C, so a slab is C / 64 whole waves and
// every `h == hp` branch is wave-uniform -- holds the register slots h * RPT ... h * RPT + RPT - 1 of column j;
// RPT = 40 / 48 (C = 192) and 56 / 64 (C = 256) give 160 / 192 / 224 / 256 padded rows.  A slot >= n is NaN in every
// column (a NaN never wins a pivot search, and a row only ever changes itself unless it is the pivot row); a column
// >= n holds zeros, is published by no step r < n and never stores.
//
// The step is the workgroup path's, in the arithmetic of gj_sweep_step_kernel (hence the same bits as the CPU oracle):
// labels are exchanged instead of rows; the published column r and the normalised pivot row go through LDS,
// double-buffered by the parity of the step, two barriers per step; EVERY wave searches the published column
// redundantly, now up to four slots (lane, lane + 64, lane + 128, lane + 192) and four label registers per lane, ties
// to the lowest row; the slab that holds the pivot slot picks its entry with a wave-uniform switch, divides once per
// column and publishes; every slot takes a[i] = fma(-f, prn, a[i]) unless f == 0; the pivot slot is overwritten with
// prn by a second wave-uniform switch.  A zero / NaN / infinite pivot, or a non-finite input entry, flags the member
// MI32_SINGULAR.
#include <type_traits>

#include "mi32_internal.h"
#include "mi32_sweep_common.h"

namespace mi32 {

static constexpr int kWideSlabs = 4;
static constexpr int kWidePadded = 256;  // the most padded rows and column lanes: the LDS arrays' length

int wide_rows_per_thread(int n)
{
    return n <= kWorkgroupMaxOrder || n > kWideMaxOrder ? 0 : n <= 160 ? 40 : n <= 192 ? 48 : n <= 224 ? 56 : 64;
}
// column lanes per slab of the class; the workgroup is 4 slabs
static constexpr int wide_columns(int rows_per_thread) { return rows_per_thread <= 48 ? 192 : 256; }
int wide_threads(int n)
{
    const int rpt = wide_rows_per_thread(n);
    return rpt ? kWideSlabs * wide_columns(rpt) : 0;
}

// `X(i)` for i = 0 ... 63 as the cases of a switch; slots >= RPT are discarded at compile time
#define MI32_WD_CASES8(X, b) X(b + 0) X(b + 1) X(b + 2) X(b + 3) X(b + 4) X(b + 5) X(b + 6) X(b + 7)
#define MI32_WD_CASES64(X)                                                                                      \
    MI32_WD_CASES8(X, 0) MI32_WD_CASES8(X, 8) MI32_WD_CASES8(X, 16) MI32_WD_CASES8(X, 24) MI32_WD_CASES8(X, 32) \
    MI32_WD_CASES8(X, 40) MI32_WD_CASES8(X, 48) MI32_WD_CASES8(X, 56)

// a[slot] for a wave-uniform slot held in a scalar register: a tree of scalar branches around one move
template <int RPT>
__device__ __forceinline__ float wide_pick(const float (&a)[RPT], int slot)
{
    float v = 0.0f;
#define MI32_WD_PICK(i) \
    case (i):           \
        if constexpr ((i) < RPT) v = a[(i)]; \
        break;
    switch (slot) { MI32_WD_CASES64(MI32_WD_PICK) default: break; }
#undef MI32_WD_PICK
    return v;
}
template <int RPT>
__device__ __forceinline__ void wide_put(float (&a)[RPT], int slot, float v)
{
#define MI32_WD_PUT(i) \
    case (i):          \
        if constexpr ((i) < RPT) a[(i)] = v; \
        break;
    switch (slot) { MI32_WD_CASES64(MI32_WD_PUT) default: break; }
#undef MI32_WD_PUT
}

// One member from the load to the un-permuted inverse on the whole workgroup.  `in` / `out`: the member's first
// element, rows n elements apart; everything but the thread's own column is workgroup-uniform.  Every element is in
// registers before the first store (the step loop's barriers lie between).  DET: every thread also multiplies each
// step's pivot into the determinant (det_accumulate of mi32_internal.h; the pivot and the swap predicate are
// workgroup-uniform, so the accumulator lives in scalar registers), thread 0 stores it to *det_mant / *det_exp, and a
// null `out` skips the inverse's stores.
template <int C, int RPT, bool PIVOT, bool DET>
__device__ __forceinline__ void wide_member(const float *in, float *out, const int n, int *status_word,
                                            double *det_mant = nullptr, int *det_exp = nullptr)
{
    static_assert(C % 64 == 0 && C <= kWidePadded, "a slab is whole waves");
    static_assert(RPT % 8 == 0 && RPT >= 40 && RPT <= 64 && kWideSlabs * RPT <= kWidePadded, "rows per thread");
    constexpr int P = kWideSlabs * RPT;  // padded rows
    __shared__ __attribute__((aligned(32))) float s_col[2][kWidePadded];   // published column r, by step parity
    __shared__ __attribute__((aligned(32))) float s_prow[2][kWidePadded];  // normalised pivot row, by step parity
    __shared__ __attribute__((aligned(16))) int s_label[kWidePadded];      // slot -> logical row, for the store
    __shared__ int s_slot_of[kWidePadded];                                 // logical row -> slot, for the store

    const int h = __builtin_amdgcn_readfirstlane((int)threadIdx.x / C);  // wave-uniform: C is a multiple of 64
    const int j = (int)threadIdx.x - h * C;
    const int lane = threadIdx.x & 63;
    const int slot0 = h * RPT;
    const bool mine = j < n;

    float a[RPT];
    bool bad = false;  // boundary rule: a NaN / inf anywhere in the input is an invalid matrix
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
        const bool live = mine && slot0 + i < n;
        // loaded unconditionally (a dead slot reads the member's first element): the loads stay in flight together
        const float v = in[live ? (size_t)(slot0 + i) * n + j : 0];
        bad = bad || (live && v - v != 0.0f);
        a[i] = slot0 + i < n ? (mine ? v : 0.0f) : not_a_candidate(0.0f);
    }
    // this wave's copy of the labels of slots lane + 64 k (slots >= P exist in no register: never candidates)
    int lab0 = lane, lab1 = lane + 64, lab2 = lane + 128, lab3 = lane + 192;
    DetAcc det = det_start(false);
    // a non-finite input entry, seen by the thread that loaded it alone: the workgroup's accumulation never starts
    if constexpr (DET) det = det_start(__syncthreads_or(bad) != 0);

#pragma unroll 1
    for (int r = 0; r < n; ++r) {
        float *const colp = s_col[r & 1];
        float *const prowp = s_prow[r & 1];
        // a. column r: publish, then the implicit identity column takes its place
        if (j == r) {
#pragma unroll
            for (int i = 0; i < RPT; i += 4) {
                *reinterpret_cast<Vec4<float> *>(&colp[slot0 + i]) = Vec4<float>{a[i], a[i + 1], a[i + 2], a[i + 3]};
                a[i] = a[i + 1] = a[i + 2] = a[i + 3] = 0.0f;
            }
        }
        __syncthreads();
        // b. the pivot slot sp
        int sp = r;  // without pivoting the labels stay the identity
        bool swap = false;
        if constexpr (PIVOT) {
            const float none = not_a_candidate(0.0f);
            // (in bounds: 256 entries; a slot >= P is written by nobody and is no candidate)
            const float v0 = colp[lane];
            const float v1 = colp[lane + 64];
            const float v2 = lane + 128 < P ? colp[lane + 128] : none;
            const float v3 = lane + 192 < P ? colp[lane + 192] : none;
            const PivotRec<float> k0 = PivotRec<float>::make(lab0 >= r ? v0 : none, lab0);
            const PivotRec<float> k1 = PivotRec<float>::make(lab1 >= r ? v1 : none, lab1);
            const PivotRec<float> k2 = PivotRec<float>::make(lab2 >= r ? v2 : none, lab2);
            const PivotRec<float> k3 = PivotRec<float>::make(lab3 >= r ? v3 : none, lab3);
            const PivotRec<float> best =
                wave_max_rec(PivotRec<float>::best_of(PivotRec<float>::best_of(k0, k1), PivotRec<float>::best_of(k2, k3)));
            const int pl = __builtin_amdgcn_readfirstlane(best.row(r));  // the pivot's logical row; r when nothing is a candidate
            const unsigned long long m0 = __builtin_amdgcn_ballot_w64(lab0 == pl);
            const unsigned long long m1 = __builtin_amdgcn_ballot_w64(lab1 == pl);
            const unsigned long long m2 = __builtin_amdgcn_ballot_w64(lab2 == pl);
            const unsigned long long m3 = __builtin_amdgcn_ballot_w64(lab3 == pl);
            // (exactly one of the four is non-zero: the labels are a permutation of 0 ... 255)
            sp = m0 ? __builtin_ctzll(m0) : m1 ? 64 + __builtin_ctzll(m1) : m2 ? 128 + __builtin_ctzll(m2) : 192 + __builtin_ctzll(m3);
            swap = pl != r;
            // pivotElements: the two labels change places
            lab0 = lab0 == pl ? r : lab0 == r ? pl : lab0;
            lab1 = lab1 == pl ? r : lab1 == r ? pl : lab1;
            lab2 = lab2 == pl ? r : lab2 == r ? pl : lab2;
            lab3 = lab3 == pl ? r : lab3 == r ? pl : lab3;
        }
        const float piv = colp[sp];
        if constexpr (DET) det_accumulate<float, PIVOT, true>(det, piv, swap);
        bad = bad || piv == 0.0f || piv - piv != 0.0f;  // zero, NaN or infinite pivot
        const int hp = sp / RPT, lp = sp - hp * RPT;
        // c. fixRow in the slab that holds the pivot slot
        if (h == hp) prowp[j] = (j == r ? 1.0f : wide_pick<RPT>(a, lp)) / piv;
        __syncthreads();
        // d. fixColumn
        const float prn = prowp[j];
#pragma unroll
        for (int i = 0; i < RPT; i += 4) {
            const Vec4<float> f = *reinterpret_cast<const Vec4<float> *>(&colp[slot0 + i]);  // the multipliers: old a[i][r]
            a[i + 0] = (f.x != 0.0f) ? fma_t(-f.x, prn, a[i + 0]) : a[i + 0];
            a[i + 1] = (f.y != 0.0f) ? fma_t(-f.y, prn, a[i + 1]) : a[i + 1];
            a[i + 2] = (f.z != 0.0f) ? fma_t(-f.z, prn, a[i + 2]) : a[i + 2];
            a[i + 3] = (f.w != 0.0f) ? fma_t(-f.w, prn, a[i + 3]) : a[i + 3];
        }
        if (h == hp) wide_put<RPT>(a, lp, prn);  // the pivot slot takes the normalised pivot row
    }

    int oc = j;
    if constexpr (PIVOT) {
        if (threadIdx.x < 64) {
            s_label[lane] = lab0;
            s_label[lane + 64] = lab1;
            s_label[lane + 128] = lab2;
            s_label[lane + 192] = lab3;
            s_slot_of[lab0] = lane;
            s_slot_of[lab1] = lane + 64;
            s_slot_of[lab2] = lane + 128;
            s_slot_of[lab3] = lane + 192;
        }
        __syncthreads();
        oc = s_slot_of[j];
    }
    if (!mine) return;
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
                if (row < n && oc < n) out[(size_t)row * n + oc] = a[i];
            }
        }
    }
    // the status word was zeroed (MI32_OK) by the host before this launch; every writer stores the same value
    if (bad) *status_word = MI32_SINGULAR;
}

#undef MI32_WD_CASES8
#undef MI32_WD_CASES64

template <int C, int RPT, bool PIVOT>
__global__ __launch_bounds__(kWideSlabs * C) void gj_wide_kernel(const float *__restrict__ in, float *__restrict__ out,
                                                                 int n, int *__restrict__ status)
{
    const size_t mat = (size_t)blockIdx.x * (size_t)n * (size_t)n;
    wide_member<C, RPT, PIVOT, false>(in + mat, out + mat, n, status + blockIdx.x);
}

// gj_wide_kernel with the determinant: member b's pair goes to det_mant[b], det_exp[b]; a null `out`: no inverse
template <int C, int RPT, bool PIVOT>
__global__ __launch_bounds__(kWideSlabs * C) void gj_wide_det_kernel(const float *__restrict__ in, float *__restrict__ out,
                                                                     int n, int *__restrict__ status,
                                                                     double *__restrict__ det_mant, int *__restrict__ det_exp)
{
    const size_t mat = (size_t)blockIdx.x * (size_t)n * (size_t)n;
    wide_member<C, RPT, PIVOT, true>(in + mat, out ? out + mat : nullptr, n, status + blockIdx.x,
                                                            det_mant + blockIdx.x, det_exp + blockIdx.x);
}

// f(rows per thread, pivot), both as compile-time constants: the one place where a run-time pair picks a kernel
// instance.  false: no instance has that many rows per thread.
template <typename F>
static bool wide_instance(int rows_per_thread, bool pivoting, F f)
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

hipError_t wide_invert(const float *d_a, float *d_inv, int n, int batch, int *d_status, const DetOut det, hipStream_t stream,
                       Profiler *prof, bool pivoting)
{
    const int rows = wide_rows_per_thread(n);
    if (rows == 0 || batch <= 0 || !d_status || !det.valid() || (!d_inv && det.empty())) return hipErrorInvalidValue;
    ProfScope ps(prof, KC_PANEL, stream);  // pivot steps on a register-resident panel: the whole matrix
    wide_instance(rows, pivoting, [&](auto rpt, auto pivot) {
        constexpr int RPT = decltype(rpt)::value;
        constexpr int C = wide_columns(RPT);
        constexpr bool PIVOT = decltype(pivot)::value;
        const dim3 grid((unsigned)batch), block(kWideSlabs * C);
        if (det.empty())
            hipLaunchKernelGGL((gj_wide_kernel<C, RPT, PIVOT>), grid, block, 0, stream, d_a, d_inv, n, d_status);
        else
            hipLaunchKernelGGL((gj_wide_det_kernel<C, RPT, PIVOT>), grid, block, 0, stream, d_a, d_inv, n, d_status,
                               det.mant, det.exp);
    });
    return hipGetLastError();
}

}  // namespace mi32
