// mi32_workgroup.hip -- the workgroup-resident path for large batches of matrices of order 65 ... 128, gfx950.
//
// One launch per call: one workgroup of 256 threads owns one matrix from the load to the un-permuted inverse.  One
// global read and one global write per element, no workspace, the matrix index is blockIdx.x alone (64-bit offsets).
//
// The member body is slab_member (mi32_slab.h: the layout and the step) with 2 slabs of 128 column lanes -- j =
// threadIdx.x & 127, h = threadIdx.x >> 7, so a slab is two whole waves --; RPT = 40 / 48 / 56 / 64 gives 80 / 96 /
// 112 / 128 padded rows, and lane l of every wave keeps the labels of slots l and l + 64.
//
// gj_workgroup_vkernel is the same body for a variable-size batch (mi32_inv_device_vbatched): the workgroup looks up
// its member's order, pointers and leading dimensions from blockIdx.x.
#include "mi32_slab.h"

namespace mi32 {

static constexpr int kWorkgroupThreads = 256;
static constexpr int kWorkgroupSlabs = 2;
static constexpr int kWorkgroupColumns = 128;  // column lanes per slab; also the most padded rows (2 x 64)

int workgroup_rows_per_thread(int n)
{
    return n <= kResidentMaxOrder || n > kWorkgroupMaxOrder ? 0 : n <= 80 ? 40 : n <= 96 ? 48 : n <= 112 ? 56 : 64;
}

int workgroup_solve_rows_per_thread(int n)
{
    return n < 1 || n >= kWorkgroupMaxOrder ? 0 : n <= 80 ? 40 : workgroup_rows_per_thread(n);
}

template <typename T, int RPT, bool PIVOT>
__global__ __launch_bounds__(kWorkgroupThreads) void gj_workgroup_kernel(const T *__restrict__ in, T *__restrict__ out,
                                                                         int n, int *__restrict__ status)
{
    const size_t mat = (size_t)blockIdx.x * (size_t)n * (size_t)n;
    slab_member<T, kWorkgroupSlabs, kWorkgroupColumns, RPT, PIVOT, false, false>(in + mat, out + mat, n, n, n,
                                                                                  status + blockIdx.x);
}

// gj_workgroup_kernel with the determinant: member b's pair goes to det_mant[b], det_exp[b]; a null `out`: no inverse
template <typename T, int RPT, bool PIVOT>
__global__ __launch_bounds__(kWorkgroupThreads) void gj_workgroup_det_kernel(const T *__restrict__ in, T *__restrict__ out,
                                                                             int n, int *__restrict__ status,
                                                                             double *__restrict__ det_mant,
                                                                             int *__restrict__ det_exp)
{
    const size_t mat = (size_t)blockIdx.x * (size_t)n * (size_t)n;
    slab_member<T, kWorkgroupSlabs, kWorkgroupColumns, RPT, PIVOT, false, true>(
        in + mat, out ? out + mat : nullptr, n, n, n, status + blockIdx.x, det_mant + blockIdx.x, det_exp + blockIdx.x);
}

// A X = B: workgroup m of the launch takes member m and the columns col0 ... col0 + cols - 1 of its B.  B and X carry
// no __restrict__: X may be B (every element is in registers before the first store).
template <typename T, int RPT, bool PIVOT>
__global__ __launch_bounds__(kWorkgroupThreads) void gj_workgroup_solve_kernel(const SolveArgs<T> s)
{
    const size_t m = blockIdx.x;
    const size_t at = m * (size_t)s.n * (size_t)s.nrhs + (size_t)s.col0;
    slab_member<T, kWorkgroupSlabs, kWorkgroupColumns, RPT, PIVOT, false, false, true>(
        s.a + m * (size_t)s.n * (size_t)s.n, s.x + at, s.n, s.n, s.nrhs, s.status + m, nullptr, nullptr, s.b + at,
        s.nrhs, s.cols);
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
    slab_member<T, kWorkgroupSlabs, kWorkgroupColumns, RPT, PIVOT, (RPT >= 56), false>(v.a[s.m], v.inv[s.m], s.n, s.lda,
                                                                                        s.ldo, v.status + s.m);
}

// gj_workgroup_vkernel with the determinant, which lands at the caller's member index like the status word; d.v.inv may
// be null (determinant only)
template <typename T, int RPT, bool PIVOT>
__global__ __launch_bounds__(kWorkgroupThreads) void gj_workgroup_det_vkernel(const VbatchDetArgs<T> d, const int first)
{
    const WorkgroupSlot s = workgroup_slot(d.v, first);
    slab_member<T, kWorkgroupSlabs, kWorkgroupColumns, RPT, PIVOT, (RPT >= 56), true>(
        d.v.a[s.m], d.v.inv ? d.v.inv[s.m] : nullptr, s.n, s.lda, s.ldo, d.v.status + s.m, d.det_mant + s.m,
        d.det_exp + s.m);
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
    slab_member<T, kWorkgroupSlabs, kWorkgroupColumns, RPT, PIVOT, false, false, true>(
        v.a[s.m], v.x[s.m] + v.col0, s.n, s.lda, s.ldx, v.status + s.m, nullptr, nullptr, v.b[s.m] + v.col0, s.ldb,
        v.cols);
}

template <typename T>
hipError_t workgroup_invert(const T *d_a, T *d_inv, int n, int batch, int *d_status, const DetOut det, hipStream_t stream,
                            Profiler *prof, bool pivoting)
{
    const int rows = workgroup_rows_per_thread(n);
    if (rows == 0 || batch <= 0 || !d_status || !det.valid() || (!d_inv && det.empty())) return hipErrorInvalidValue;
    ProfScope ps(prof, KC_PANEL, stream);  // pivot steps on a register-resident panel: the whole matrix
    slab_instance(rows, pivoting, [&](auto rpt, auto pivot) {
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
    const bool found = slab_instance(rows_per_thread, pivoting, [&](auto rpt, auto pivot) {
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
    slab_instance(rows, pivoting, [&](auto rpt, auto pivot) {
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
    const bool found = slab_instance(rows_per_thread, pivoting, [&](auto rpt, auto pivot) {
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
