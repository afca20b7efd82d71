// mi32_wide.hip -- the wide workgroup-resident path for large batches of fp32 matrices of order 129 ... 256, gfx950.
//
// One launch per call: one workgroup of 768 or 1024 threads owns one matrix from the load to the un-permuted inverse.
// One global read and one global write per element, no workspace, the matrix index is blockIdx.x alone (64-bit
// offsets).  fp32 only: a 256 x 256 fp64 matrix is the whole vector register file of a CU.
//
// The member body is slab_member (mi32_slab.h: the layout and the step) with 4 slabs of C = 192 / 256 column lanes
// -- h = threadIdx.x / C, so a slab is C / 64 whole waves --; RPT = 40 / 48 (C = 192) and 56 / 64 (C = 256) give 160 /
// 192 / 224 / 256 padded rows, and lane l of every wave keeps the labels of slots l, l + 64, l + 128 and l + 192.  Rows
// are n elements apart on both sides; the body's row pointer, its leading dimensions and its solve columns are unused
// here.
#include "mi32_slab.h"

namespace mi32 {

static constexpr int kWideSlabs = 4;

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

template <int C, int RPT, bool PIVOT>
__global__ __launch_bounds__(kWideSlabs * C) void gj_wide_kernel(const float *__restrict__ in, float *__restrict__ out,
                                                                 int n, int *__restrict__ status)
{
    const size_t mat = (size_t)blockIdx.x * (size_t)n * (size_t)n;
    slab_member<float, kWideSlabs, C, RPT, PIVOT, false, false>(in + mat, out + mat, n, n, n, status + blockIdx.x);
}

// gj_wide_kernel with the determinant: member b's pair goes to det_mant[b], det_exp[b]; a null `out`: no inverse
template <int C, int RPT, bool PIVOT>
__global__ __launch_bounds__(kWideSlabs * C) void gj_wide_det_kernel(const float *__restrict__ in, float *__restrict__ out,
                                                                     int n, int *__restrict__ status,
                                                                     double *__restrict__ det_mant, int *__restrict__ det_exp)
{
    const size_t mat = (size_t)blockIdx.x * (size_t)n * (size_t)n;
    slab_member<float, kWideSlabs, C, RPT, PIVOT, false, true>(in + mat, out ? out + mat : nullptr, n, n, n,
                                                               status + blockIdx.x, det_mant + blockIdx.x,
                                                               det_exp + blockIdx.x);
}

hipError_t wide_invert(const float *d_a, float *d_inv, int n, int batch, int *d_status, const DetOut det, hipStream_t stream,
                       Profiler *prof, bool pivoting)
{
    const int rows = wide_rows_per_thread(n);
    if (rows == 0 || batch <= 0 || !d_status || !det.valid() || (!d_inv && det.empty())) return hipErrorInvalidValue;
    ProfScope ps(prof, KC_PANEL, stream);  // pivot steps on a register-resident panel: the whole matrix
    slab_instance(rows, pivoting, [&](auto rpt, auto pivot) {
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
