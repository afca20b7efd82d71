// mi32_relax.h -- the residual of the block rows of a CSR matrix and the fused block-Jacobi sweep from the stored block
// inverses (mi32_csr_block_residual_device*, mi32_csr_relax_stored_device*): what mi32_relax.hip (the kernels) and
// mi32_device.hip (the entry points) share.  The launch list is the apply call's (apply_walk): one launch per lane class
// that has members.
#pragma once
#include "mat_inv_32_relax.h"
#include "mi32_apply.h"

namespace mi32 {

// Both results are fixed bit for bit (mat_inv_32_relax.h): the residual of a row from eight partial sums over its
// entries in stored order and a three-level butterfly, the sweep as the product of mi32_apply_stored_device on the
// block's residuals and one fma with omega.  Everything here is device memory.
template <typename T>
struct RelaxArgs {
    const int *orders;           // int[batch], in the caller's member order
    const int *members;          // int[batch], the member indices in ascending order of their orders (stable)
    const void *row_ptr;         // I[N + 1], I = int32_t or int64_t by index_bytes
    const void *col;             // I[nnz]
    const T *val;                // T[nnz]
    const long long *first;      // int64[batch]: member b is the block of rows and columns first[b] ... first[b] + n_b - 1
    const unsigned char *store;  // the sweep: the store, its offsets and formats as in StoredApplyArgs
    const long long *offset;
    const int *format;
    const T *x;                  // T[N]
    const T *b;                  // T[N]
    T *xnew;                     // the sweep: T[N], written at the blocks' rows alone; null: the residual alone
    T *const *r;                 // the residual alone: member pointers, n_b elements each; null: the sweep
    T omega;
    int index_bytes;             // 4 or 8
};

// A launch takes the `count` members from `first` on of the plan's sorted list, all of one lane class (kApplyLanes):
// the sweep where a.xnew is set, the residual alone where a.r is.  hipErrorInvalidValue for a lane class or an index
// width without an instance, an empty or negative range, a null pointer, or both or neither of xnew and r.
template <typename T>
hipError_t relax_vlaunch(int lanes, const RelaxArgs<T> &a, int first, int count, hipStream_t stream, Profiler *prof);

}  // namespace mi32
