// mi32_csr_blocks.h -- gathering square blocks of a CSR matrix into the members of a variable-size batch
// (mi32_csr_blocks_device*): what mi32_csr_blocks.hip (the kernels) and mi32_device.hip (the entry points) share.  The
// launch list is the apply call's (apply_walk): one launch per lane class that has members.
#pragma once
#include "mat_inv_32_csr.h"
#include "mi32_apply.h"

namespace mi32 {

// The result is fixed bit for bit:  out[b][i * ld + j] = the stored value of entry (first[b] + i, first[b] + j), copied;
// +0 where the CSR stores none.  Every element of every member is written exactly once, nothing else is.  Everything
// here is device memory.
template <typename T>
struct CsrBlocksArgs {
    const int *orders;       // int[batch], in the caller's member order
    const int *members;      // int[batch], the member indices in ascending order of their orders (stable)
    const void *row_ptr;     // I[N + 1], I = int32_t or int64_t by index_bytes
    const void *col;         // I[nnz]
    const T *val;            // T[nnz]
    const long long *first;  // int64[batch]: member b is the block of rows and columns first[b] ... first[b] + n_b - 1
    T *const *out;           // member pointers, row-major, rows ldout[b] elements apart
    const int *ldout;        // null: orders[b]
    int index_bytes;         // 4 or 8
};

// A launch takes the `count` members from `first` on of the plan's sorted list, all of one lane class (kApplyLanes).
// hipErrorInvalidValue for a lane class or an index width without an instance, an empty or negative range or a null
// pointer.
template <typename T>
hipError_t csr_blocks_vlaunch(int lanes, const CsrBlocksArgs<T> &a, int first, int count, hipStream_t stream,
                              Profiler *prof);

}  // namespace mi32
