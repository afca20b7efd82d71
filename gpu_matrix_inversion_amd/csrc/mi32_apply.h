// mi32_apply.h -- Z_b = X_b R_b for the members of a variable-size batch (mi32_apply_device_vbatched*): what
// mi32_apply.hip (the kernels), mi32_plan.hip (the launch list) and mi32_device.hip (the entry points) share.  Included
// by these three units and, through mi32_stored.h and mi32_csr_blocks.h, by the stored-inverse and CSR units, which walk
// the same launch list: the elimination kernels never see it.  Host declarations only: what the kernels of that list
// share is mi32_member_walk.h.
#pragma once
#include <functional>

#include "mi32_internal.h"

namespace mi32 {

// The product's arithmetic is fixed:  z[i][k] = acc after acc = +0; for j = 0 ... n-1 ascending: acc = fma(x[i][j],
// r[j][k], acc) -- one fused multiply-add per term in the element type, no term skipped.  Nothing of the layout below
// (lanes, tiles, column chunks) enters the result.
//
// A launch takes the `count` members from `first` on of the plan's sorted list, all of one lane class: a group of
// `lanes` lanes (8 / 16 / 32 / 64: 256 / lanes members per workgroup, every group inside one wave; 128: one workgroup
// per member) owns one member, lane i its row i.  The nrhs columns are walked inside the kernel in chunks of
// apply_chunk_cols.  Everything here is device memory.
template <typename T>
struct ApplyArgs {
    const int *orders;   // int[batch], in the caller's member order
    const int *members;  // int[batch], the member indices in ascending order of their orders (stable)
    const T *const *x;   // member pointers, row-major: X is n x n, rows ldx[b] elements apart
    const T *const *r;   // R is n x nrhs, rows ldr[b] elements apart
    T *const *z;         // Z is n x nrhs, rows ldz[b] elements apart; z[b] may be r[b] with ldz[b] == ldr[b]
    const int *ldx;      // null: orders[b]
    const int *ldr;      // null: nrhs
    const int *ldz;      // null: nrhs
    int nrhs;
};

static constexpr int kApplyClasses = 5;
static constexpr int kApplyLanes[kApplyClasses] = {8, 16, 32, 64, 128};
// the columns of R and Z a group holds at a time: 32 bytes of accumulators per lane
constexpr int apply_chunk_cols(size_t elem_bytes) { return elem_bytes == 8 ? 4 : 8; }

// One launch of a call: the `count` sorted members from `first` on, `lanes` per member, the columns in chunks of `cols`.
// The four ints are what mi32_vbatch_apply_launches reports per launch.
struct ApplyLaunch {
    int first, count, lanes, cols;
};
using ApplyLaunchFn = std::function<bool(const ApplyLaunch &)>;  // false ends the walk
// The launches of a call on a plan's members (class_begin as in mi32_vbatch), in the order they are enqueued: one per
// lane class that has members, whatever nrhs is.  The plan's classes 0 ... 3 are the lane classes 8 ... 64, its classes
// 4 ... 7 together the 128-thread class.  The one place the rule lives (mi32_plan.hip).
void apply_walk(const int *class_begin, size_t elem_bytes, const ApplyLaunchFn &f);

// hipErrorInvalidValue for a lane class without an instance, an empty or negative range, no columns or a null pointer
template <typename T>
hipError_t apply_vlaunch(int lanes, const ApplyArgs<T> &a, int first, int count, hipStream_t stream, Profiler *prof);

}  // namespace mi32
