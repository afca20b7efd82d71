// mi32_csr_blocks.hip -- the square blocks of a CSR matrix as the members of a variable-size batch
// (mi32_csr_blocks_device*): the first link of a block-Jacobi set-up, from the sparse matrix to the packed blocks that
// mi32_inv_device_vbatched inverts in place.  A copy: memory-bound, no arithmetic, no workspace, no atomics.
//
// The result is fixed (mi32_csr_blocks.h): out[b][i][j] is the stored value of (first[b] + i, first[b] + j), +0 where
// there is none.  A GROUP OWNS A BLOCK ROW: it zeroes a row buffer of its own in LDS, scans the CSR row with
// consecutive lanes on consecutive entries -- an entry whose column falls into the block is stored into the buffer at
// that column, every other one is skipped --, and writes the buffer out with consecutive lanes on consecutive
// elements.  Columns need no order, a row may be empty, and every element of the member is written once, by the one
// store of the write-out.
//
// A row is a chain of dependent memory latencies -- its range from row_ptr, then its entries, then the store -- and a
// block's rows hold tens of entries, so a group that took them one by one would wait, not move bytes.  Hence (1) the
// ranges of ALL of a group's rows are loaded up front, lane i that of the group's i-th row, and handed round by
// __shfl; (2) a group works on kRows rows at a time, each with a buffer of its own: the entries of all of them are
// loaded before the first is scattered.
//
// L <= 64: as in mi32_apply.hip a group of L lanes owns one member and walks its rows; workgroups of 256 threads hold
// 256 / L members, so that 10^6 members of order 4 are 31 250 workgroups.  Groups of different orders and rows of
// different lengths share a wave: every loop runs to the wave's largest trip count, and a group past its own does
// nothing inside.  L = 128: a member has one workgroup of 128 threads, whose two waves take its even and its odd rows;
// a wave's 64 lanes cover a row in two passes.  A group never leaves its wave, so the order of zeroing, scatter and
// read-back needs group_sync alone, never a workgroup barrier.
#include <cstdint>

#include "mi32_csr_blocks.h"
#include "mi32_member_walk.h"

namespace mi32 {

template <typename T, int L>
struct CsrGeom {
    static constexpr int kThreads = walk_threads(L);
    static constexpr int kLanes = L > 64 ? 64 : L;        // of a group: it lies inside one wave
    static constexpr int kGroups = kThreads / kLanes;
    static constexpr int kShare = L > 64 ? kGroups : 1;   // the groups that share one member, row by row
    static constexpr int kSlots = kGroups / kShare;       // members per workgroup
    static constexpr int kRows = 4;                       // the rows a group has in flight
    // a group has at most ceil(L / kShare) <= kLanes rows, one range per lane, and takes them kRows at a time
    static_assert(L <= kShare * kLanes && kLanes % kRows == 0, "one lane per row of the group");
    static_assert(kSlots == kThreads / L, "the grid of member_walk_launch");
};

// Slot s of the launch takes member members[first + s] of the plan's sorted list; s is a 64-bit function of blockIdx.x
// alone.  The lookup is this kernel's own, not member_slot: in the 128 class two groups of 64 lanes share a slot, and
// the member's order stays a per-lane value.  I: the index type of row_ptr and col.
template <typename T, typename I, int L>
__global__ __launch_bounds__(walk_threads(L)) void csr_blocks_vkernel(const CsrBlocksArgs<T> a, const int first,
                                                                     const int count)
{
    using G = CsrGeom<T, L>;
    constexpr int GL = G::kLanes, R = G::kRows;
    __shared__ T rows[G::kGroups * R * L];
    const int lane = threadIdx.x & (GL - 1);
    const int grp = threadIdx.x / GL;
    const long long slot = (long long)blockIdx.x * G::kSlots + grp / G::kShare;
    const bool valid = slot < (long long)count;
    const int m = valid ? a.members[(size_t)first + (size_t)slot] : 0;
    const int n = valid ? a.orders[m] : 0;  // a group past the end of the range has n = 0: it loads and stores nothing
    const I *rp = static_cast<const I *>(a.row_ptr);
    const I *col = static_cast<const I *>(a.col);
    long long f = 0;
    T *out = nullptr;
    size_t ld = (size_t)n;
    if (valid) {
        f = a.first[m];
        out = a.out[m];
        if (a.ldout) ld = (size_t)a.ldout[m];
    }
    T *buf = rows + grp * (R * L);
    // the group's t-th row is row row0 + t * kShare of the block; lane t holds its range (empty past the block)
    const int row0 = grp % G::kShare;
    const int mine = row0 + lane * G::kShare;
    long long begin_l = 0, end_l = 0;
    if (mine < n) {
        begin_l = (long long)rp[f + mine];
        end_l = (long long)rp[f + mine + 1];
    }
    const int trips = wave_max<GL>((n - row0 + G::kShare - 1) / G::kShare);  // (n = 0: none)
    for (int t0 = 0; t0 < trips; t0 += R) {  // (wave-uniform)
        long long k[R], end[R];
        int most = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            k[r] = __shfl(begin_l, t0 + r, GL);
            end[r] = __shfl(end_l, t0 + r, GL);
            const long long len = end[r] > k[r] ? end[r] - k[r] : 0;
            const int rounds = (int)((len + GL - 1) / GL);
            most = rounds > most ? rounds : most;
            k[r] += lane;
        }
        most = wave_max<GL>(most);
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int c = lane; c < L; c += GL) buf[r * L + c] = T(0);
        group_sync<GL>();
        for (int round = 0; round < most; ++round) {
            long long c[R];
            T v[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {  // every load of the round before its first LDS store
                c[r] = -1;
                v[r] = T(0);
                if (k[r] < end[r]) {
                    c[r] = (long long)col[k[r]] - f;
                    v[r] = a.val[k[r]];
                }
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                // inside the block's columns: 0 <= c < n as one unsigned compare (a negative c wraps far past n)
                if ((unsigned long long)c[r] < (unsigned long long)n) buf[r * L + c[r]] = v[r];
                k[r] += GL;
            }
        }
        group_sync<GL>();
        // each lane reads back the elements it zeroed: the next rows' zeroing needs no further fence
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = row0 + (t0 + r) * G::kShare;
            if (i < n) {
                T *orow = out + (size_t)i * ld;
#pragma unroll
                for (int cc = lane; cc < L; cc += GL)
                    if (cc < n) orow[cc] = buf[r * L + cc];
            }
        }
    }
}

template <typename T>
hipError_t csr_blocks_vlaunch(int lanes, const CsrBlocksArgs<T> &a, int first, int count, hipStream_t stream,
                              Profiler *prof)
{
    if (count <= 0 || first < 0 || !a.orders || !a.members || !a.row_ptr || !a.col || !a.val || !a.first || !a.out)
        return hipErrorInvalidValue;
    if (a.index_bytes != 4 && a.index_bytes != 8) return hipErrorInvalidValue;
    const auto k32 = [](auto l) { return csr_blocks_vkernel<T, int32_t, decltype(l)::value>; };
    const auto k64 = [](auto l) { return csr_blocks_vkernel<T, int64_t, decltype(l)::value>; };
    return a.index_bytes == 4 ? member_walk_launch(lanes, k32, a, first, count, stream, prof)
                              : member_walk_launch(lanes, k64, a, first, count, stream, prof);
}
template hipError_t csr_blocks_vlaunch(int, const CsrBlocksArgs<float> &, int, int, hipStream_t, Profiler *);
template hipError_t csr_blocks_vlaunch(int, const CsrBlocksArgs<double> &, int, int, hipStream_t, Profiler *);

}  // namespace mi32
