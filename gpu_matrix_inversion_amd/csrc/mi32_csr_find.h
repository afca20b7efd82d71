// mi32_csr_find.h -- finding the block-Jacobi blocks of a CSR sparsity pattern (mi32_csr_find_blocks_device):
// supervariable agglomeration, what mi32_csr_find.hip (the kernels) and mi32_device.hip (the entry points) share.  Host
// declarations and the layout of the caller's temporary memory; integers only, no values are read.
#pragma once
#include "mat_inv_32_csr_find.h"
#include "mi32_internal.h"

namespace mi32 {

// The result is fixed (include/mat_inv_32_csr_find.h):
//   nat[i]  = i == 0, or rows i - 1 and i differ in their number of entries or in a column index, in stored order
//   run(i)  = the largest j <= i with nat[j]
//   sv[i]   = nat[i] or (i - run(i)) % max_order == 0
//   start   = sv without agglomeration; with it the orbit of row 0 under
//             next(i) = the largest p in (i, i + max_order] with (p == N or sv[p])
// Rows are taken in TILES (one workgroup of the compare kernel, one run-start summary) and CHUNKS (one workgroup of the
// orbit kernels): a chunk workgroup has kFindThreads threads with kFindPer consecutive rows each, of which the last
// kFindMaxOrder are the look-ahead into the next chunk that next() needs.
static constexpr int kFindMaxOrder = 128;
static constexpr int kFindTile = 128;
static constexpr int kFindThreads = 1024;
static constexpr int kFindPer = 4;
static constexpr int kFindWindow = kFindThreads * kFindPer;       // 4096 rows in LDS
static constexpr int kFindChunk = kFindWindow - kFindMaxOrder;    // 3968 rows owned
static constexpr int kFindTilesPerChunk = kFindChunk / kFindTile; // 31
static_assert(kFindChunk % kFindTile == 0 && kFindChunk % 4 == 0, "tiles fill a chunk; a thread's rows are one word");

// The caller's temporary memory, every region on a 16-byte boundary of a 16-byte aligned base.  Per row 2 bytes (nat and
// step), per tile 8, per chunk 8 + 128 + 4: 2.1 bytes per row.
struct FindLayout {
    long long tiles, chunks;
    size_t tile_last;   // int64[tiles]: the last row of the tile with nat, -1 for none
    size_t run_before;  // int64[chunks]: the last row before the chunk with nat, -1 for none (chunk 0 only)
    size_t exits;       // uint8[chunks][128]: for the orbit entering the chunk at row offset k, its offset in the next one
    size_t entry;       // int32[chunks]: the offset at which the orbit of row 0 enters the chunk
    size_t nat;         // uint8[chunks * kFindChunk + kFindMaxOrder]
    size_t step;        // uint8[chunks * kFindChunk]: next(i) - i
    size_t bytes;
};
inline FindLayout find_layout(long long n)
{
    const auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    FindLayout l;
    l.tiles = (n + kFindTile - 1) / kFindTile;
    l.chunks = (n + kFindChunk - 1) / kFindChunk;
    size_t at = 0;
    const auto take = [&](size_t bytes) {
        const size_t off = at;
        at = up16(at + bytes);
        return off;
    };
    l.tile_last = take((size_t)l.tiles * 8);
    l.run_before = take((size_t)l.chunks * 8);
    l.exits = take((size_t)l.chunks * kFindMaxOrder);
    l.entry = take((size_t)l.chunks * 4);
    l.nat = take((size_t)l.chunks * kFindChunk + kFindMaxOrder);
    l.step = take((size_t)l.chunks * kFindChunk);
    l.bytes = at;
    return l;
}

// the stages of a call, in launch order; agglomerate off ends after FIND_SV, which then writes the result
enum FindStage { FIND_NAT = 1, FIND_RUNS = 2, FIND_SV = 4, FIND_CHAIN = 8, FIND_MARK = 16, FIND_ALL = 31 };

struct FindArgs {
    long long n;
    const void *row_ptr;  // I[n + 1], I = int32_t or int64_t by index_bytes
    const void *col;      // I[nnz]
    int index_bytes;
    int max_order;        // 1 ... kFindMaxOrder
    int agglomerate;
    unsigned char *start; // uint8[n], every element written exactly once
    void *work;           // find_layout(n).bytes, 16-byte aligned
};

// Enqueues the stages of `stages` (FIND_ALL: the call); a stage alone is for measuring it on the work memory a whole
// call left.  The arguments are the caller's to check.
hipError_t csr_find_launch(const FindArgs &a, int stages, hipStream_t stream, Profiler *prof);

}  // namespace mi32
