// mi32_csr_find.hip -- the block-Jacobi blocks of a CSR sparsity pattern by supervariable agglomeration
// (mi32_csr_find_blocks_device): the stage in front of the gather of mi32_csr_blocks.hip.  Integers only, no values,
// no atomics, no workspace of the context: the temporary memory is the caller's (FindLayout).
//
// The result is fixed (mi32_csr_find.h).  Five launches, three without agglomeration:
//   nat    THE HOT STAGE, one pass over row_ptr and col.  A workgroup of 128 threads owns a tile of 128 rows, thread t
//          loads the range of row t (coalesced), and a group of 16 lanes takes 16 consecutive rows, four at a time: rows
//          i - 1 ... i + 3 are adjacent in col, so per round of 16 entries a lane loads one entry of each of the five
//          -- every load of the round before the first compare -- and compares neighbours.  A pair of different lengths
//          loads nothing.  Lane t keeps row t's answer, so nat is written with consecutive lanes on consecutive bytes.
//          The tile's last row with nat is its run-start summary.
//   runs   one workgroup: per chunk the maximum of its tiles' summaries, then an exclusive prefix maximum over the
//          chunks, 1024 at a time -- a natural run can span the whole matrix.
//   sv     a workgroup per chunk, four consecutive rows per thread, the chunk and 128 rows of look-ahead in LDS: the
//          prefix maximum of the nat rows gives run(i) and sv; without agglomeration that is the result.  With it, the
//          prefix maximum of the sv rows gives next(i) (sv boundaries are never further apart than max_order, so the
//          look-ahead suffices), kept as one byte per row, and twelve rounds of pointer jumping give, for each of the
//          128 rows at which the orbit of row 0 can enter the chunk, the row at which it enters the next one.
//   chain  one workgroup stages those tables in LDS, 256 chunks at a time, and one thread follows them: the one loop
//          whose iterations depend on one another, of length N / 3968, on LDS and not on global memory.
//   mark   a workgroup per chunk marks the orbit from the chunk's real entry, again by pointer jumping (a marked row
//          marks its jump target, then every jump doubles), and writes the result.
#include <cstdint>

#include "mi32_csr_find.h"
#include "mi32_member_walk.h"

namespace mi32 {

static constexpr int kNatLanes = 16;  // of a group: a row pair's entries, 16 per round
static constexpr int kNatRows = 4;    // the row pairs a group has in flight
static_assert(kFindTile % 64 == 0 && 64 % kNatLanes == 0 && kNatLanes % kNatRows == 0, "groups lie inside a wave");

// what the chunk kernels read of a call
struct FindDev {
    long long n;
    int max_order, agglomerate;
    const unsigned char *nat;
    const long long *run_before;
    unsigned char *step;
    unsigned char *exits;
    const int *entry;
    unsigned char *start;
};

template <typename I>
__global__ __launch_bounds__(kFindTile) void csr_find_nat_kernel(const I *rp, const I *col, const long long n,
                                                                 unsigned char *nat, long long *tile_last)
{
    constexpr int GL = kNatLanes, R = kNatRows;
    __shared__ int wave_last[kFindTile / 64];
    const int lane = threadIdx.x & (GL - 1);
    const int sub = (threadIdx.x & 63) / GL;  // the group inside its wave
    const long long row = (long long)blockIdx.x * kFindTile + threadIdx.x;  // lane t of a group holds its t-th row
    long long begin_l = 0, end_l = 0, before = 0;
    if (row < n) {
        begin_l = (long long)rp[row];
        end_l = (long long)rp[row + 1];
        if (lane == 0 && row > 0) before = (long long)rp[row - 1];  // where the row in front of the group begins
    }
    // b[r], len[r]: row row0 + t0 + r - 1 (an empty row past the matrix; a range that runs backwards is empty)
    long long b[R + 1], len[R + 1];
    b[0] = __shfl(before, 0, GL);
    len[0] = __shfl(begin_l, 0, GL) - b[0];
    len[0] = len[0] > 0 ? len[0] : 0;
    bool mine = false;
    for (int t0 = 0; t0 < GL; t0 += R) {
        int most = 0;
#pragma unroll
        for (int r = 1; r <= R; ++r) {
            b[r] = __shfl(begin_l, t0 + r - 1, GL);
            len[r] = __shfl(end_l, t0 + r - 1, GL) - b[r];
            len[r] = len[r] > 0 ? len[r] : 0;
            if (len[r] == len[r - 1]) {  // only a pair of equal lengths is compared
                const long long rounds = (len[r] + GL - 1) / GL;
                const int ri = rounds > 0x7fffffff ? 0x7fffffff : (int)rounds;
                most = ri > most ? ri : most;
            }
        }
        most = wave_max<GL>(most);
        bool diff[R + 1];
#pragma unroll
        for (int r = 0; r <= R; ++r) diff[r] = false;
        for (int round = 0; round < most; ++round) {  // (wave-uniform)
            const long long k = (long long)round * GL + lane;
            I v[R + 1];
#pragma unroll
            for (int r = 0; r <= R; ++r) v[r] = k < len[r] ? col[b[r] + k] : (I)-1;  // every load before the compares
#pragma unroll
            for (int r = 1; r <= R; ++r) diff[r] |= v[r] != v[r - 1];  // (past equal lengths: -1 beside -1)
        }
#pragma unroll
        for (int r = 1; r <= R; ++r) {
            const unsigned long long m = __ballot(diff[r]);
            const bool d = len[r] != len[r - 1] || ((m >> (sub * GL)) & ((1ull << GL) - 1)) != 0;
            if (lane == t0 + r - 1) mine = d;
        }
        b[0] = b[R];
        len[0] = len[R];
    }
    mine = (mine || row == 0) && row < n;
    if (row < n) nat[row] = mine ? 1 : 0;
    // the tile's last row with nat
    const int last = wave_max<1>(mine ? (int)threadIdx.x : -1);
    if ((threadIdx.x & 63) == 0) wave_last[threadIdx.x / 64] = last;
    __syncthreads();
    if (threadIdx.x == 0) {
        int m = -1;
#pragma unroll
        for (int w = 0; w < kFindTile / 64; ++w) m = wave_last[w] > m ? wave_last[w] : m;
        tile_last[blockIdx.x] = m >= 0 ? (long long)blockIdx.x * kFindTile + m : -1;
    }
}

// run_before[c] = the largest tile_last of the tiles in front of chunk c (-1: none)
__global__ __launch_bounds__(kFindThreads) void csr_find_runs_kernel(const long long *tile_last, const long long tiles,
                                                                     const long long chunks, long long *run_before)
{
    constexpr int kWaves = kFindThreads / 64;
    __shared__ long long total[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x / 64;
    long long carry = -1;
    for (long long c0 = 0; c0 < chunks; c0 += kFindThreads) {  // (uniform; the loads of a trip wait for none before)
        const long long c = c0 + threadIdx.x;
        long long v = -1;
        if (c < chunks) {
#pragma unroll
            for (int t = 0; t < kFindTilesPerChunk; ++t) {
                const long long tile = c * kFindTilesPerChunk + t;
                const long long x = tile < tiles ? tile_last[tile] : -1;
                v = x > v ? x : v;
            }
        }
        long long inc = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const long long o = __shfl_up(inc, off, 64);
            if (lane >= off) inc = o > inc ? o : inc;
        }
        long long exc = __shfl_up(inc, 1, 64);
        if (lane == 0) exc = -1;
        if (lane == 63) total[wave] = inc;
        __syncthreads();
        long long prev = carry, all = carry;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const long long x = total[w];
            if (w < wave) prev = x > prev ? x : prev;
            all = x > all ? x : all;
        }
        exc = prev > exc ? prev : exc;
        if (c < chunks) run_before[c] = exc;
        carry = all;
        __syncthreads();  // before total is written again
    }
}

// Inclusive prefix maximum over the workgroup's kFindWindow entries, thread t holding entries t * kFindPer ... in v.
__device__ __forceinline__ void window_prefix_max(int (&v)[kFindPer], int *total)
{
    constexpr int kWaves = kFindThreads / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x / 64;
#pragma unroll
    for (int k = 1; k < kFindPer; ++k) v[k] = v[k - 1] > v[k] ? v[k - 1] : v[k];
    int inc = v[kFindPer - 1];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(inc, off, 64);
        if (lane >= off) inc = o > inc ? o : inc;
    }
    int exc = __shfl_up(inc, 1, 64);
    if (lane == 0) exc = -1;
    if (lane == 63) total[wave] = inc;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const int x = total[w];
        if (w < wave) exc = x > exc ? x : exc;
    }
    __syncthreads();  // before total is written again
#pragma unroll
    for (int k = 0; k < kFindPer; ++k) v[k] = exc > v[k] ? exc : v[k];
}

// four consecutive bytes at p, of which the first `count` are the caller's: one word where that is all four, aligned
__device__ __forceinline__ void store_bytes4(unsigned char *p, const int (&v)[kFindPer], const int count)
{
    static_assert(kFindPer == 4, "one 32-bit word");
    if (count >= 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
        *reinterpret_cast<uint32_t *>(p) = (uint32_t)v[0] | (uint32_t)v[1] << 8 | (uint32_t)v[2] << 16 | (uint32_t)v[3] << 24;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < count) p[k] = (unsigned char)v[k];
    }
}

__global__ __launch_bounds__(kFindThreads) void csr_find_sv_kernel(const FindDev d)
{
    __shared__ int total[kFindThreads / 64];
    __shared__ unsigned short last[kFindWindow];  // the last boundary at or before a window row
    __shared__ unsigned short jump[kFindWindow];
    const long long c = blockIdx.x;
    const long long r0 = c * kFindChunk;
    const int l0 = threadIdx.x * kFindPer;
    const int M = d.max_order;
    const long long left = d.n - r0;  // >= 1
    // the window's rows that exist; where the matrix ends inside the window, window row `rows` is row N
    const int rows = left < kFindWindow ? (int)left : kFindWindow;
    const int own = rows < kFindChunk ? rows : kFindChunk;  // the chunk's rows

    // run(i) and sv
    const uint32_t w = *reinterpret_cast<const uint32_t *>(d.nat + r0 + l0);  // (inside the region: FindLayout)
    bool isnat[kFindPer];
    int v[kFindPer];
#pragma unroll
    for (int k = 0; k < kFindPer; ++k) {
        isnat[k] = l0 + k < rows && ((w >> (8 * k)) & 0xff) != 0;
        v[k] = isnat[k] ? l0 + k : -1;
    }
    window_prefix_max(v, total);
    const long long rb = d.run_before[c];  // -1 in chunk 0 alone, whose row 0 has nat
    const int off0 = (int)((r0 - rb) % M);
    int bnd[kFindPer];
#pragma unroll
    for (int k = 0; k < kFindPer; ++k) {
        const int l = l0 + k;
        const int dist = v[k] >= 0 ? l - v[k] : off0 + l;  // i - run(i), or something congruent to it
        const bool sv = isnat[k] || dist % M == 0;
        bnd[k] = l < rows ? sv : l == rows;
    }
    if (!d.agglomerate) {  // (uniform)
        if (l0 < own) store_bytes4(d.start + r0 + l0, bnd, own - l0);
        return;
    }

    // next(i) = the last boundary at or before min(i + M, N)
#pragma unroll
    for (int k = 0; k < kFindPer; ++k) v[k] = bnd[k] ? l0 + k : -1;
    window_prefix_max(v, total);
#pragma unroll
    for (int k = 0; k < kFindPer; ++k) last[l0 + k] = (unsigned short)v[k];
    __syncthreads();
    int nx[kFindPer], st[kFindPer];
#pragma unroll
    for (int k = 0; k < kFindPer; ++k) {
        const int l = l0 + k;
        nx[k] = l;  // the look-ahead rows and whatever lies past the matrix stay where they are
        if (l < own) {
            const int target = l + M < rows ? l + M : rows;  // <= kFindWindow - 1: own <= kFindChunk, M <= 128
            nx[k] = last[target];                            // in (l, target]: boundaries are at most M apart
        }
        st[k] = nx[k] - l;
        jump[l] = (unsigned short)nx[k];
    }
    if (l0 < kFindChunk) store_bytes4(d.step + r0 + l0, st, 4);
    // where the orbit leaves the chunk for each of the rows it can enter at: at most kFindChunk < 2^12 steps
    for (int round = 0; round < 12; ++round) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kFindPer; ++k) nx[k] = jump[jump[l0 + k]];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kFindPer; ++k) jump[l0 + k] = (unsigned short)nx[k];
    }
    __syncthreads();
    if (threadIdx.x < kFindMaxOrder) {
        const int j = jump[threadIdx.x];
        d.exits[c * kFindMaxOrder + threadIdx.x] = (unsigned char)(j >= kFindChunk ? j - kFindChunk : 0);  // (0: the last chunk)
    }
}

__global__ __launch_bounds__(256) void csr_find_chain_kernel(const unsigned char *exits, const long long chunks, int *entry)
{
    constexpr int kBatch = 256;
    __shared__ __attribute__((aligned(16))) unsigned char table[kBatch * kFindMaxOrder];
    __shared__ int carry;
    if (threadIdx.x == 0) carry = 0;
    for (long long c0 = 0; c0 < chunks; c0 += kBatch) {  // (uniform)
        const int count = chunks - c0 < kBatch ? (int)(chunks - c0) : kBatch;
        const uint4 *src = reinterpret_cast<const uint4 *>(exits + c0 * kFindMaxOrder);
        for (int i = threadIdx.x; i < count * (kFindMaxOrder / 16); i += 256) reinterpret_cast<uint4 *>(table)[i] = src[i];
        __syncthreads();
        if (threadIdx.x == 0) {
            int e = carry;
            for (int cc = 0; cc < count; ++cc) {  // the chain: each step waits for the one before, in LDS
                entry[c0 + cc] = e;
                e = table[cc * kFindMaxOrder + e];
            }
            carry = e;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kFindThreads) void csr_find_mark_kernel(const FindDev d)
{
    __shared__ unsigned short jump[kFindChunk + kFindPer];
    __shared__ unsigned char mark[kFindChunk + kFindPer];
    const long long c = blockIdx.x;
    const long long r0 = c * kFindChunk;
    const int l0 = threadIdx.x * kFindPer;
    const long long left = d.n - r0;
    const int rows = left < kFindChunk ? (int)left : kFindChunk;  // the chunk's rows; slot `rows` is "past the chunk"
    const int e = d.entry[c];
    if (l0 <= kFindChunk) {
        const uint32_t w = l0 < kFindChunk ? *reinterpret_cast<const uint32_t *>(d.step + r0 + l0) : 0;
#pragma unroll
        for (int k = 0; k < kFindPer; ++k) {
            const int l = l0 + k;
            const int j = l + (int)((w >> (8 * k)) & 0xff);
            jump[l] = (unsigned short)(l < rows && j < rows ? j : rows);
            mark[l] = l == e && l < rows;
        }
    }
    // marked: the orbit's rows less than `span` steps from the entry; jump: `span` steps ahead
    for (int span = 1; span < rows; span <<= 1) {  // (uniform)
        __syncthreads();
        int a[kFindPer], b[kFindPer];
        bool m[kFindPer];
        if (l0 < kFindChunk) {
#pragma unroll
            for (int k = 0; k < kFindPer; ++k) {
                m[k] = mark[l0 + k] != 0;
                a[k] = jump[l0 + k];
                b[k] = jump[a[k]];
            }
        }
        __syncthreads();
        if (l0 < kFindChunk) {
#pragma unroll
            for (int k = 0; k < kFindPer; ++k) {
                if (m[k]) mark[a[k]] = 1;
                jump[l0 + k] = (unsigned short)b[k];
            }
        }
    }
    __syncthreads();
    if (l0 < rows) {
        int out[kFindPer];
#pragma unroll
        for (int k = 0; k < kFindPer; ++k) out[k] = mark[l0 + k];
        store_bytes4(d.start + r0 + l0, out, rows - l0);
    }
}

hipError_t csr_find_launch(const FindArgs &a, int stages, hipStream_t stream, Profiler *prof)
{
    if (a.n < 1 || !a.row_ptr || !a.col || !a.start || !a.work) return hipErrorInvalidValue;
    if (a.index_bytes != 4 && a.index_bytes != 8) return hipErrorInvalidValue;
    if (a.max_order < 1 || a.max_order > kFindMaxOrder) return hipErrorInvalidValue;
    const FindLayout l = find_layout(a.n);
    if (l.tiles > 0x7fffffffLL) return hipErrorInvalidValue;  // a grid dimension
    unsigned char *w = static_cast<unsigned char *>(a.work);
    long long *tile_last = reinterpret_cast<long long *>(w + l.tile_last);
    long long *run_before = reinterpret_cast<long long *>(w + l.run_before);
    int *entry = reinterpret_cast<int *>(w + l.entry);
    const FindDev d{a.n, a.max_order, a.agglomerate, w + l.nat, run_before, w + l.step, w + l.exits, entry, a.start};
    const dim3 tiles((unsigned)l.tiles), chunks((unsigned)l.chunks);
    ProfScope ps(prof, KC_UPDATE_IN, stream);
    if (stages & FIND_NAT) {
        if (a.index_bytes == 4)
            hipLaunchKernelGGL(csr_find_nat_kernel<int32_t>, tiles, dim3(kFindTile), 0, stream,
                               static_cast<const int32_t *>(a.row_ptr), static_cast<const int32_t *>(a.col), a.n,
                               w + l.nat, tile_last);
        else
            hipLaunchKernelGGL(csr_find_nat_kernel<int64_t>, tiles, dim3(kFindTile), 0, stream,
                               static_cast<const int64_t *>(a.row_ptr), static_cast<const int64_t *>(a.col), a.n,
                               w + l.nat, tile_last);
    }
    if (stages & FIND_RUNS)
        hipLaunchKernelGGL(csr_find_runs_kernel, dim3(1), dim3(kFindThreads), 0, stream, tile_last, l.tiles, l.chunks,
                           run_before);
    if (stages & FIND_SV) hipLaunchKernelGGL(csr_find_sv_kernel, chunks, dim3(kFindThreads), 0, stream, d);
    if (a.agglomerate) {
        if (stages & FIND_CHAIN)
            hipLaunchKernelGGL(csr_find_chain_kernel, dim3(1), dim3(256), 0, stream, w + l.exits, l.chunks, entry);
        if (stages & FIND_MARK) hipLaunchKernelGGL(csr_find_mark_kernel, chunks, dim3(kFindThreads), 0, stream, d);
    }
    return hipGetLastError();
}

}  // namespace mi32
