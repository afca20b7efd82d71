// mi32_det_large.hip -- the small kernels of the determinant above order kWorkgroupMaxOrder (see mi32_det_large.h):
// the input scan, the pivot gather of the blocked fp32 path, the parity of its row map, and the finish kernel that
// runs the (mantissa, exponent) recurrence over a matrix's recorded pivots.
#include "mi32_det_large.h"

namespace mi32 {

DetMem det_carve(void *base, int np, int batch, size_t elem_bytes, WsRegions *regions)
{
    WsCarver c(base, regions);
    DetMem m;
    m.wbytes = align256(sizeof(int) * (size_t)batch);
    m.flag = c.take<int>(m.wbytes, WS_RECORDS, "flag");
    m.parity = c.take<int>(m.wbytes, WS_RECORDS, "parity");
    const size_t pbytes = align256((size_t)np * elem_bytes);
    m.piv = c.take<void>(pbytes * batch, WS_VALUES, "piv");
    m.pstride = pbytes / elem_bytes;
    m.bytes = c.off;
    return m;
}
size_t det_bytes(int np, int batch, size_t elem_bytes, WsRegions *regions)
{
    return det_carve(nullptr, np, batch, elem_bytes, regions).bytes;
}

// ---- a non-finite input entry --------------------------------------------------------------------------------------
// The init kernels fold it into the status word, where it cannot be told from a bad pivot; the pair needs the
// difference.  One read of the input; every writer of flag[b] stores the same value.
static constexpr int kScanThreads = 256;
static constexpr int kScanPerThread = 8;
template <typename T>
__global__ __launch_bounds__(kScanThreads) void det_scan_kernel(const T *__restrict__ in, size_t count, int *__restrict__ flag)
{
    const int b = blockIdx.y;
    const T *a = in + (size_t)b * count;
    const size_t i0 = ((size_t)blockIdx.x * kScanPerThread) * kScanThreads + threadIdx.x;
    bool bad = false;
#pragma unroll
    for (int u = 0; u < kScanPerThread; ++u) {
        const size_t i = i0 + (size_t)u * kScanThreads;
        const T v = i < count ? a[i] : T(0);
        bad = bad || (v - v != T(0));
    }
    if (bad) flag[b] = 1;
}
template <typename T>
void launch_det_scan(const T *d_a, int n, int batch, int *flag, hipStream_t stream)
{
    const size_t count = (size_t)n * n;
    const size_t per_wg = (size_t)kScanThreads * kScanPerThread;
    hipLaunchKernelGGL((det_scan_kernel<T>), dim3((unsigned)((count + per_wg - 1) / per_wg), batch), dim3(kScanThreads), 0,
                       stream, d_a, count, flag);
}
template void launch_det_scan(const float *, int, int, int *, hipStream_t);
template void launch_det_scan(const double *, int, int, int *, hipStream_t);

// ---- blocked fp32: the pivots of one outer block ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void det_gather_kernel(const float *__restrict__ mf_all, size_t mfstride, int mf_ld,
                                                          const int *__restrict__ rowsrc, int np, int C0, int kb,
                                                          float *__restrict__ piv, size_t pstride,
                                                          const int *__restrict__ guard)
{
    const int b = blockIdx.y;
    if (matrix_given_up(guard, b)) return;
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= kb) return;
    int q = rowsrc[(size_t)b * np + C0 + m];
    q = q < 0 ? 0 : q >= np ? np - 1 : q;  // (a permutation of [0, np) unless the matrix was given up meanwhile)
    piv[(size_t)b * pstride + C0 + m] = -mf_all[(size_t)b * mfstride + (size_t)q * mf_ld + m];
}
void launch_det_gather(const float *mf, size_t mfstride, int mf_ld, const int *rowsrc, int np, int C0, int kb, float *piv,
                       size_t pstride, int batch, const int *guard, hipStream_t stream)
{
    hipLaunchKernelGGL(det_gather_kernel, dim3((kb + 255) / 256, batch), dim3(256), 0, stream, mf, mfstride, mf_ld, rowsrc,
                       np, C0, kb, piv, pstride, guard);
}

// ---- blocked fp32: the parity of the final row map -------------------------------------------------------------------
// (np - cycles) mod 2, one workgroup per matrix, the map in LDS.  Cycles are counted by pointer jumping: after round k
// nxt[i] = orig^(2^k)(i) and lab[i] = the smallest index among i, orig(i), ... orig^(2^k - 1)(i); after ceil(log2 np)
// rounds lab[i] is the smallest index of i's cycle, and the cycles are the indices with lab[i] == i.  Two arrays of np
// 16-bit indices (np <= 16384: 64 KiB); every round reads both into registers, then writes them, with a barrier in
// between.  (A first version let every index WALK its cycle until it met a smaller index: the smallest index of a
// long cycle takes about np / 2 dependent LDS round trips -- 0.1 ms at 4096 rows, as much as everything else the
// determinant adds.  A walk through global memory would be slower still.)  The number of rounds is fixed, so the
// kernel ends on any contents.
static constexpr int kParityThreads = 1024;
static constexpr int kParityPerThread = 16;  // np <= kParityThreads * kParityPerThread = 16384 (blocked_supported)
__global__ __launch_bounds__(kParityThreads) void det_parity_kernel(const int *__restrict__ orig, int np,
                                                                    int *__restrict__ parity,
                                                                    const int *__restrict__ guard)
{
    extern __shared__ int s_words[];
    unsigned short *nxt = reinterpret_cast<unsigned short *>(s_words);
    unsigned short *lab = nxt + np;
    const int b = blockIdx.x;
    if (matrix_given_up(guard, b)) return;
    const int tid = threadIdx.x;
#pragma unroll
    for (int u = 0; u < kParityPerThread; ++u) {
        const int i = tid + u * kParityThreads;
        if (i < np) {
            const int v = orig[(size_t)b * np + i];
            nxt[i] = (unsigned short)(v < 0 ? 0 : v >= np ? np - 1 : v);
            lab[i] = (unsigned short)i;
        }
    }
    __syncthreads();
    for (int span = 1; span < np; span <<= 1) {
        unsigned short nn[kParityPerThread], ll[kParityPerThread];
#pragma unroll
        for (int u = 0; u < kParityPerThread; ++u) {
            const int i = tid + u * kParityThreads;
            if (i < np) {
                const int j = nxt[i];
                const unsigned short lj = lab[j], li = lab[i];
                ll[u] = lj < li ? lj : li;
                nn[u] = nxt[j];
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < kParityPerThread; ++u) {
            const int i = tid + u * kParityThreads;
            if (i < np) {
                lab[i] = ll[u];
                nxt[i] = nn[u];
            }
        }
        __syncthreads();
    }
    int cycles = 0;
#pragma unroll
    for (int u = 0; u < kParityPerThread; ++u) {
        const int i = tid + u * kParityThreads;
        if (i < np) cycles += (lab[i] == i);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cycles += __shfl_xor(cycles, off, 64);
    __syncthreads();  // every read of the arrays is over: their first words carry the waves' counts
    if ((tid & 63) == 0) s_words[tid >> 6] = cycles;
    __syncthreads();
    if (tid == 0) {
        int total = 0;
        for (int w = 0; w < kParityThreads / 64; ++w) total += s_words[w];
        parity[b] = (np - total) & 1;
    }
}
void launch_det_parity(const int *orig, int np, int batch, int *parity, const int *guard, hipStream_t stream)
{
    const int words = np > kParityThreads / 64 ? np : kParityThreads / 64;
    hipLaunchKernelGGL(det_parity_kernel, dim3(batch), dim3(kParityThreads), (size_t)words * sizeof(int), stream, orig, np,
                       parity, guard);
}

// ---- the recurrence ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ float det_readlane(float v, int lane)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
__device__ __forceinline__ double det_readlane(double v, int lane)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane),
                            __builtin_amdgcn_readlane(__double2loint(v), lane));
}
// One wave per matrix.  The lanes load 64 pivots at a time; the steps are then taken in order, one after the other,
// with det_accumulate -- the pair is DEFINED by this serial chain (mat_inv_32_c.h), it is not reassociated.  The chain
// ends at the first bad pivot.  The exchanges are applied at the end as one parity (mi32_det_large.h, fact 1).
template <typename T, bool PIVOT>
__global__ __launch_bounds__(64) void det_finish_kernel(const T *__restrict__ piv_all, size_t pstride, int first, int n,
                                                         const int *__restrict__ parity, const int *__restrict__ flag,
                                                         const int *__restrict__ status, double *__restrict__ mant,
                                                         int *__restrict__ exp)
{
    const int b = blockIdx.x;
    const int lane = threadIdx.x;
    const T *piv = piv_all + (size_t)b * pstride + first;
    const bool input_bad = __builtin_amdgcn_readfirstlane(flag[b]) != 0;
    const int st = __builtin_amdgcn_readfirstlane(status[b]);
    // det_accumulate (mi32_internal.h) with swap = false, taken apart so that only what depends on the running
    // mantissa stays on the serial chain: the pivots' own frexp -- (pm, pe) -- and the bad-pivot test are done for 64
    // pivots at once, one per lane; a step is then prod = m * pm, m = frexp_mant(prod), e += pe + frexp_exp(prod), the
    // same IEEE operations on the same operands.  Every lane carries the same (m, e).
    double m = 1.0;
    int e = 0;
    bool flagged = false;
    if (!input_bad && st != MI32_RUNTIME_ERROR) {
        for (int base = 0; base < n; base += 64) {
            const int cnt = (n - base < 64) ? n - base : 64;
            const T v = (lane < cnt) ? piv[base + lane] : T(1);
            const bool bad = pivot_unusable(v);
            const double pd = (double)v;                  // exact
            const double pm = __builtin_amdgcn_frexp_mant(pd);
            const int pe = __builtin_amdgcn_frexp_exp(pd);
            const unsigned long long badmask = __ballot(bad);
            const int good = badmask ? __ffsll((long long)badmask) - 1 : cnt;  // steps in front of the first bad pivot
            if (good == 64) {  // a whole chunk: the same steps unrolled, the lane reads off the chain
#pragma unroll
                for (int k = 0; k < 64; ++k) {
                    const double prod = m * det_readlane(pm, k);
                    m = __builtin_amdgcn_frexp_mant(prod);
                    e += __builtin_amdgcn_readlane(pe, k) + __builtin_amdgcn_frexp_exp(prod);
                }
            } else {
                for (int k = 0; k < good; ++k) {
                    const double prod = m * det_readlane(pm, k);  // in +-[0.25, 1): never under- or overflows
                    m = __builtin_amdgcn_frexp_mant(prod);
                    e += __builtin_amdgcn_readlane(pe, k) + __builtin_amdgcn_frexp_exp(prod);
                }
            }
            if (badmask) {  // the step that flags the member ends the accumulation
                m = (PIVOT && det_readlane(v, good) == T(0)) ? 0.0 : __builtin_nan("");
                e = 0;
                flagged = true;
                break;
            }
        }
    }
    if (input_bad || st == MI32_RUNTIME_ERROR || (!flagged && st != MI32_OK)) {
        m = __builtin_nan("");
        e = 0;
    } else if (!flagged && (__builtin_amdgcn_readfirstlane(parity[b]) & 1)) {
        m = -m;
    }
    if (lane == 0) {
        mant[b] = m;
        exp[b] = e;
    }
}
template <typename T>
void launch_det_finish(const T *piv, size_t pstride, int first, int n, const int *parity, const int *flag,
                       const int *status, bool pivoting, DetOut det, int batch, hipStream_t stream)
{
    if (pivoting)
        hipLaunchKernelGGL((det_finish_kernel<T, true>), dim3(batch), dim3(64), 0, stream, piv, pstride, first, n, parity,
                           flag, status, det.mant, det.exp);
    else
        hipLaunchKernelGGL((det_finish_kernel<T, false>), dim3(batch), dim3(64), 0, stream, piv, pstride, first, n, parity,
                           flag, status, det.mant, det.exp);
}
template void launch_det_finish(const float *, size_t, int, int, const int *, const int *, const int *, bool, DetOut, int,
                                hipStream_t);
template void launch_det_finish(const double *, size_t, int, int, const int *, const int *, const int *, bool, DetOut, int,
                                hipStream_t);

}  // namespace mi32
