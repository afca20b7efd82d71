// mi32_apply.hip -- Z_b = X_b R_b for the members of a variable-size batch: applying stored block inverses, the
// per-iteration half of a block-Jacobi preconditioner (mi32_apply_device_vbatched*).  Memory-bound: every element of X
// is read once per chunk of columns and takes part in one fused multiply-add per column.
//
// The arithmetic is fixed (mi32_apply.h): per component one chain of fused multiply-adds over j ascending, from +0.
// LANE = ROW: a group of L lanes owns one member and lane i keeps the accumulators of row i, so the chain runs inside
// one lane and nothing is reduced across lanes.
//
// X goes through LDS in tiles of TJ columns (128 bytes of a row, or the whole row of a narrower class).  The group
// loads a tile with consecutive lanes on consecutive elements of a row -- scalar loads, any alignment -- and writes
// it to LDS at the odd row pitch TJ + 1, so that the lane = row reads that follow fall into 64 different banks (fp64:
// 32 lanes on 32 bank pairs).  The chunk of R (n x KC) is staged once per chunk and read as a broadcast; the groups of
// a wave sit four elements further apart than their size, which keeps their broadcasts on different banks.  The next
// tile's global loads are issued before the current tile's multiply-adds and parked in registers.
//
// L <= 64: workgroups of 256 threads hold 256 / L members, every group inside one wave: no workgroup barrier, only
// program order within the wave.  Groups of different orders share a wave; every loop runs to the wave's largest order
// nmax, and what lies past a group's own order is staged as +0 in X and as -0 in R.  The padded product is then
// exactly -0, and fma(+0, -0, acc) = (-0) + acc returns acc for EVERY acc: +0, -0 (a chain can end in -0: a negative
// product below half the smallest subnormal rounds to it), every finite value, infinities and NaN.  (+0 in both
// factors would turn a final -0 into +0.)  So the padded terms change no bit, and a lane past the order stores
// nothing.  L = 128: one workgroup of 128 threads per member; the trip count of every loop with a barrier is the
// member's, uniform by construction.
#include "mi32_apply.h"

namespace mi32 {

__device__ __forceinline__ float fma_t(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_t(double a, double b, double c) { return __builtin_fma(a, b, c); }

constexpr int apply_threads(int lanes) { return lanes > 64 ? lanes : 256; }

template <typename T, int L>
struct ApplyGeom {
    static constexpr int kThreads = apply_threads(L);
    static constexpr int kGroups = kThreads / L;
    static constexpr int kRowBytes = 128;  // of a tile's row, where the class is that wide
    static constexpr int TJ = L * (int)sizeof(T) < kRowBytes ? L : kRowBytes / (int)sizeof(T);
    static constexpr int kPitch = TJ + 1;
    static constexpr int kRows = L / TJ;  // the rows of a tile one round of loads covers
    static constexpr int KC = apply_chunk_cols(sizeof(T));
    static constexpr int kRGroup = L * KC + 4;
    static_assert(L % TJ == 0 && (kPitch & 1) == 1, "tile geometry");
};

// what one group knows of its member
template <typename T>
struct ApplyMember {
    const T *x;
    const T *r;
    T *z;
    int n, nmax, ldx, ldr, ldz;
};

// the lane's TJ elements of the tile at column j0: round t takes the rows t * kRows ... of the tile
template <typename T, int L>
__device__ __forceinline__ void apply_load_tile(const ApplyMember<T> &mb, const int j0, const int trow, const int tcol,
                                                T (&pf)[ApplyGeom<T, L>::TJ])
{
    using G = ApplyGeom<T, L>;
    const int col = j0 + tcol;
#pragma unroll
    for (int t = 0; t < G::TJ; ++t) {
        const int row = t * G::kRows + trow;
        pf[t] = (row < mb.n && col < mb.n) ? mb.x[(size_t)row * mb.ldx + col] : T(0);
    }
}

// One chunk of KCN = 1 or KC columns from column k0 on, of which the first kc are the call's.
template <typename T, int L, int KCN>
__device__ __forceinline__ void apply_chunk(const ApplyMember<T> &mb, T *xg, T *rg, const int lane, const int k0,
                                            const int kc)
{
    using G = ApplyGeom<T, L>;
    const int trow = lane / G::TJ, tcol = lane % G::TJ;
    T pf[G::TJ];
    apply_load_tile<T, L>(mb, 0, trow, tcol, pf);
    // R: element e of the chunk is r[e / KCN][k0 + e % KCN]; every load of the chunk precedes every store of it.  What
    // is not the member's is staged as MINUS zero: beside X's +0 the padded product is exactly -0 (see the top).
#pragma unroll
    for (int t = 0; t < KCN; ++t) {
        const int e = t * L + lane;
        const int j = e / KCN, k = e % KCN;
        rg[e] = (j < mb.n && k < kc) ? mb.r[(size_t)j * mb.ldr + k0 + k] : T(-0.0);
    }
    T acc[KCN];
#pragma unroll
    for (int k = 0; k < KCN; ++k) acc[k] = T(0);
    const T *xrow = xg + lane * G::kPitch;
    for (int j0 = 0; j0 < mb.nmax; j0 += G::TJ) {  // (workgroup-uniform for L = 128: nmax is the member's order)
#pragma unroll
        for (int t = 0; t < G::TJ; ++t) xg[(t * G::kRows + trow) * G::kPitch + tcol] = pf[t];
        group_sync<L>();
        if (j0 + G::TJ < mb.nmax) apply_load_tile<T, L>(mb, j0 + G::TJ, trow, tcol, pf);
        const int jn = mb.nmax - j0 < G::TJ ? mb.nmax - j0 : G::TJ;
        const T *rj = rg + j0 * KCN;
#pragma unroll 8
        for (int jj = 0; jj < jn; ++jj) {
            const T xv = xrow[jj];
#pragma unroll
            for (int k = 0; k < KCN; ++k) acc[k] = fma_t(xv, rj[jj * KCN + k], acc[k]);
        }
        group_sync<L>();  // before the tile and, in the next chunk, R are overwritten
    }
    if (lane < mb.n) {
#pragma unroll
        for (int k = 0; k < KCN; ++k)
            if (k < kc) mb.z[(size_t)lane * mb.ldz + k0 + k] = acc[k];
    }
}

// Group g of the launch takes member members[first + g] of the plan's sorted list; g is a 64-bit function of
// blockIdx.x alone.  The member pointers carry no __restrict__: a member may be applied in place.
template <typename T, int L>
__global__ __launch_bounds__(apply_threads(L)) void apply_vkernel(const ApplyArgs<T> a, const int first,
                                                                           const int count)
{
    using G = ApplyGeom<T, L>;
    __shared__ T xs[G::kThreads * G::kPitch];
    __shared__ T rs[G::kGroups * G::kRGroup];
    const int lane = threadIdx.x & (L - 1);
    const int grp = threadIdx.x / L;
    const long long g = (long long)blockIdx.x * G::kGroups + grp;
    const bool valid = g < (long long)count;
    int m = valid ? a.members[(size_t)first + (size_t)g] : 0;
    int n = valid ? a.orders[m] : 0;
    if constexpr (L >= 64) {  // the group is the wave, or the workgroup: both waves read the same member
        m = __builtin_amdgcn_readfirstlane(m);
        n = __builtin_amdgcn_readfirstlane(n);
    }
    int nmax = n;  // the largest order in the wave
    if constexpr (L < 64) {
#pragma unroll
        for (int off = L; off < 64; off <<= 1) {
            const int o = __shfl_xor(nmax, off, 64);
            nmax = o > nmax ? o : nmax;
        }
        nmax = __builtin_amdgcn_readfirstlane(nmax);
    }
    // a group past the end of the range has n = 0: it loads and stores nothing
    ApplyMember<T> mb{nullptr, nullptr, nullptr, n, nmax, n, a.nrhs, a.nrhs};
    if (valid) {
        mb.x = a.x[m];
        mb.r = a.r[m];
        mb.z = a.z[m];
        if (a.ldx) mb.ldx = a.ldx[m];
        if (a.ldr) mb.ldr = a.ldr[m];
        if (a.ldz) mb.ldz = a.ldz[m];
    }
    T *xg = xs + grp * (L * G::kPitch);
    T *rg = rs + grp * G::kRGroup;
    for (int k0 = 0; k0 < a.nrhs; k0 += G::KC) {
        const int kc = a.nrhs - k0 < G::KC ? a.nrhs - k0 : G::KC;
        // (uniform) a single column does not pay for the accumulators it leaves empty; the bits are those of the wide form
        if (kc == 1) apply_chunk<T, L, 1>(mb, xg, rg, lane, k0, kc);
        else apply_chunk<T, L, G::KC>(mb, xg, rg, lane, k0, kc);
    }
}

template <typename T, int L>
static void apply_launch_class(const ApplyArgs<T> &a, int first, int count, hipStream_t stream)
{
    using G = ApplyGeom<T, L>;
    const dim3 grid((unsigned)(((long long)count + G::kGroups - 1) / G::kGroups));
    hipLaunchKernelGGL((apply_vkernel<T, L>), grid, dim3(G::kThreads), 0, stream, a, first, count);
}

template <typename T>
hipError_t apply_vlaunch(int lanes, const ApplyArgs<T> &a, int first, int count, hipStream_t stream, Profiler *prof)
{
    if (count <= 0 || first < 0 || a.nrhs < 1 || !a.orders || !a.members || !a.x || !a.r || !a.z) return hipErrorInvalidValue;
    ProfScope ps(prof, KC_UPDATE_IN, stream);  // multiply-adds on finished data: the class of the in-block updates
    switch (lanes) {
        case 8: apply_launch_class<T, 8>(a, first, count, stream); break;
        case 16: apply_launch_class<T, 16>(a, first, count, stream); break;
        case 32: apply_launch_class<T, 32>(a, first, count, stream); break;
        case 64: apply_launch_class<T, 64>(a, first, count, stream); break;
        case 128: apply_launch_class<T, 128>(a, first, count, stream); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
template hipError_t apply_vlaunch(int, const ApplyArgs<float> &, int, int, hipStream_t, Profiler *);
template hipError_t apply_vlaunch(int, const ApplyArgs<double> &, int, int, hipStream_t, Profiler *);

}  // namespace mi32
