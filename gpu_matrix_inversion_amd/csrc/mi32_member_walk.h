// mi32_member_walk.h -- what the kernels that walk a plan's sorted member list share, and their launchers: mi32_apply.hip,
// mi32_stored.hip, mi32_csr_blocks.hip and mi32_relax.hip, one launch per lane class that has members (apply_walk).
// Device code and its launch layer: no host unit includes it.  First the layer every such kernel uses -- the threads rule, the fence inside a
// group, the group-to-member lookup, the wave-wide maximum, the lane-class dispatch and the launch --, then the body of
// the product Z = X R around a loader (mi32_apply.hip, whose top explains the layout and the +0 / -0 padding rule).
#pragma once
#include <type_traits>

#include "mi32_apply.h"

namespace mi32 {

// 8 / 16 / 32 / 64 lanes per member: workgroups of 256 threads; 128: one workgroup per member
constexpr int walk_threads(int lanes) { return lanes > 64 ? lanes : 256; }

// LDS written by one lane of a group of L lanes is read by another
template <int L>
__device__ __forceinline__ void group_sync()
{
    if constexpr (L > 64) {
        __syncthreads();
    } else {  // the group lies inside one wave: program order, which the compiler must keep
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// what a group of L lanes (the workgroup of the 128 class) finds of its member
struct MemberSlot {
    int lane, grp, m, n;
    bool valid;
};
// Group g of the launch takes member members[first + g] of the plan's sorted list; g is a 64-bit function of
// blockIdx.x alone.  A group past the end of the range has n = 0: it loads and stores nothing.
template <int L>
__device__ __forceinline__ MemberSlot member_slot(const int *orders, const int *members, const int first, const int count)
{
    constexpr int kGroups = walk_threads(L) / L;
    MemberSlot s;
    s.lane = threadIdx.x & (L - 1);
    s.grp = threadIdx.x / L;
    const long long g = (long long)blockIdx.x * kGroups + threadIdx.x / L;
    s.valid = g < (long long)count;
    s.m = s.valid ? members[(size_t)first + (size_t)g] : 0;
    s.n = s.valid ? orders[s.m] : 0;
    if constexpr (L >= 64) {  // the group is the wave, or the workgroup: both waves read the same member
        s.m = __builtin_amdgcn_readfirstlane(s.m);
        s.n = __builtin_amdgcn_readfirstlane(s.n);
    }
    return s;
}

// the largest value among a wave's groups of GL lanes, wave-uniform
template <int GL>
__device__ __forceinline__ int wave_max(int v)
{
#pragma unroll
    for (int off = GL; off < 64; off <<= 1) {
        const int o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return __builtin_amdgcn_readfirstlane(v);
}

// f(std::integral_constant<int, L>) for the lane class `lanes`; false where there is no such class
template <typename F>
static bool lane_class(int lanes, const F &f)
{
    switch (lanes) {
        case 8: f(std::integral_constant<int, 8>()); return true;
        case 16: f(std::integral_constant<int, 16>()); return true;
        case 32: f(std::integral_constant<int, 32>()); return true;
        case 64: f(std::integral_constant<int, 64>()); return true;
        case 128: f(std::integral_constant<int, 128>()); return true;
        default: return false;
    }
}

// One launch: kernel_of(std::integral_constant<int, L>) is the instance for the lane class, a kernel (args, first, count)
// over the `count` sorted members from `first` on, walk_threads(L) / L of them per workgroup.  Profiling class: multiply-
// adds and copies on finished data, that of the in-block updates.  hipErrorInvalidValue for a class without an instance.
template <typename Args, typename K>
static hipError_t member_walk_launch(int lanes, const K &kernel_of, const Args &a, int first, int count, hipStream_t stream,
                                     Profiler *prof)
{
    ProfScope ps(prof, KC_UPDATE_IN, stream);
    const bool ok = lane_class(lanes, [&](auto l) {
        constexpr int L = decltype(l)::value;
        constexpr int kSlots = walk_threads(L) / L;
        const dim3 grid((unsigned)(((long long)count + kSlots - 1) / kSlots));
        hipLaunchKernelGGL(kernel_of(l), grid, dim3(walk_threads(L)), 0, stream, a, first, count);
    });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}

// ---- Z = X R for the group's member, around a loader Ld -------------------------------------------------------------
// Ld::Member: x as the loader reads it, r, z, n, nmax (the largest order in the wave), ldr, ldz.  Ld::Raw: what one
// loaded element of X is parked as until its tile is written to LDS.  Ld::load_tile<L>(mb, j0, trow, tcol, pf): the
// lane's TJ elements of the tile at column j0, round t the rows t * kRows ... of the tile, +0 past the member's order.
// Ld::write_tile<L>(mb, xg, trow, tcol, pf): the same elements as T into the group's tile.
__device__ __forceinline__ float fma_t(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_t(double a, double b, double c) { return __builtin_fma(a, b, c); }

template <typename T, int L>
struct ApplyGeom {
    static constexpr int kThreads = walk_threads(L);
    static constexpr int kGroups = kThreads / L;
    static constexpr int kRowBytes = 128;  // of a tile's row, where the class is that wide
    static constexpr int TJ = L * (int)sizeof(T) < kRowBytes ? L : kRowBytes / (int)sizeof(T);
    static constexpr int kPitch = TJ + 1;
    static constexpr int kRows = L / TJ;  // the rows of a tile one round of loads covers
    static constexpr int KC = apply_chunk_cols(sizeof(T));
    static constexpr int kRGroup = L * KC + 4;
    static_assert(L % TJ == 0 && (kPitch & 1) == 1, "tile geometry");
};

// One chunk of KCN = 1 or KC columns from column k0 on, of which the first kc are the call's.
template <typename T, int L, int KCN, typename Ld>
__device__ __forceinline__ void apply_chunk(const typename Ld::Member &mb, T *xg, T *rg, const int lane, const int k0,
                                            const int kc)
{
    using G = ApplyGeom<T, L>;
    const int trow = lane / G::TJ, tcol = lane % G::TJ;
    typename Ld::Raw pf[G::TJ];
    Ld::template load_tile<L>(mb, 0, trow, tcol, pf);
    // R: element e of the chunk is r[e / KCN][k0 + e % KCN]; every load of the chunk precedes every store of it.  What
    // is not the member's is staged as MINUS zero: beside X's +0 the padded product is exactly -0 (mi32_apply.hip).
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
        Ld::template write_tile<L>(mb, xg, trow, tcol, pf);
        group_sync<L>();
        if (j0 + G::TJ < mb.nmax) Ld::template load_tile<L>(mb, j0 + G::TJ, trow, tcol, pf);
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

// every chunk of the call's columns for the group's member
template <typename T, int L, typename Ld>
__device__ __forceinline__ void apply_columns(const typename Ld::Member &mb, T *xg, T *rg, const int lane, const int nrhs)
{
    using G = ApplyGeom<T, L>;
    for (int k0 = 0; k0 < nrhs; k0 += G::KC) {
        const int kc = nrhs - k0 < G::KC ? nrhs - k0 : G::KC;
        // (uniform) a single column does not pay for the accumulators it leaves empty; the bits are those of the wide form
        if (kc == 1) apply_chunk<T, L, 1, Ld>(mb, xg, rg, lane, k0, kc);
        else apply_chunk<T, L, G::KC, Ld>(mb, xg, rg, lane, k0, kc);
    }
}

}  // namespace mi32
