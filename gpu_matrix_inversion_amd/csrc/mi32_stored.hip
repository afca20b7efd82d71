// mi32_stored.hip -- block inverses kept in the narrowest storage format that is safe for each member, the
// adaptive-precision block-Jacobi of Anzt, Dongarra, Flegar, Higham and Quintana-Orti: three kernel families over the
// plan's sorted member list, launched by the apply call's rule (apply_walk: one launch per lane class that has members,
// at most five).  None uses a workspace, a memset or atomics.
//
// BLOCK STATISTICS (block_stats_vkernel): what the choice of a format needs of a member, as three doubles -- the
// 1-norm, the largest and the smallest nonzero magnitude.  LANE = COLUMN: lane j walks the rows of column j ascending,
// so consecutive lanes read consecutive elements of a row, and the column sum is one chain of additions in double
// inside one lane; only the final max / min cross lanes.  A NaN anywhere makes all three values NaN.
//
// STORE (store_vkernel): member b's n^2 elements, narrowed to its format, row-major and dense at store + offset[b];
// consecutive lanes on consecutive elements, every element written exactly once, nothing between members.  Narrowing
// to a 16-bit format is integer arithmetic on the float's bits (mi32_stored.h): no denormal mode enters it.
//
// APPLY FROM THE STORE (apply_stored_vkernel): the body of apply_vkernel (mi32_apply.hip, whose top explains the layout
// and the +0 / -0 padding rule), shared through mi32_member_walk.h, with a loader that reads 2, 4 or 8 bytes per element.
// The prefetch parks the RAW BITS as they were loaded, in the registers that hold the tile in apply_vkernel; they are
// widened when the tile is written to LDS, which holds T as before, so the inner loop, the padding rule and every bit
// of Z are those of apply_vkernel on the widened members.  The format is uniform per member, not per wave below 64
// lanes: a branch per element size around the tile's loads and per format around its LDS writes, outside the unrolled
// loops.
#include "mi32_stored_loader.h"

namespace mi32 {

// ---- block statistics ----------------------------------------------------------------------------------------------
struct ColumnStats {
    double sum, big, small;  // the column's sum of magnitudes, its largest and its smallest nonzero magnitude
    int nan;
};
__device__ __forceinline__ void stats_merge(ColumnStats &s, const double sum, const double big, const double small,
                                            const int nan)
{
    s.sum = sum > s.sum ? sum : s.sum;
    s.big = big > s.big ? big : s.big;
    s.small = small < s.small ? small : s.small;
    s.nan |= nan;
}

template <typename T, int L>
__global__ __launch_bounds__(walk_threads(L)) void block_stats_vkernel(const BlockStatsArgs<T> a, const int first,
                                                                        const int count)
{
    const MemberSlot g = member_slot<L>(a.orders, a.members, first, count);
    ColumnStats s{0.0, 0.0, __builtin_huge_val(), 0};  // neutral: a lane past the order, a group past the range
    if (g.lane < g.n) {
        const size_t ld = a.lda ? (size_t)a.lda[g.m] : (size_t)g.n;
        const T *col = a.a[g.m] + g.lane;
#pragma unroll 4
        for (int i = 0; i < g.n; ++i) {
            const double v = __builtin_fabs((double)col[(size_t)i * ld]);
            s.sum = s.sum + v;
            s.nan |= v != v;
            s.big = v > s.big ? v : s.big;
            s.small = (v != 0.0 && v < s.small) ? v : s.small;
        }
    }
    constexpr int W = L > 64 ? 64 : L;
#pragma unroll
    for (int off = W / 2; off >= 1; off >>= 1)
        stats_merge(s, __shfl_xor(s.sum, off, 64), __shfl_xor(s.big, off, 64), __shfl_xor(s.small, off, 64),
                    __shfl_xor(s.nan, off, 64));
    if constexpr (L > 64) {  // one member per workgroup: its second wave hands its half over (workgroup-uniform)
        __shared__ double part[3];
        __shared__ int part_nan;
        if (threadIdx.x == 64) {
            part[0] = s.sum;
            part[1] = s.big;
            part[2] = s.small;
            part_nan = s.nan;
        }
        __syncthreads();
        if (threadIdx.x == 0) stats_merge(s, part[0], part[1], part[2], part_nan);
    }
    if (g.lane == 0 && g.valid) {
        const double nan = __builtin_nan("");
        double *out = a.stats + 3 * (size_t)g.m;
        out[0] = s.nan ? nan : s.sum;
        out[1] = s.nan ? nan : s.big;
        out[2] = s.nan ? nan : s.small;
    }
}

// ---- store ---------------------------------------------------------------------------------------------------------
template <typename T, int L>
__global__ __launch_bounds__(walk_threads(L)) void store_vkernel(const StoreArgs<T> a, const int first, const int count)
{
    const MemberSlot g = member_slot<L>(a.orders, a.members, first, count);
    if (!g.valid) return;
    const size_t ld = a.ldx ? (size_t)a.ldx[g.m] : (size_t)g.n;
    const T *x = a.x[g.m];
    const int f = a.format[g.m];
    unsigned char *dst = a.store + a.offset[g.m];
    const int nn = g.n * g.n;
    for (int e = g.lane; e < nn; e += L) {
        const int row = e / g.n, col = e - row * g.n;
        const T v = x[row * ld + col];
        if (f == MI32_STORE_NATIVE || (f == MI32_STORE_FLOAT32 && sizeof(T) == 4)) {
            reinterpret_cast<T *>(dst)[e] = v;
        } else if (f == MI32_STORE_FLOAT32) {
            reinterpret_cast<float *>(dst)[e] = (float)v;
        } else if (f == MI32_STORE_FLOAT16 || f == MI32_STORE_BFLOAT16) {  // from double through float: two roundings
            const uint32_t u = __float_as_uint((float)v);
            reinterpret_cast<uint16_t *>(dst)[e] = f == MI32_STORE_FLOAT16 ? f32_to_f16_bits(u) : f32_to_bf16_bits(u);
        }
    }
}

// ---- apply from the store (the loader: mi32_stored_loader.h) -------------------------------------------------------
// Two waves per SIMD, as the widest apply_vkernel instances have: the loader's three element sizes must not cost the
// second wave (without the bound the fp32 64-lane instance takes 258 vector registers).
template <typename T, int L>
__global__ __launch_bounds__(walk_threads(L), 2) void apply_stored_vkernel(const StoredApplyArgs<T> a, const int first,
                                                                         const int count)
{
    using G = ApplyGeom<T, L>;
    __shared__ T xs[G::kThreads * G::kPitch];
    __shared__ T rs[G::kGroups * G::kRGroup];
    const MemberSlot g = member_slot<L>(a.orders, a.members, first, count);
    StoredMember<T> mb{nullptr, nullptr, nullptr, g.n, wave_max<L>(g.n), a.nrhs, a.nrhs, MI32_STORE_NATIVE};
    if (g.valid) {
        mb.x = a.store + a.offset[g.m];
        mb.r = a.r[g.m];
        mb.z = a.z[g.m];
        mb.fmt = a.format[g.m];
        if (a.ldr) mb.ldr = a.ldr[g.m];
        if (a.ldz) mb.ldz = a.ldz[g.m];
    }
    if constexpr (L >= 64) mb.fmt = __builtin_amdgcn_readfirstlane(mb.fmt);  // one member per wave: scalar branches
    apply_columns<T, L, StoredLoader<T>>(mb, xs + g.grp * (L * G::kPitch), rs + g.grp * G::kRGroup, g.lane, a.nrhs);
}

// ---- launches ------------------------------------------------------------------------------------------------------
template <typename T>
hipError_t block_stats_vlaunch(int lanes, const BlockStatsArgs<T> &a, int first, int count, hipStream_t stream,
                               Profiler *prof)
{
    if (count <= 0 || first < 0 || !a.orders || !a.members || !a.a || !a.stats) return hipErrorInvalidValue;
    return member_walk_launch(lanes, [](auto l) { return block_stats_vkernel<T, decltype(l)::value>; }, a, first, count, stream, prof);
}

template <typename T>
hipError_t store_vlaunch(int lanes, const StoreArgs<T> &a, int first, int count, hipStream_t stream, Profiler *prof)
{
    if (count <= 0 || first < 0 || !a.orders || !a.members || !a.x || !a.format || !a.offset || !a.store)
        return hipErrorInvalidValue;
    return member_walk_launch(lanes, [](auto l) { return store_vkernel<T, decltype(l)::value>; }, a, first, count, stream, prof);
}

template <typename T>
hipError_t apply_stored_vlaunch(int lanes, const StoredApplyArgs<T> &a, int first, int count, hipStream_t stream,
                                Profiler *prof)
{
    if (count <= 0 || first < 0 || a.nrhs < 1 || !a.orders || !a.members || !a.store || !a.offset || !a.format || !a.r || !a.z)
        return hipErrorInvalidValue;
    return member_walk_launch(lanes, [](auto l) { return apply_stored_vkernel<T, decltype(l)::value>; }, a, first, count, stream, prof);
}

template hipError_t block_stats_vlaunch(int, const BlockStatsArgs<float> &, int, int, hipStream_t, Profiler *);
template hipError_t block_stats_vlaunch(int, const BlockStatsArgs<double> &, int, int, hipStream_t, Profiler *);
template hipError_t store_vlaunch(int, const StoreArgs<float> &, int, int, hipStream_t, Profiler *);
template hipError_t store_vlaunch(int, const StoreArgs<double> &, int, int, hipStream_t, Profiler *);
template hipError_t apply_stored_vlaunch(int, const StoredApplyArgs<float> &, int, int, hipStream_t, Profiler *);
template hipError_t apply_stored_vlaunch(int, const StoredApplyArgs<double> &, int, int, hipStream_t, Profiler *);

}  // namespace mi32
