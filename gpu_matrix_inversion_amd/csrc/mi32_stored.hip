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
// and the +0 / -0 padding rule) with a loader that reads 2, 4 or 8 bytes per element.  It is a restatement, not a shared
// template: sharing the body through a loader policy changed the code of the ten apply_vkernel instances, and those
// stay as they are.  The prefetch parks the RAW BITS as they were loaded, in the registers that hold the
// tile in apply_vkernel; they are widened when the tile is written to LDS, which holds T as before, so the inner loop,
// the padding rule and every bit of Z are those of apply_vkernel on the widened members.  The format is uniform per
// member, not per wave below 64 lanes: a branch per element size around the tile's loads and per format around its
// LDS writes, outside the unrolled loops.
#include <type_traits>

#include "mi32_stored.h"

namespace mi32 {

// ---- the body of apply_vkernel (mi32_apply.hip), restated around a loader Ld -------------------------------------------
__device__ __forceinline__ float stored_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double stored_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

constexpr int stored_threads(int lanes) { return lanes > 64 ? lanes : 256; }

template <typename T, int L>
struct StoredGeom {
    static constexpr int kThreads = stored_threads(L);
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
__device__ __forceinline__ void stored_chunk(const typename Ld::Member &mb, T *xg, T *rg, const int lane, const int k0,
                                            const int kc)
{
    using G = StoredGeom<T, L>;
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
            for (int k = 0; k < KCN; ++k) acc[k] = stored_fma(xv, rj[jj * KCN + k], acc[k]);
        }
        group_sync<L>();  // before the tile and, in the next chunk, R are overwritten
    }
    if (lane < mb.n) {
#pragma unroll
        for (int k = 0; k < KCN; ++k)
            if (k < kc) mb.z[(size_t)lane * mb.ldz + k0 + k] = acc[k];
    }
}

// the order of the group's member and the largest order in its wave (wave-uniform), for a group of L <= 64 lanes;
// both the member's own order where the group is the wave or the workgroup
template <int L>
__device__ __forceinline__ int stored_wave_nmax(const int n)
{
    int nmax = n;
    if constexpr (L < 64) {
#pragma unroll
        for (int off = L; off < 64; off <<= 1) {
            const int o = __shfl_xor(nmax, off, 64);
            nmax = o > nmax ? o : nmax;
        }
        nmax = __builtin_amdgcn_readfirstlane(nmax);
    }
    return nmax;
}

// every chunk of the call's columns for the group's member
template <typename T, int L, typename Ld>
__device__ __forceinline__ void stored_columns(const typename Ld::Member &mb, T *xg, T *rg, const int lane, const int nrhs)
{
    using G = StoredGeom<T, L>;
    for (int k0 = 0; k0 < nrhs; k0 += G::KC) {
        const int kc = nrhs - k0 < G::KC ? nrhs - k0 : G::KC;
        // (uniform) a single column does not pay for the accumulators it leaves empty; the bits are those of the wide form
        if (kc == 1) stored_chunk<T, L, 1, Ld>(mb, xg, rg, lane, k0, kc);
        else stored_chunk<T, L, G::KC, Ld>(mb, xg, rg, lane, k0, kc);
    }
}

// ---- what a group of L lanes (threads of the 128 class) finds of its member ---------------------------------------
template <int L>
struct StoredSlot {
    int lane, m, n;
    bool valid;
};
// Group g of the launch takes member members[first + g] of the plan's sorted list; g is a 64-bit function of
// blockIdx.x alone.  A group past the end of the range has n = 0: it loads and stores nothing.
template <int L>
__device__ __forceinline__ StoredSlot<L> stored_slot(const int *orders, const int *members, const int first, const int count)
{
    constexpr int kGroups = stored_threads(L) / L;
    StoredSlot<L> s;
    s.lane = threadIdx.x & (L - 1);
    const long long g = (long long)blockIdx.x * kGroups + threadIdx.x / L;
    s.valid = g < (long long)count;
    s.m = s.valid ? members[(size_t)first + (size_t)g] : 0;
    s.n = s.valid ? orders[s.m] : 0;
    if constexpr (L >= 64) {  // the group is the wave, or the workgroup
        s.m = __builtin_amdgcn_readfirstlane(s.m);
        s.n = __builtin_amdgcn_readfirstlane(s.n);
    }
    return s;
}

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
__global__ __launch_bounds__(stored_threads(L)) void block_stats_vkernel(const BlockStatsArgs<T> a, const int first,
                                                                        const int count)
{
    const StoredSlot<L> g = stored_slot<L>(a.orders, a.members, first, count);
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
__global__ __launch_bounds__(stored_threads(L)) void store_vkernel(const StoreArgs<T> a, const int first, const int count)
{
    const StoredSlot<L> g = stored_slot<L>(a.orders, a.members, first, count);
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

// ---- apply from the store ------------------------------------------------------------------------------------------
template <typename T>
struct StoredMember {
    const unsigned char *x;  // n x n, dense, in format fmt
    const T *r;
    T *z;
    int n, nmax, ldr, ldz, fmt;
};

// What one loaded element is parked as: the bits as they came, in the registers a tile of T takes.  For T = double
// that is a PAIR of 32-bit registers, and a 2- or 4-byte element goes into the low one alone: zero-extending it to 64
// bits would be an operation on the loaded value, i.e. a wait right behind every load.
struct RawBits32 {
    uint32_t lo;
};
struct RawBits64 {
    uint32_t lo, hi;  // hi is written and read by the 8-byte format only
};
__device__ __forceinline__ void raw_set(RawBits32 &r, const uint32_t v) { r.lo = v; }
__device__ __forceinline__ void raw_set(RawBits64 &r, const uint32_t v) { r.lo = v; }
__device__ __forceinline__ void raw_set(RawBits64 &r, const unsigned long long v)
{
    r.lo = (uint32_t)v;
    r.hi = (uint32_t)(v >> 32);
}
__device__ __forceinline__ float raw_native(const RawBits32 &r, float) { return __uint_as_float(r.lo); }
__device__ __forceinline__ double raw_native(const RawBits64 &r, double)
{
    return __longlong_as_double((long long)(((unsigned long long)r.hi << 32) | r.lo));
}

template <typename T>
struct StoredLoader {
    using Member = StoredMember<T>;
    using Raw = typename std::conditional<sizeof(T) == 8, RawBits64, RawBits32>::type;
    using Word = typename std::conditional<sizeof(T) == 8, unsigned long long, uint32_t>::type;  // a native element

    template <int L, typename E>
    static __device__ __forceinline__ void load_as(const Member &mb, const int j0, const int trow, const int tcol,
                                                   Raw (&pf)[StoredGeom<T, L>::TJ])
    {
        using G = StoredGeom<T, L>;
        using V = typename std::conditional<sizeof(E) == 8, unsigned long long, uint32_t>::type;
        const E *x = reinterpret_cast<const E *>(mb.x);
        const int col = j0 + tcol;
#pragma unroll
        for (int t = 0; t < G::TJ; ++t) {
            const int row = t * G::kRows + trow;
            raw_set(pf[t], (row < mb.n && col < mb.n) ? (V)x[row * mb.n + col] : V(0));  // all bits clear: +0 in every format
        }
    }
    template <int L>
    static __device__ __forceinline__ void load_tile(const Member &mb, const int j0, const int trow, const int tcol,
                                                     Raw (&pf)[StoredGeom<T, L>::TJ])
    {
        const int bytes = store_elem_bytes(mb.fmt, sizeof(T));
        if (bytes == 2) load_as<L, uint16_t>(mb, j0, trow, tcol, pf);
        else if (bytes == 4) load_as<L, uint32_t>(mb, j0, trow, tcol, pf);
        else load_as<L, Word>(mb, j0, trow, tcol, pf);
    }

    template <int F>
    static __device__ __forceinline__ T widen(const Raw &raw)
    {
        if constexpr (F == MI32_STORE_FLOAT16) return (T)(float)__builtin_bit_cast(_Float16, (uint16_t)raw.lo);
        else if constexpr (F == MI32_STORE_BFLOAT16) return (T)__uint_as_float(raw.lo << 16);
        else if constexpr (F == MI32_STORE_FLOAT32 && sizeof(T) == 8) return (T)__uint_as_float(raw.lo);
        else return raw_native(raw, T());
    }
    template <int L, int F>
    static __device__ __forceinline__ void write_as(T *xg, const int trow, const int tcol, const Raw (&pf)[StoredGeom<T, L>::TJ])
    {
        using G = StoredGeom<T, L>;
#pragma unroll
        for (int t = 0; t < G::TJ; ++t) xg[(t * G::kRows + trow) * G::kPitch + tcol] = widen<F>(pf[t]);
    }
    template <int L>
    static __device__ __forceinline__ void write_tile(const Member &mb, T *xg, const int trow, const int tcol,
                                                      const Raw (&pf)[StoredGeom<T, L>::TJ])
    {
        if (mb.fmt == MI32_STORE_FLOAT16) write_as<L, MI32_STORE_FLOAT16>(xg, trow, tcol, pf);
        else if (mb.fmt == MI32_STORE_BFLOAT16) write_as<L, MI32_STORE_BFLOAT16>(xg, trow, tcol, pf);
        else if (mb.fmt == MI32_STORE_FLOAT32) write_as<L, MI32_STORE_FLOAT32>(xg, trow, tcol, pf);
        else write_as<L, MI32_STORE_NATIVE>(xg, trow, tcol, pf);
    }
};

// Two waves per SIMD, as the widest apply_vkernel instances have: the loader's three element sizes must not cost the
// second wave (without the bound the fp32 64-lane instance takes 258 vector registers).
template <typename T, int L>
__global__ __launch_bounds__(stored_threads(L), 2) void apply_stored_vkernel(const StoredApplyArgs<T> a, const int first,
                                                                         const int count)
{
    using G = StoredGeom<T, L>;
    __shared__ T xs[G::kThreads * G::kPitch];
    __shared__ T rs[G::kGroups * G::kRGroup];
    const StoredSlot<L> g = stored_slot<L>(a.orders, a.members, first, count);
    const int grp = threadIdx.x / L;
    StoredMember<T> mb{nullptr, nullptr, nullptr, g.n, stored_wave_nmax<L>(g.n), a.nrhs, a.nrhs, MI32_STORE_NATIVE};
    if (g.valid) {
        mb.x = a.store + a.offset[g.m];
        mb.r = a.r[g.m];
        mb.z = a.z[g.m];
        mb.fmt = a.format[g.m];
        if (a.ldr) mb.ldr = a.ldr[g.m];
        if (a.ldz) mb.ldz = a.ldz[g.m];
    }
    if constexpr (L >= 64) mb.fmt = __builtin_amdgcn_readfirstlane(mb.fmt);  // one member per wave: scalar branches
    stored_columns<T, L, StoredLoader<T>>(mb, xs + grp * (L * G::kPitch), rs + grp * G::kRGroup, g.lane, a.nrhs);
}

// ---- launches ------------------------------------------------------------------------------------------------------
template <int L>
static dim3 stored_grid(int count)
{
    constexpr int kGroups = stored_threads(L) / L;
    return dim3((unsigned)(((long long)count + kGroups - 1) / kGroups));
}

// f(std::integral_constant<int, L>) for the lane class `lanes`; false where there is no such class
template <typename F>
static bool stored_lane_class(int lanes, const F &f)
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

template <typename T>
hipError_t block_stats_vlaunch(int lanes, const BlockStatsArgs<T> &a, int first, int count, hipStream_t stream,
                               Profiler *prof)
{
    if (count <= 0 || first < 0 || !a.orders || !a.members || !a.a || !a.stats) return hipErrorInvalidValue;
    ProfScope ps(prof, KC_UPDATE_IN, stream);  // the class of the apply launches, whose members it measures
    const bool ok = stored_lane_class(lanes, [&](auto l) {
        constexpr int L = decltype(l)::value;
        hipLaunchKernelGGL((block_stats_vkernel<T, L>), stored_grid<L>(count), dim3(stored_threads(L)), 0, stream, a, first, count);
    });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}

template <typename T>
hipError_t store_vlaunch(int lanes, const StoreArgs<T> &a, int first, int count, hipStream_t stream, Profiler *prof)
{
    if (count <= 0 || first < 0 || !a.orders || !a.members || !a.x || !a.format || !a.offset || !a.store)
        return hipErrorInvalidValue;
    ProfScope ps(prof, KC_UPDATE_IN, stream);
    const bool ok = stored_lane_class(lanes, [&](auto l) {
        constexpr int L = decltype(l)::value;
        hipLaunchKernelGGL((store_vkernel<T, L>), stored_grid<L>(count), dim3(stored_threads(L)), 0, stream, a, first, count);
    });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}

template <typename T>
hipError_t apply_stored_vlaunch(int lanes, const StoredApplyArgs<T> &a, int first, int count, hipStream_t stream,
                                Profiler *prof)
{
    if (count <= 0 || first < 0 || a.nrhs < 1 || !a.orders || !a.members || !a.store || !a.offset || !a.format || !a.r || !a.z)
        return hipErrorInvalidValue;
    ProfScope ps(prof, KC_UPDATE_IN, stream);  // multiply-adds on finished data, as the plain apply
    const bool ok = stored_lane_class(lanes, [&](auto l) {
        constexpr int L = decltype(l)::value;
        hipLaunchKernelGGL((apply_stored_vkernel<T, L>), stored_grid<L>(count), dim3(stored_threads(L)), 0, stream, a, first, count);
    });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}

template hipError_t block_stats_vlaunch(int, const BlockStatsArgs<float> &, int, int, hipStream_t, Profiler *);
template hipError_t block_stats_vlaunch(int, const BlockStatsArgs<double> &, int, int, hipStream_t, Profiler *);
template hipError_t store_vlaunch(int, const StoreArgs<float> &, int, int, hipStream_t, Profiler *);
template hipError_t store_vlaunch(int, const StoreArgs<double> &, int, int, hipStream_t, Profiler *);
template hipError_t apply_stored_vlaunch(int, const StoredApplyArgs<float> &, int, int, hipStream_t, Profiler *);
template hipError_t apply_stored_vlaunch(int, const StoredApplyArgs<double> &, int, int, hipStream_t, Profiler *);

}  // namespace mi32
