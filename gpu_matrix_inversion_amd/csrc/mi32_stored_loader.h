// mi32_stored_loader.h -- the loader that reads a member of the store (mi32_stored.h) for the product body of
// mi32_member_walk.h: what apply_stored_vkernel (mi32_stored.hip) and relax_stored_vkernel (mi32_relax.hip) share.
// Device code: no host unit includes it.
//
// The prefetch parks the RAW BITS as they were loaded, in the registers that hold the tile in apply_vkernel; they are
// widened when the tile is written to LDS, which holds T as before, so the inner loop, the padding rule and every bit
// of Z are those of apply_vkernel on the widened members.  The format is uniform per member, not per wave below 64
// lanes: a branch per element size around the tile's loads and per format around its LDS writes, outside the unrolled
// loops.
#pragma once
#include "mi32_member_walk.h"
#include "mi32_stored.h"

namespace mi32 {

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
                                                   Raw (&pf)[ApplyGeom<T, L>::TJ])
    {
        using G = ApplyGeom<T, L>;
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
                                                     Raw (&pf)[ApplyGeom<T, L>::TJ])
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
    static __device__ __forceinline__ void write_as(T *xg, const int trow, const int tcol, const Raw (&pf)[ApplyGeom<T, L>::TJ])
    {
        using G = ApplyGeom<T, L>;
#pragma unroll
        for (int t = 0; t < G::TJ; ++t) xg[(t * G::kRows + trow) * G::kPitch + tcol] = widen<F>(pf[t]);
    }
    template <int L>
    static __device__ __forceinline__ void write_tile(const Member &mb, T *xg, const int trow, const int tcol,
                                                      const Raw (&pf)[ApplyGeom<T, L>::TJ])
    {
        if (mb.fmt == MI32_STORE_FLOAT16) write_as<L, MI32_STORE_FLOAT16>(xg, trow, tcol, pf);
        else if (mb.fmt == MI32_STORE_BFLOAT16) write_as<L, MI32_STORE_BFLOAT16>(xg, trow, tcol, pf);
        else if (mb.fmt == MI32_STORE_FLOAT32) write_as<L, MI32_STORE_FLOAT32>(xg, trow, tcol, pf);
        else write_as<L, MI32_STORE_NATIVE>(xg, trow, tcol, pf);
    }
};

}  // namespace mi32
