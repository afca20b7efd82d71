// mi32_stored.h -- block inverses kept in a per-member storage format (mi32_block_stats_device*,
// mi32_store_inverses_device*, mi32_apply_stored_device*): what mi32_stored.hip (the kernels) and mi32_device.hip (the
// entry points) share.  The launch list is the apply call's (apply_walk): one launch per lane class that has members.
#pragma once
#include <cstdint>
#include <cstring>

#include "mat_inv_32_stored.h"
#include "mi32_apply.h"

namespace mi32 {

// The storage formats (MI32_STORE_*): 0 the working type T, 1 IEEE float32 (T = double only), 2 IEEE float16,
// 3 bfloat16.  Narrowing is round-to-nearest-even with IEEE results; from double to a 16-bit format through float.
// Widening is exact.
constexpr int kStoreFormats = 4;
constexpr int store_elem_bytes(int format, size_t native) { return format == 0 ? (int)native : format == 1 ? 4 : 2; }

// float -> IEEE float16 bits in integer arithmetic: independent of any denormal mode, the same code on host and device
__host__ __device__ inline uint16_t f32_to_f16_bits(uint32_t u)
{
    const uint32_t sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);   // NaN
    if (a >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);  // 65520 and above, infinity included: +-inf
    if (a >= 0x38800000u) {                                   // 2^-14 and above: a normal result
        const uint32_t r = a - 0x38000000u;                   // exponent bias 127 -> 15
        return (uint16_t)(sign | ((r + 0xfffu + ((r >> 13) & 1u)) >> 13));
    }
    if (a <= 0x33000000u) return (uint16_t)sign;              // 2^-25 (a tie, to even) and below: a zero
    // a subnormal result: the 24-bit significand in units of 2^(e - 150), rounded to units of 2^-24
    const uint32_t e = a >> 23, mant = (a & 0x7fffffu) | 0x800000u, s = 126u - e;  // s = 14 ... 24
    const uint32_t half = 1u << (s - 1), rem = mant & ((1u << s) - 1u);
    uint32_t q = mant >> s;
    if (rem > half || (rem == half && (q & 1u))) ++q;         // 0x400 is the smallest normal: the right encoding
    return (uint16_t)(sign | q);
}

// float -> bfloat16 bits: the usual integer form; a NaN stays a NaN
__host__ __device__ inline uint16_t f32_to_bf16_bits(uint32_t u)
{
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// Everything below is device memory.  Members are addressed by pointer and leading dimension, statistics and the store
// in the caller's member order.
template <typename T>
struct BlockStatsArgs {
    const int *orders;   // int[batch], in the caller's member order
    const int *members;  // int[batch], the member indices in ascending order of their orders (stable)
    const T *const *a;   // member pointers, row-major, rows lda[b] elements apart
    const int *lda;      // null: orders[b]
    double *stats;       // double[3 * batch]: norm1, absmax, absmin of member b at 3 b ...
};

template <typename T>
struct StoreArgs {
    const int *orders;
    const int *members;
    const T *const *x;        // member pointers, row-major, rows ldx[b] elements apart
    const int *ldx;           // null: orders[b]
    const int *format;        // int[batch]: the storage format of member b
    const long long *offset;  // int64[batch]: the byte offset of member b in the store, a multiple of 8
    unsigned char *store;
};

template <typename T>
struct StoredApplyArgs {
    const int *orders;
    const int *members;
    const unsigned char *store;
    const long long *offset;
    const int *format;
    const T *const *r;  // R is n x nrhs, rows ldr[b] elements apart
    T *const *z;        // Z is n x nrhs, rows ldz[b] elements apart; z[b] may be r[b] with ldz[b] == ldr[b]
    const int *ldr;     // null: nrhs
    const int *ldz;     // null: nrhs
    int nrhs;
};

// A launch takes the `count` members from `first` on of the plan's sorted list, all of one lane class (kApplyLanes).
// hipErrorInvalidValue for a lane class without an instance, an empty or negative range or a null pointer.
template <typename T>
hipError_t block_stats_vlaunch(int lanes, const BlockStatsArgs<T> &a, int first, int count, hipStream_t stream,
                               Profiler *prof);
template <typename T>
hipError_t store_vlaunch(int lanes, const StoreArgs<T> &a, int first, int count, hipStream_t stream, Profiler *prof);
template <typename T>
hipError_t apply_stored_vlaunch(int lanes, const StoredApplyArgs<T> &a, int first, int count, hipStream_t stream,
                                Profiler *prof);

}  // namespace mi32
