// mi32_dpp.h -- cross-lane helpers of the blocked fp32 path (gfx950 only): the DPP wave reduction of the panel's pivot
// search, v_readlane broadcasts, and the DPP row helpers with the cases of their self-test.
#pragma once
#include <hip/hip_runtime.h>
#include <utility>

namespace mi32 {

// ---- wave-level arg-max helpers (DPP, no LDS traffic) ----------------------------
// Canonical gfx9 wave64 reduction: quad_perm x2, row_half_mirror, row_mirror, then
// row_bcast15 / row_bcast31 fold the four rows; lane 63 ends up with the total.  Each stage
// is ONE instruction (v_max_u32 / v_min_u32 with a DPP source); hipcc's update_dpp builtin
// emits v_mov_dpp + op + copy per stage, and this chain sits on the critical path of every
// pivot step.  The s_nop covers the VALU-write -> DPP-read hazard (2 wait states), which the
// compiler does not pad inside an asm statement.
#define MI32_DPP_REDUCE(OP, V)                                                        \
    asm volatile("s_nop 1\n\t" OP " %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t" \
                 "s_nop 1\n\t" OP " %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t" \
                 "s_nop 1\n\t" OP " %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"     \
                 "s_nop 1\n\t" OP " %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf\n\t"          \
                 "s_nop 1\n\t" OP " %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"        \
                 "s_nop 1\n\t" OP " %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"        \
                 "s_nop 1"                                                                          \
                 : "+v"(V))
__device__ __forceinline__ unsigned wave_max_u32(unsigned v)
{
    MI32_DPP_REDUCE("v_max_u32_dpp", v);
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ float lane_bcast(float v, int srclane)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), srclane));
}

// ---- a wave-uniform row of 16 floats in ONE register (entry c in lane c of every row of 16 lanes), used through a
// DPP source: row_newbcast:c = "lane c of my own row of 16".  Correct on gfx950 -- mi32_debug_dpp_selftest below is the
// proof -- but NOT used by the panel step: an fp32 FMA with a DPP source issues at two thirds of the plain rate
// (tools/valu_peak.hip), which cost the 4-rows-per-lane panels 4 us per launch.
// Both forms read the row register from OTHER lanes: full EXEC only (a disabled source lane delivers no data),
// row_mask / bank_mask 0xf, and no VALU write of the row register in the two instructions before.
//   row_fmac<C>:   dst = fma(row[C], -f, dst)  -- the single-rounding FMA of __builtin_fmaf(-f, row[C], dst)
//   row_select<C>: lane == pick ? row[C] : old
template <int C>
__device__ __forceinline__ void row_fmac(float &dst, float row, float f)
{
    static_assert(C >= 0 && C < 16, "row_newbcast addresses one row of 16 lanes");
    asm volatile("v_fmac_f32_dpp %0, %1, -%2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
                 : "+v"(dst) : "v"(row), "v"(f), "n"(C));
}
template <int C>
__device__ __forceinline__ float row_select(float old, float row, int lane, int pick)
{
    static_assert(C >= 0 && C < 16, "row_newbcast addresses one row of 16 lanes");
    asm volatile("v_cmp_ne_u32 vcc, %3, %2\n\t"
                 "v_cndmask_b32_dpp %0, %1, %0, vcc row_newbcast:%4 row_mask:0xf bank_mask:0xf"
                 : "+v"(old) : "v"(row), "v"(lane), "s"(pick), "n"(C) : "vcc");
    return old;
}

// The self-test: one wave per case, in[case][3][64] = {row, f, acc} words; out[case][16][4][64] = for every C:
// row_fmac, __builtin_fmaf on the entry fetched with ds_bpermute, row_select, the same select in plain C++.
// Words 0 / 1 and 2 / 3 must agree bit for bit.
template <int C>
__device__ __forceinline__ void dpp_selftest_case(float row, float f, float acc, int lane, int pick, unsigned *out)
{
    const float rc = __int_as_float(__builtin_amdgcn_ds_bpermute(((lane & ~15) + C) * 4, __float_as_int(row)));
    float d = acc;
    row_fmac<C>(d, row, f);
    const int pk = (pick + 5 * C) & 63;
    out[(C * 4 + 0) * 64 + lane] = __float_as_uint(d);
    out[(C * 4 + 1) * 64 + lane] = __float_as_uint(__builtin_fmaf(-f, rc, acc));
    out[(C * 4 + 2) * 64 + lane] = __float_as_uint(row_select<C>(acc, row, lane, pk));
    out[(C * 4 + 3) * 64 + lane] = __float_as_uint(lane == pk ? rc : acc);
}
template <int... Cs>
__device__ __forceinline__ void dpp_selftest_cases(float row, float f, float acc, int lane, int pick, unsigned *out,
                                                   std::integer_sequence<int, Cs...>)
{
    (dpp_selftest_case<Cs>(row, f, acc, lane, pick, out), ...);
}

}  // namespace mi32
