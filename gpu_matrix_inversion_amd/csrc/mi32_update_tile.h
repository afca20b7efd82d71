// mi32_update_tile.h -- the 64-column tiles that ride in the sub-panel launches of the blocked fp32 path (gfx950 only):
// update(t) of the block's own columns on the fp32 matrix cores and strip(t) of the columns outside the block.
#pragma once
#include "mi32_blocked_internal.h"
#include "mi32_strip.h"

namespace mi32 {

// One pivot step of a row that is not a candidate, for the in-block update tiles: the row's BK panel entries
// are spread over the 4 threads of a quad (BK/4 consecutive columns each); its current entry in column R
// lives in thread R / (BK/4) and is broadcast with one quad_perm DPP move.  That entry is the row's multiplier of
// the step (fm: kept by the thread that owns column R).
template <int BK, int R>
__device__ __forceinline__ void above_rows_step(float (&v)[BK / 4], float (&fm)[BK / 4], const float *s_prn, int q4)
{
    constexpr int CPT = BK / 4;
    constexpr int kQuad = (R / CPT) * 0x55;  // quad_perm:[q,q,q,q]
    const float f = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v[R % CPT]), kQuad, 0xf, 0xf, false));
    fm[R % CPT] = (q4 == R / CPT) ? f : fm[R % CPT];
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
        const int c = q4 * CPT + j;
        const float base = (c == R) ? 0.0f : v[j];
        v[j] = __builtin_fmaf(-f, s_prn[R * BK + c], base);
    }
}
template <int BK, int... Rs>
__device__ __forceinline__ void above_rows_steps(float (&v)[BK / 4], float (&fm)[BK / 4], const float *s_prn, int q4,
                                                 std::integer_sequence<int, Rs...>)
{
    (above_rows_step<BK, Rs>(v, fm, s_prn, q4), ...);
}

// Step R of a row that WAS in a one-workgroup panel, which leaves the row's entries in the sub-panel's own columns
// c <= R to the update tiles (panel_step): what fixColumn makes of them, from the row's multiplier of the step
// (known up front: Mt) and the normalised pivot row.  Column R holds the identity column's 0 when its step runs;
// the pivot row of the step (ps == R) takes the normalised row itself.  A column c > R is not touched: v[j] is
// still the 0 it started from when step c reaches it.  The same fmaf, operands and order as the full panel step.
template <int BK, int R>
__device__ __forceinline__ void panel_rows_step(float (&v)[BK / 4], const float (&fm)[BK / 4], const float *s_prn,
                                                int q4, int ps)
{
    constexpr int CPT = BK / 4;
    constexpr int kQuad = (R / CPT) * 0x55;  // quad_perm:[q,q,q,q]
    const float f = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(fm[R % CPT]), kQuad, 0xf, 0xf, false));
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
        const int c = q4 * CPT + j;
        const float p = s_prn[R * BK + c];
        const float t = (ps == R) ? p : __builtin_fmaf(-f, p, v[j]);
        v[j] = (c <= R) ? t : v[j];
    }
}
template <int BK, int... Rs>
__device__ __forceinline__ void panel_rows_steps(float (&v)[BK / 4], const float (&fm)[BK / 4], const float *s_prn,
                                                 int q4, int ps, std::integer_sequence<int, Rs...>)
{
    (panel_rows_step<BK, Rs>(v, fm, s_prn, q4, ps), ...);
}

// ---- update(t): the in-block rank-W update on the fp32 matrix cores ---------------
// For the columns j of the block that are not sub-panel t's own, 64 x 64 tiles, 256 threads = 4 waves in a 2x2
// arrangement per tile (NG tiles per workgroup), one 32x32 MFMA tile per wave:
//   strip   : the tile's 64 columns of the W pivot rows of t run the W steps (strip_step): u_m[j] and the pivot
//             rows' new values;
//   update  : y[i][j] = x[map[i]][j] - sum_m f_m[i] * u_m[j] for every other row, ONE accumulation chain per output
//             element starting from the old value, m ascending (v_mfma_f32_32x32x2_f32 with the old value as its
//             C operand is that fmaf chain): exactly the operations the reference's step loop applies to the
//             element, in its order (mat_inv_32.cpp:28-38,317-362) -- bit for bit oracle/gj_oracle.c's
//             gjo_matrix_inv_32_inplace.
// The column-tile-0 workgroups also materialise sub-panel t's own columns G_t into y[i][c0 + k] (row-major) and
// the rows' negated multipliers into mf[block-start row][c0 - C0 + k], where the rank-bw update finds them.
template <int BK>
struct __attribute__((aligned(16))) UpdateTileShared {
    static constexpr int LDA = 64 + ((32 / BK) > 0 ? (32 / BK) : 1);
    static constexpr int LDB = 64 + 4;
    static constexpr int LT = BK + 4;
    float s_b[BK * LDB];     // pivot rows (through the row map) x 64 columns; after the strip: u_m
    float s_xs[BK * LDB];    // the pivot rows after the W steps
    float s_lt[BK * LT];     // -multipliers of the W pivot rows, [step][row]
    float s_prn[BK * BK];    // sub-panel t's normalised pivot rows
    float s_bprev[BK * BK];  // u_m of sub-panel t-1 restricted to sub-panel t's columns
    float s_a[BK * LDA];     // -multipliers of the tile's rows, [k][row]
    int s_map[64];
    int s_pmap[BK];          // where the W pivot rows lie in the order before the sub-panel's swaps
    int s_rs[64];            // the tile's rows' indices at the start of the block
};

template <int BK, int NG>
__device__ __forceinline__ void inblock_update_body(const SubpanelArgs &A, int u, unsigned char *smem)
{
    typedef UpdateTileShared<BK> TS;
    constexpr int LDA = TS::LDA, LDB = TS::LDB, LT = TS::LT;
    constexpr int CPT = BK / 4;
    const int grp = threadIdx.x >> 8, tid = threadIdx.x & 255;
    TS &T = reinterpret_cast<TS *>(smem)[grp];
    const int np = A.np, ld = A.ld, c0 = A.u_c0;
    const int tiles_x = A.kb / 64;
    const int wgs_per_matrix = tiles_x * (np / 64) / NG;
    const int b = u / wgs_per_matrix;
    if (matrix_given_up(A.guard, b)) return;
    const int id = (u % wgs_per_matrix) * NG + grp;
    const int tx = id % tiles_x, ty = id / tiles_x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int row0 = ty * 64;
    const int col0 = A.C0 + tx * 64;
    const float *src = A.x + (size_t)b * A.mstride;
    float *dst = A.y + (size_t)b * A.mstride;
    const float *g = A.u_gt + (size_t)b * A.tstride;
    const float *mt = A.u_mt + (size_t)b * A.mtstride;
    const int mtld = A.mtld;
    const int *map = A.u_submap + (size_t)b * np;
    const bool some_above = row0 < A.u_above_hi || row0 + 64 > A.u_panel_hi;  // some of this tile's rows were not in panel(t)

    // Two dependent rounds of global loads in all: the maps first, then everything they index (old values,
    // multipliers, pivot rows) -- requested into registers back to back, before the first of them is needed.
    if (tid < 64) T.s_map[tid] = map[row0 + tid];
    else if (tid < 64 + BK) T.s_pmap[tid - 64] = map[c0 + tid - 64];
    else if (tid >= 128 && tid < 192) T.s_rs[tid - 128] = (A.u_rowsrc + (size_t)b * np)[row0 + tid - 128];
    if (some_above || (tx == 0 && A.u_tri)) {  // (the rows of a one-workgroup panel need the pivot rows as well)
        const float *aux = A.u_aux + (size_t)b * kAuxFloats;
        for (int i = tid; i < BK * BK; i += 256) {
            T.s_prn[i] = aux[i];
            if (A.u_has_prev) T.s_bprev[i] = aux[kMaxW * kMaxW + i];
        }
    }
    __syncthreads();
    // 32-bit byte offsets from the matrix's (scalar) base: one v_mad_u32_u24 per access instead of a 64-bit
    // multiply-add pair (np <= 16384: the last byte of a matrix lies below 2^31)
    const unsigned ld4 = (unsigned)ld * 4u;
    const char *srcb = reinterpret_cast<const char *>(src);
    // (1) the W pivot rows' own multipliers: Mt_t[step][index of the row of step kk in order after t-1]
    constexpr int NLT = (BK * BK + 255) / 256;
    float lval[NLT];
#pragma unroll
    for (int q = 0; q < NLT; ++q) {
        const int i = tid + q * 256;
        lval[q] = (i < BK * BK) ? mt[(size_t)(i % BK) * mtld + T.s_pmap[i / BK]] : 0.0f;
    }
    // (2) the W pivot rows (through the row map) x 64 columns
    constexpr int NBQ = (BK * 16 + 255) / 256;
    float4 bq[NBQ];
#pragma unroll
    for (int q = 0; q < NBQ; ++q) {
        const int idx = tid + q * 256;
        if (idx < BK * 16)
            bq[q] = *reinterpret_cast<const float4 *>(
                srcb + ((unsigned)T.s_pmap[idx / 16] * ld4 + (unsigned)(col0 + (idx % 16) * 4) * 4u));
    }
    // (3) the accumulators start from the (row-mapped) old values
    float16v acc;
    const int lcol = lane & 31;
    const int lhalf = lane >> 5;
    {
        const unsigned col4 = (unsigned)(col0 + wc * 32 + lcol) * 4u;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int lr = wr * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * lhalf;
            acc[reg] = *reinterpret_cast<const float *>(srcb + ((unsigned)T.s_map[lr] * ld4 + col4));
        }
    }
    {
        // (4) stage A = the tile's rows' multipliers, negated, [k][row]; 4 threads per row, BK/4 columns each.
        //  * rows that were in panel(t): its compact output mt[k][map[row]].  The row's new entries in sub-panel t's
        //    own columns: gt[k][map[row]] where the panel stored them (multi-workgroup and no-pivot panels), else
        //    (u_tri) computed here from the W multipliers and the pivot rows, panel_rows_step;
        //  * rows above (never candidates, never moved): the row's W entries of the panel input Pt_t, brought up
        //    to date with update(t-1) where that was still pending (the chain of the panel prologue: old value -
        //    sum_m f_m[row] * u_m[c], f_m as materialised in mf), then taken through the W pivot steps with the
        //    exported normalised pivot rows -- fixColumn (mat_inv_32.cpp:28-38) on one row, the very fmaf
        //    sequence the panel applies to a dead row; the entry the row holds in the pivot column when a step
        //    runs is its multiplier.
        const int rr = tid >> 2, q4 = tid & 3;
        const int grow = row0 + rr;
        float v[CPT], fm[CPT];
#pragma unroll
        for (int j = 0; j < CPT; ++j) { v[j] = 0.0f; fm[j] = 0.0f; }
        float *mfrow = A.u_mf + (size_t)b * A.mfstride + (size_t)T.s_rs[rr] * A.mf_ld + (c0 - A.C0);
        if (grow >= A.u_above_hi && grow < A.u_panel_hi) {
#pragma unroll
            for (int j = 0; j < CPT; ++j) fm[j] = mt[(size_t)(q4 * CPT + j) * mtld + T.s_map[rr]];
            if (tx == 0) {
                if (A.u_tri) {  // (the four threads of a row take this branch together: the multipliers cross the quad)
                    panel_rows_steps<BK>(v, fm, T.s_prn, q4, grow - c0, std::make_integer_sequence<int, BK>{});
                } else {
#pragma unroll
                    for (int j = 0; j < CPT; ++j) v[j] = g[(size_t)(q4 * CPT + j) * np + T.s_map[rr]];
                }
            }
        } else {
            const float *pt_in = A.u_pt_in + (size_t)b * A.tstride;
#pragma unroll
            for (int j = 0; j < CPT; ++j) v[j] = pt_in[(size_t)(q4 * CPT + j) * np + grow];
            if (A.u_has_prev) {
                const float *mp = mfrow - BK;  // -f_m of sub-panel t-1 for this row: same width, same block
#pragma unroll
                for (int k4 = 0; k4 < BK; k4 += 4) {
                    const float4 gq = *reinterpret_cast<const float4 *>(mp + k4);
                    const float gk4[4] = {gq.x, gq.y, gq.z, gq.w};
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                        for (int j = 0; j < CPT; ++j)
                            v[j] = __builtin_fmaf(gk4[kk], T.s_bprev[(k4 + kk) * BK + q4 * CPT + j], v[j]);
                }
            }
            above_rows_steps<BK>(v, fm, T.s_prn, q4, std::make_integer_sequence<int, BK>{});
        }
        // everything requested; now into LDS
#pragma unroll
        for (int q = 0; q < NLT; ++q) {
            const int i = tid + q * 256;
            if (i < BK * BK) T.s_lt[(i % BK) * LT + i / BK] = -lval[q];
        }
#pragma unroll
        for (int q = 0; q < NBQ; ++q) {
            const int idx = tid + q * 256;
            if (idx < BK * 16) *reinterpret_cast<float4 *>(&T.s_b[(idx / 16) * LDB + (idx % 16) * 4]) = bq[q];
        }
#pragma unroll
        for (int j = 0; j < CPT; ++j) T.s_a[(q4 * CPT + j) * LDA + rr] = -fm[j];
        if (tx == 0) {  // materialise: G_t into the row-major working copy, -f into the block's multiplier matrix
#pragma unroll
            for (int j = 0; j < CPT; ++j) {
                dst[(size_t)grow * ld + c0 + q4 * CPT + j] = v[j];
                mfrow[q4 * CPT + j] = -fm[j];
            }
        }
    }
    __syncthreads();
    {   // the strip: column tid >> 2 of the W pivot rows, rows CPT * (tid & 3) ... in this lane
        const int c = tid >> 2, q4 = tid & 3;
        float x[CPT];
#pragma unroll
        for (int j = 0; j < CPT; ++j) x[j] = T.s_b[(CPT * q4 + j) * LDB + c];
        strip_steps<BK>(x, T.s_lt, LT, q4, &T.s_b[c], LDB, std::make_integer_sequence<int, BK>{});
#pragma unroll
        for (int j = 0; j < CPT; ++j) T.s_xs[(CPT * q4 + j) * LDB + c] = x[j];
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < BK; kk += 2) {
        const float af = T.s_a[(kk + lhalf) * LDA + wr * 32 + lcol];
        const float bf = T.s_b[(kk + lhalf) * LDB + wc * 32 + lcol];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af, bf, acc, 0, 0, 0);
    }
    {
        const int col = col0 + wc * 32 + lcol;
        if (!(col >= c0 && col < c0 + BK)) {  // sub-panel t's own columns hold G_t, not an update result
            // the W pivot rows of t are rows c0 .. c0+W-1 of the new order: they take what the strip left
            if (row0 + wr * 32 < c0 + BK && row0 + wr * 32 + 32 > c0) {
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int rel = row0 + wr * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * lhalf - c0;
                    if ((unsigned)rel < (unsigned)BK) acc[reg] = T.s_xs[rel * LDB + wc * 32 + lcol];
                }
            }
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int grow = row0 + wr * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * lhalf;
                *reinterpret_cast<float *>(reinterpret_cast<char *>(dst) + ((unsigned)grow * ld4 + (unsigned)col * 4u)) = acc[reg];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)  // registers 4q .. 4q+3 are 4 consecutive rows: one 16-byte store
                panel_export_store4(A.u_exp, A.tstride, b, np, col, row0 + wr * 32 + 8 * q + 4 * lhalf, acc[4 * q],
                                    acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
        }
    }
}

// ---- strip(t): what the columns OUTSIDE the block see of sub-panel t's W pivot steps ---------------
// One 256-thread group per 64-column tile outside the block.  The W pivot rows of t have not been touched by the
// block's earlier sub-panels in these columns (their update is delayed to the end of the block), so their values at
// the start of the block first take the block's earlier steps,
//     x[kk][j] = fmaf(-f_m[row kk], u_m[j], x[kk][j]),  m = 0 .. c0 - C0 - 1 ascending        (mat_inv_32.cpp:28-38)
// (u_m: left in ub by the strips of the earlier sub-panels; -f_m: the block's multiplier matrix mf), then run their
// own W steps (strip_step: W dependent IEEE divisions).  Out: ub[c0 - C0 + m][j] = u_m[j], the pivot row of step m
// as fixColumn sees it = the B operand of the block's rank-bw update, and xs[c0 - C0 + kk][j] = pivot row kk after
// the sub-panel's last step = where that row's accumulation starts in the rank-bw update (which applies the later
// sub-panels' steps to it and nothing else: gj_mult_transpose_kernel masks the rest).
// The tiles ride in the launch of the NEXT panel (or in the block's last in-block update): off the chain of pivot steps.
//
// The earlier steps are one accumulation chain per element with m ascending -- what an fp32 MFMA computes with the old
// value as its C operand (the update tiles above).  Here it is v_mfma_f32_16x16x4_f32: four steps
// per instruction, 16 rows -- what W = 16 needs -- and a dependent instruction every 40 cycles instead of 64 for two
// steps; tests/test_gpu_outside_strips.py and tests/test_gpu_subnormal.py hold it to the oracle's bits.  Waves 0 and 1
// of the group take 32 of the tile's 64 columns each, as two 16-column tiles (two independent chains per wave; two row
// tiles at W = 32): C = the W pivot rows at the start of the block (rows past W: zero, A = 0, never stored),
// A = mf[row of kk][m], B = ub[m][column].  No barrier inside the loop: both operands are requested MC steps ahead of
// the chain, B (one row of ub per 16 lanes) straight into the registers the MFMA reads.  A is one float per lane and
// step from a different row of mf in every lane: a load in the MFMA's own layout touches W cache lines for 4 W useful
// bytes and the tiles become bound by those loads.  Each wave therefore reads its A set as 16-byte pieces of rows, four
// rows per 16 lanes, and turns it through a stage of its own in LDS (s_a[wave]: written and read by that wave alone,
// in program order, so no barrier).  The result goes through s_x into the quad layout of strip_steps.
typedef float float4v __attribute__((ext_vector_type(4)));

template <int BK>
struct __attribute__((aligned(16))) OStripShared {
    static constexpr int MC = 32;            // earlier steps per set of operands
    static constexpr int LDU = 64 + 4;
    static constexpr int LT = BK + 4;
    static constexpr int RS = BK + BK / 4;   // [step][row] stride of an A set: its writes and its reads hit distinct banks
    static constexpr int LPR = 64 / BK;      // lanes that share a row of mf in a load of the A set, 4 steps each
    static constexpr int NLA = BK >= 8 ? BK / 8 : 1;  // such loads per set
    float s_x[BK * LDU];    // the W pivot rows x 64 columns after the block's earlier steps; after the strip: u_m
    float s_xs[BK * LDU];   // the W pivot rows after the sub-panel's last step
    float s_lt[BK * LT];    // -multipliers of the W pivot rows in the W steps of t, [step][row]
    float s_a[2][MC * RS];  // per MFMA wave: -f_m of the W pivot rows in the set of steps it is working on
    int s_q[BK], s_idx[BK]; // their row index at the start of the block / in the order before t's swaps
};

// One set = the (at most MC) steps from m on; mc = the steps left from m on (a multiple of BK; more than MC: a whole
// set).  Lane l of a wave loads the steps k0 + 4 LPR q ... + 3 of row l / LPR (pa: that row of mf at column m + k0).
template <int BK>
__device__ __forceinline__ void ostrip_fetch_a(float4 (&an)[OStripShared<BK>::NLA], const float *pa, int k0, int mc)
{
    constexpr int LPR = OStripShared<BK>::LPR, NLA = OStripShared<BK>::NLA;
#pragma unroll
    for (int q = 0; q < NLA; ++q) {
        const int k = k0 + q * 4 * LPR;
        if (k < 32 && k < mc) an[q] = *reinterpret_cast<const float4 *>(pa + q * 4 * LPR);
    }
}
template <int BK>
__device__ __forceinline__ void ostrip_stage_a(float *sa, const float4 (&an)[OStripShared<BK>::NLA], int r, int k0, int mc)
{
    constexpr int LPR = OStripShared<BK>::LPR, NLA = OStripShared<BK>::NLA, RS = OStripShared<BK>::RS;
#pragma unroll
    for (int q = 0; q < NLA; ++q) {
        const int k = k0 + q * 4 * LPR;
        if (k < 32 && k < mc) {
            sa[(k + 0) * RS + r] = an[q].x;
            sa[(k + 1) * RS + r] = an[q].y;
            sa[(k + 2) * RS + r] = an[q].z;
            sa[(k + 3) * RS + r] = an[q].w;
        }
    }
    __builtin_amdgcn_wave_barrier();
}
// b[2 j + ct]: the lane's B value of MFMA j of the set in column tile ct -- steps m + 4j ... m + 4j + 3, quarter lk of
// the wave takes step m + 4j + lk (pb: the lane's column of ub at row m + lk; np4 = 4 np).  Only whole groups of
// min(BK, 32) steps are predicated.  The scheduling barrier keeps the loads of a set in front of the chain that runs
// while they travel.
template <int BK>
__device__ __forceinline__ void ostrip_fetch_b(float (&b)[16], const float *pb, unsigned np4, int mc)
{
    constexpr int G = BK < 32 ? BK : 32;
#pragma unroll
    for (int g0 = 0; g0 < 32; g0 += G) {
        if (G == 32 || g0 < mc) {
#pragma unroll
            for (int j = g0 / 4; j < (g0 + G) / 4; ++j) {
                b[2 * j] = pb[(size_t)j * np4];
                b[2 * j + 1] = pb[(size_t)j * np4 + 16];
            }
        }
    }
    __builtin_amdgcn_sched_barrier(0);
}
// sal: the lane's A values of the staged set, sa + lk RS + li; arow[rt]: the lane has a row in row tile rt, else A = 0.
// acc[2 rt + ct]: the 16 x 16 tile of rows 16 rt ..., columns 16 ct ... of the wave's 32.
template <int BK>
__device__ __forceinline__ void ostrip_chain(float4v (&acc)[BK > 16 ? 4 : 2], const float *sal, const bool (&arow)[2],
                                             const float (&b)[16], int mc)
{
    constexpr int G = BK < 32 ? BK : 32, RS = OStripShared<BK>::RS, RT = BK > 16 ? 2 : 1;
    float a[8][RT];
#pragma unroll
    for (int g0 = 0; g0 < 32; g0 += G) {
        if (G == 32 || g0 < mc) {
#pragma unroll
            for (int j = g0 / 4; j < (g0 + G) / 4; ++j)
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) a[j][rt] = sal[4 * j * RS + 16 * rt];
        }
    }
#pragma unroll
    for (int g0 = 0; g0 < 32; g0 += G) {
        if (G == 32 || g0 < mc) {
#pragma unroll
            for (int j = g0 / 4; j < (g0 + G) / 4; ++j)
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    const float av = arow[rt] ? a[j][rt] : 0.0f;
                    acc[2 * rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b[2 * j], acc[2 * rt], 0, 0, 0);
                    acc[2 * rt + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b[2 * j + 1], acc[2 * rt + 1], 0, 0, 0);
                }
        }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_sched_barrier(0);
}

template <int BK>
__device__ __forceinline__ void ostrip_body(const SubpanelArgs &A, int tile, unsigned char *smem_group, int tid)
{
    typedef OStripShared<BK> S;
    constexpr int MC = S::MC, LDU = S::LDU, LT = S::LT, CPT = BK / 4;
    S &T = *reinterpret_cast<S *>(smem_group);
    const int np = A.np, ld = A.ld, c0 = A.u_c0, C0 = A.C0, kb = A.kb;
    const int tiles = A.os_ntiles;
    // The 256-thread groups of a wider workgroup run different tiles and share the workgroup's barriers: no group
    // leaves early.  A group past the last tile repeats the last one without storing; a given-up matrix (its row
    // maps still hold valid positions) is computed and not stored.
    bool store_ok = tile < tiles * A.batch;
    if (!store_ok) tile = tiles * A.batch - 1;
    const int b = tile / tiles;
    store_ok = store_ok && !matrix_given_up(A.guard, b);
    int col0 = A.os_first + (tile % tiles) * 64;
    if (A.os_first == 0 && col0 >= C0) col0 += kb;  // all columns but the block's own
    const float *cur = A.os_cur + (size_t)b * A.mstride;
    const float *mt = A.u_mt + (size_t)b * A.mtstride;
    const float *mf = A.u_mf + (size_t)b * A.mfstride;
    float *ub = A.os_ub + (size_t)b * A.ubstride;
    float *xs = A.os_xs + (size_t)b * A.ubstride;
    const int K = c0 - C0;  // the block's steps before this sub-panel, a multiple of BK
    // (every group executes the same number of barriers: three, whatever K is)
    if (tid < BK) {
        T.s_idx[tid] = (A.u_submap + (size_t)b * np)[c0 + tid];
        T.s_q[tid] = (A.u_rowsrc + (size_t)b * np)[c0 + tid];
    }
    __syncthreads();
    for (int i = tid; i < BK * BK; i += 256)
        T.s_lt[(i % BK) * LT + i / BK] = -mt[(size_t)(i % BK) * A.mtld + T.s_idx[i / BK]];
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (wave < 2) {
        const int lane = tid & 63, li = lane & 15, lk = lane >> 4;
        const int col = col0 + wave * 32 + li;
        // register q of accumulator 2 rt + ct: row 16 rt + 4 lk + q of the W pivot rows, column 16 ct + li of the wave's 32
        constexpr int RT = BK > 16 ? 2 : 1;
        float4v acc[2 * RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = 16 * rt + 4 * lk + q;
                acc[2 * rt][q] = 0.0f;
                acc[2 * rt + 1][q] = 0.0f;
                if (row < BK) {
                    const float *src = cur + (size_t)T.s_q[row] * ld + col;
                    acc[2 * rt][q] = src[0];
                    acc[2 * rt + 1][q] = src[16];
                }
            }
        const bool arow[2] = {li < BK, 16 + li < BK};
        const int r = lane / S::LPR, k0 = 4 * (lane % S::LPR);
        const float *pa = mf + (size_t)T.s_q[r] * A.mf_ld + k0;
        const float *pb = ub + (size_t)lk * np + col;
        const unsigned np4 = 4u * (unsigned)np;
        const size_t bstep = (size_t)MC * np;
        float *sa = T.s_a[wave];
        const float *sal = sa + lk * S::RS + li % BK;
        float4 an[S::NLA];
        float b0[16], b1[16];
        __builtin_amdgcn_sched_barrier(0);
        if (K > 0) {
            ostrip_fetch_a<BK>(an, pa, k0, K);
            ostrip_fetch_b<BK>(b0, pb, np4, K);
        }
#pragma unroll 1
        for (int left = K; left > 0; left -= 2 * MC) {  // steps left; two sets of MC per trip
            ostrip_stage_a<BK>(sa, an, r, k0, left);
            if (left > MC) {
                ostrip_fetch_a<BK>(an, pa + MC, k0, left - MC);
                ostrip_fetch_b<BK>(b1, pb + bstep, np4, left - MC);
            }
            ostrip_chain<BK>(acc, sal, arow, b0, left);
            if (left > MC) {
                pa += 2 * MC;
                pb += 2 * bstep;
                ostrip_stage_a<BK>(sa, an, r, k0, left - MC);
                if (left > 2 * MC) {
                    ostrip_fetch_a<BK>(an, pa, k0, left - 2 * MC);
                    ostrip_fetch_b<BK>(b0, pb, np4, left - 2 * MC);
                }
                ostrip_chain<BK>(acc, sal, arow, b1, left - MC);
            }
        }
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = 16 * rt + 4 * lk + q;
                if (row < BK) {
                    T.s_x[row * LDU + wave * 32 + li] = acc[2 * rt][q];
                    T.s_x[row * LDU + wave * 32 + 16 + li] = acc[2 * rt + 1][q];
                }
            }
    }
    __syncthreads();
    const int c = tid >> 2, g = tid & 3;
    float x[CPT];
#pragma unroll
    for (int j = 0; j < CPT; ++j) x[j] = T.s_x[(CPT * g + j) * LDU + c];
    strip_steps<BK>(x, T.s_lt, LT, g, &T.s_x[c], LDU, std::make_integer_sequence<int, BK>{});
#pragma unroll
    for (int j = 0; j < CPT; ++j) T.s_xs[(CPT * g + j) * LDU + c] = x[j];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < (BK * 16 + 255) / 256; ++q) {
        const int idx = tid + q * 256;
        if (idx < BK * 16 && store_ok) {
            const int kk = idx / 16, c4 = (idx % 16) * 4;
            *reinterpret_cast<float4 *>(ub + (size_t)(K + kk) * np + col0 + c4) =
                *reinterpret_cast<const float4 *>(&T.s_x[kk * LDU + c4]);
            *reinterpret_cast<float4 *>(xs + (size_t)(K + kk) * np + col0 + c4) =
                *reinterpret_cast<const float4 *>(&T.s_xs[kk * LDU + c4]);
        }
    }
}

}  // namespace mi32
