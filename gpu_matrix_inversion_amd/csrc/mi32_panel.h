// mi32_panel.h -- panel(s) of the blocked fp32 path (gfx950 only): W pivot steps on a register-resident slab, by one
// workgroup or by several that exchange every step's winner.
#pragma once
#include "mi32_blocked_internal.h"
#include "mi32_dpp.h"
#include "mi32_strip.h"

namespace mi32 {

// Diagnostic builds (make stamps -> lib/libmat_inv_32_stamps.so, tools/panel_stamps.py) record s_memtime at the
// phase boundaries of every panel launch (wave 0 of workgroup 0); in the product build the macro expands to nothing.
#ifdef MI32_PANEL_STAMPS
__device__ unsigned long long *g_panel_stamps;  // [1024 launches][64 slots]
#define MI32_PSTAMP(TAG_, SLOT_)                                                                             \
    do {                                                                                                     \
        if (g_panel_stamps && threadIdx.x == 0 && blockIdx.x == 0)                                           \
            g_panel_stamps[(size_t)((TAG_) & 1023u) * 64 + (SLOT_)] = __builtin_amdgcn_s_memtime();          \
    } while (0)
#else
#define MI32_PSTAMP(TAG_, SLOT_) do { } while (0)
#endif

// ---- the panel: W pivot steps on a register-resident slab ----------------------
// Each thread keeps RPT rows of the panel in registers for the whole kernel: row
// CONTENTS never move between threads.  What a row swap changes is only an integer
// label = the position (row index of the working matrix) that the content of a
// register row currently occupies:
//   pivotElements (mat_inv_32.cpp:154-173)  ==  exchange of two labels.
// submap[position] = where the data that now belongs at that position lies in the
// previous order tells the rank-k updates where every other column's data still lives.

template <int NW, int W, bool TRI>
struct __attribute__((aligned(16))) PanelShared {
    float cand[NW][W];          // per wave: its best candidate row as found (wave-private scratch)
    float prn[2][NW][W];        // per step parity, per wave: that row NORMALISED (candidate pivot row)
    unsigned long long key[W];  // one cross-wave arg-max word per step, zeroed at kernel start
    float prn_all[W][W];        // the normalised pivot row of every step, exported for the rows above the block
    float bprev[W][W];          // the previous sub-panel's W pivot rows, restricted to this sub-panel's columns
    float uprev[W][W];          // ... as that sub-panel's own steps saw them (u_m of the strip)
    float lt[W][W + 4];         // -multipliers of those W pivot rows, [step][row] (the prologue's strip)
    unsigned gx[2][kMaxPanelGroups][W + 2];  // multi-workgroup panels: every workgroup's winner of this step
    int lost;                   // multi-workgroup panels: a partner timed out (sticky; zeroed at kernel start)
    // triangular steps (the only instances that pay for it): the winner of step R as found, [R][c < R] = its
    // multipliers of the earlier steps, [R][R] = its pivot (tri_left_rows makes prn_all's left part of them)
    float raw[TRI ? W : 1][W];
};

// which matrix row register row k of thread tid holds: V consecutive rows per thread so that the
// compact panel is loaded and stored with one 4*V-byte access per column (three rows per lane: V = 1 -- a vector of
// three floats occupies 16 bytes)
template <int RPT>
constexpr int panel_vec()
{
    return RPT == 3 ? 1 : (RPT < 4 ? RPT : 4);
}
template <int NT, int RPT>
__device__ __forceinline__ int panel_row(int tid, int k)
{
    constexpr int V = panel_vec<RPT>();
    return (k / V) * (V * NT) + V * tid + (k % V);
}

// One pivot step (column c0 + R of the working matrix, R a compile-time constant) with ONE workgroup
// barrier.
//
// The step is a chain of dependent, mostly scalar and cross-lane operations executed by in-order waves:
// s_memtime stamps show ~3500 cycles per step even with ONE wave per SIMD, of
// which the 16 FMAs per row are ~5 %.  What a step costs is the NUMBER of instructions every wave runs
// between two barriers, so the step is written to be short rather than clever:
//  * ONE pass over the lane's rows finds its best candidate under the exact order of the reference's scan
//    (largest |a|, lowest position among equals; mat_inv_32.cpp:121-127): a 64-bit comparison of
//    {bits(|a|), ~position}.  The whole state of a row is ONE register npl[k]: ~position (top bit set)
//    while the row can still be chosen, its position itself (top bit clear) once it cannot -- rows above
//    the block, rows already used as a pivot in this panel, rows beyond the matrix.  A dead row's |a| key
//    is masked to 0 and its small npl loses every tie against a live row;
//  * one DPP max over the 32-bit |a| keys, one ballot; only a genuine tie between lanes pays for a second
//    DPP reduction over the positions;
//  * every wave SPECULATES: the lane that holds the wave's best candidate writes that row to LDS, lanes
//    0..W-1 divide one element each by the candidate's pivot-column entry (IEEE division, the identity
//    column's entry becomes 1/pivot) and publish the NORMALISED row next to a 64-bit arg-max key
//    (ds_max_u64).  After the single barrier the key's low bits name the winning wave and its row is read
//    straight from LDS: no second barrier and no division on the post-barrier path;
//  * pivotElements (mat_inv_32.cpp:154-173) is an exchange of two position labels, done branch-free by
//    every lane (no table of who holds which position);
//  * a NaN is never special-cased in the search: its bit pattern wins the unsigned max, the step then has
//    a NaN pivot and the winning wave flags the matrix as singular -- the result is poisoned either way.
// What a workgroup of a multi-workgroup panel knows about the others (MULTI instances only).
struct PanelGroup {
    int ngroups, grp;           // workgroups sharing this panel, and which one this is
    unsigned long long *xch;    // this matrix's exchange granules, [2][kMaxPanelGroups][32] x {payload, tag}
    unsigned tag_base;          // unique per launch within a call (<< 8 | step + 1 = the tag of a step)
    bool timed_out;
};

// V floats to sbase (wave-uniform) + voff bytes (per lane): global_store with a scalar base.  (Inline asm: hipcc does
// not insert the wait state between a store of more than 8 bytes and the overwrite of its data registers here.)
template <int V, typename T>
__device__ __forceinline__ void mt_store(float *sbase, unsigned voff, T v)
{
    if constexpr (V == 1) asm volatile("global_store_dword %0, %1, %2" ::"v"(voff), "v"(v), "s"(sbase));
    else if constexpr (V == 2) asm volatile("global_store_dwordx2 %0, %1, %2" ::"v"(voff), "v"(v), "s"(sbase));
    else asm volatile("global_store_dwordx4 %0, %1, %2\n\ts_nop 1" ::"v"(voff), "v"(v), "s"(sbase));
}

// Every step stores its multiplier column straight away: mtp = this lane's first slot of Mt row 0 (slab order), or,
// LBL (fused instances: the rows' labels at entry differ from their slab index), mt_base + moff[k] per row.
template <int NT, int RPT, int W, int R, bool MULTI, bool LBL>
__device__ __forceinline__ void panel_step(float (&a)[RPT][W], unsigned (&npl)[RPT],
                                           const int (&moff)[LBL ? RPT : 1],
                                           PanelShared<NT / 64, W, panel_tri(NT, RPT, W, MULTI, LBL)> &sh,
                                           int wave_u, int c0, bool wave_active, bool &singular, PanelGroup &pg,
                                           float *mtp, int mtld)
{
    constexpr int par = R & 1;
    constexpr bool TRI = panel_tri(NT, RPT, W, MULTI, LBL);  // the step runs on the columns c > R only (fixColumn below)
    const int slot = c0 + R;
    // The lane id is recomputed in every step (two v_mbcnt, opaque to the optimiser): a `lane` carried through
    // the 16 unrolled steps is the first thing the 128-VGPR instances spill, and every path of the step reads
    // it -- a scratch reload in front of each compare on the critical path.
    int lane;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));

    constexpr bool kSub = (R == W / 2);  // diagnostic builds: phase stamps inside one representative step
    if (kSub) MI32_PSTAMP(pg.tag_base, 32);
    // -- maxPivot over this lane's rows
    float col[RPT];
#pragma unroll
    for (int k = 0; k < RPT; ++k) col[k] = a[k][R];
    // the multiplier column of this step (mat_inv_32.cpp:30: what fixColumn reads before it overwrites the column);
    // the pivot row's own entry is the pivot
    // One store per step, fire and forget -- written so that NOTHING of it lives in vector registers across the
    // steps: the base is scalar (global_store ... saddr form), the 32-bit lane offset is recomputed from the lane id
    // (fused instances: one kept offset per row).  A pointer kept in VGPRs is the first thing the 128-VGPR instances
    // spill, and its reload's s_waitcnt vmcnt(0) then waits for the previous step's store to be acknowledged by the
    // memory system: +0.9 us per pivot step (measured: 28.5 -> 43 us per 16-step launch).
    if constexpr (LBL) {
#pragma unroll
        for (int k = 0; k < RPT; ++k) mt_store<1>(mtp + (size_t)R * mtld, (unsigned)moff[k] * 4u, col[k]);
    } else {
        constexpr int V = panel_vec<RPT>();
        typedef float mvecV __attribute__((ext_vector_type(V)));
        const unsigned voff = (unsigned)(wave_u * 64 + lane) * (4u * V);
#pragma unroll
        for (int g = 0; g < RPT / V; ++g) {
            mvecV v;
#pragma unroll
            for (int j = 0; j < V; ++j) v[j] = col[g * V + j];
            if constexpr (V == 1) mt_store<1>(mtp + (size_t)R * mtld + g * (V * NT), voff, v[0]);
            else mt_store<V>(mtp + (size_t)R * mtld + g * (V * NT), voff, v);
        }
    }
    int own_lane = -1, own_k = 0;
    bool cand_bad = false;  // this wave's candidate has a zero / NaN / infinite pivot entry
    float qv = 0.0f;        // lanes 0..W-1: this wave's candidate row, normalised (kept for the export if it wins)
    if (wave_active) {
        unsigned mkey = 0u, mnp = 0u;
        int kb = 0;
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
            const unsigned lm = (unsigned)((int)npl[k] >> 31);                    // all ones while live
            const unsigned key = __float_as_uint(col[k]) & lm & 0x7fffffffu;
            // (two 32-bit compares, not one 64-bit compare: the register pairs a v_cmp_gt_u64 needs cost the 128-VGPR
            // instances copies and spills in the middle of the steps)
            const bool better = key > mkey || (key == mkey && npl[k] > mnp);
            mkey = better ? key : mkey;
            mnp = better ? npl[k] : mnp;
            kb = better ? k : kb;
        }
        if (kSub) MI32_PSTAMP(pg.tag_base, 33);
        const unsigned wm = wave_max_u32(mkey);
        if (kSub) MI32_PSTAMP(pg.tag_base, 34);
        // lanes that hold the wave maximum and a real candidate: almost always exactly one
        unsigned long long hit = __ballot(mkey == wm && (int)mnp < 0);
        if (hit != 0ull) {  // this wave has a candidate
            if ((hit & (hit - 1ull)) != 0ull) {  // tie between lanes: lowest position = largest ~position
                const unsigned hv = (mkey == wm && (int)mnp < 0) ? mnp : 0u;
                const unsigned hmax = wave_max_u32(hv);  // all lanes take part: never under a lane condition
                hit = __ballot(hv == hmax);              // hmax != 0: at least two lanes hold a live candidate
            }
            own_lane = __ffsll((long long)hit) - 1;
            own_k = __builtin_amdgcn_readlane(kb, own_lane);
            const unsigned wi = ~(unsigned)__builtin_amdgcn_readlane((int)mnp, own_lane);
            // the candidate row, as found, into this wave's scratch slot (the holder lane writes it)
#pragma unroll
            for (int k = 0; k < RPT; ++k)
                if (own_k == k) {
                    if (lane == own_lane) {
#pragma unroll
                        for (int c = 0; c < W; c += 4)
                            *reinterpret_cast<float4 *>(&sh.cand[wave_u][c]) =
                                make_float4(a[k][c], a[k][c + 1], a[k][c + 2], a[k][c + 3]);
                    }
                }
            if (kSub) MI32_PSTAMP(pg.tag_base, 35);
            // fixRow, speculatively: lanes 0..W-1 divide one element each (IEEE); identity entry -> 1/piv.
            // One wave's LDS operations execute in order, so no s_barrier is needed between the holder
            // lane's store and these loads -- only the compiler must not reorder here.
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const float cpiv = sh.cand[wave_u][R];
            const float num = (lane < W) ? ((lane == R) ? 1.0f : sh.cand[wave_u][lane]) : 0.0f;
            if (kSub) MI32_PSTAMP(pg.tag_base, 36);
            qv = num / cpiv;
            // Triangular steps: the candidate's columns < R hold its multipliers of those steps, not row entries
            // (the steps below leave columns <= R alone).  Should it win, the register takes to LDS what the epilogue
            // needs instead: lanes < R the multiplier as found, lane W the pivot.
            if constexpr (TRI) qv = (lane < R) ? num : (lane == W ? cpiv : qv);
            cand_bad = pivot_unusable(cpiv);
            if (kSub) MI32_PSTAMP(pg.tag_base, 37);
            if (lane < W) sh.prn[par][wave_u][lane] = qv;
            if (lane == 0)
                atomicMax(&sh.key[R], ((unsigned long long)wm << 32) |
                                          (unsigned long long)(((0xFFFFFu - wi) << 8) | (unsigned)wave_u));
        }
    }
    if (kSub) MI32_PSTAMP(pg.tag_base, 38);
    __syncthreads();
    if (kSub) MI32_PSTAMP(pg.tag_base, 39);
    // (Tried: reading every wave's candidate in the same LDS round as the arg-max word and picking the winner's W
    // entries out of their lanes with v_readlane into SGPRs -- no dependent second read, no spills in the 128-VGPR
    // instances.  16 v_readlane per wave and step cost more than the LDS round trip they replace once 2 or 4
    // waves share a SIMD: 2905 -> 3556 cycles per step at 4096 rows, 1876 -> 1800 with one wave per SIMD.)
    unsigned long long key = sh.key[R];
    unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(key & 0xFFFFFFFFull));
    if (kSub) MI32_PSTAMP(pg.tag_base, 40);
    float prn[W];  // prn[R] = 1/piv (the identity column's entry), prn[c] = normalised pivot row
    bool my_group_won = true;
    if constexpr (MULTI) {
        // -- the workgroups of this panel exchange their local winners: W normalised entries + the 64-bit key,
        //    as 8-byte {payload, tag} granules, each written by ONE agent-scope store and polled with agent-scope
        //    loads (a granule is its own flag: MI355X_MICROARCH.md, handoff-1to1).  The tag is unique per step
        //    and launch and the buffers alternate with the step parity: a workgroup can only be one step ahead.
        //    Every spin is bounded: on a time-out the matrix is flagged and the step goes on with what it has.
        const unsigned tag = (pg.tag_base << 8) | (unsigned)(R + 1);
        unsigned long long *xq = pg.xch + (size_t)par * (kMaxPanelGroups * 32);
        if (wave_u == 0 && lane < W + 2) {
            const int lwv = (int)(lo & 0xFFu);
            unsigned payload;
            if (lane < W) payload = __float_as_uint(sh.prn[par][lwv][lane]);
            else if (lane == W) payload = (lo & ~0xFFu) | ((unsigned)pg.grp << 4) | (unsigned)lwv;
            else payload = (unsigned)(key >> 32);
            __hip_atomic_store(&xq[pg.grp * 32 + lane], ((unsigned long long)tag << 32) | payload, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        }
        if (wave_u < pg.ngroups) {  // wave g collects workgroup g's record (its own workgroup's too)
            const unsigned long long *src = xq + wave_u * 32;
            unsigned long long v = 0ull;
            // Every spin is bounded in TIME (s_memrealtime: 100 MHz).  A partner that has not shown up after
            // kPanelXchTimeoutTicks is given up for good: its record counts as "no candidate" (key 0) in this and
            // every later step -- all labels stay valid positions of the present rows -- the matrix is flagged
            // MI32_RUNTIME_ERROR, skipped by every later launch of the call and handed out NaN-filled.
            const unsigned long long t_start = __builtin_amdgcn_s_memrealtime();
            for (;;) {
                if (lane < W + 2) v = __hip_atomic_load(&src[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const bool ok = (lane >= W + 2) || ((unsigned)(v >> 32) == tag);
                if (__all(ok)) break;
                if (pg.timed_out || __builtin_amdgcn_s_memrealtime() - t_start > kPanelXchTimeoutTicks) {
                    v = 0ull;
                    if (lane == 0) sh.lost = 1;
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
            if (lane < W + 2) sh.gx[par][wave_u][lane] = (unsigned)v;
        }
        __syncthreads();
        if (sh.lost != 0) pg.timed_out = true;  // workgroup-uniform from here on
        int gw = 0;
        key = ((unsigned long long)sh.gx[par][0][W + 1] << 32) | sh.gx[par][0][W];
#pragma unroll
        for (int g = 1; g < kMaxPanelGroups; ++g)
            if (g < pg.ngroups) {
                const unsigned long long kg = ((unsigned long long)sh.gx[par][g][W + 1] << 32) | sh.gx[par][g][W];
                if (kg > key) { key = kg; gw = g; }
            }
        gw = __builtin_amdgcn_readfirstlane(gw);
        lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(key & 0xFFFFFFFFull));
        my_group_won = (gw == pg.grp);
#pragma unroll
        for (int c = 0; c < W; c += 4) {
            const uint4 t = *reinterpret_cast<const uint4 *>(&sh.gx[par][gw][c]);
            prn[c] = __uint_as_float(t.x); prn[c + 1] = __uint_as_float(t.y);
            prn[c + 2] = __uint_as_float(t.z); prn[c + 3] = __uint_as_float(t.w);
        }
        if (wave_u == 0 && lane < W) sh.prn_all[R][lane] = __uint_as_float(sh.gx[par][gw][lane]);
    }
    int p = (int)(0xFFFFFu - (lo >> 8));
    if constexpr (MULTI) {
        // no record at all (only after a partner was lost and this workgroup has no candidate left): keep the
        // label a valid position -- nothing out of range may ever reach the row maps
        if (key == 0ull) p = slot;
    }
    const int wv = MULTI ? (int)(lo & 0xFu) : (int)(lo & 0xFFu);
    if (key == 0ull) singular = true;  // cannot happen (position `slot` is always a live candidate); never trust it
    if constexpr (!MULTI) {  // triangular steps: only the columns c > R are read below
#pragma unroll
        for (int c = TRI ? ((R + 1) / 4) * 4 : 0; c < W; c += 4) {
            const float4 t = *reinterpret_cast<const float4 *>(&sh.prn[par][wv][c]);
            prn[c] = t.x; prn[c + 1] = t.y; prn[c + 2] = t.z; prn[c + 3] = t.w;
        }
    }
    if (kSub) { asm volatile("" ::"v"(prn[W - 1])); MI32_PSTAMP(pg.tag_base, 41); }
    // -- fixColumn on the slab, branch-free; the pivot column holds the implicit identity column, whose
    //    entry is 0 in every row but the pivot row.  The pivot row itself is overwritten right after.
    //    Triangular steps (panel_tri, mi32_internal.h) run on the columns c > R only -- all that the later searches
    //    and multipliers depend on.  A column c <= R keeps what it held when its own step ran, the row's multiplier of
    //    that step (its pivot, in the pivot row): the finished entries of those columns are a function of the
    //    multipliers and the normalised pivot rows, and the update tiles evaluate it (inblock_update_body).
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
        const float f = col[k];
        if constexpr (!TRI) {
#pragma unroll
            for (int c = 0; c < W; ++c)
                a[k][c] = (c == R) ? __builtin_fmaf(-f, prn[R], 0.0f) : __builtin_fmaf(-f, prn[c], a[k][c]);
        } else {
#pragma unroll
            for (int c = R + 1; c < W; ++c) a[k][c] = __builtin_fmaf(-f, prn[c], a[k][c]);
        }
    }
    if (kSub) { asm volatile("" ::"v"(a[0][W - 1]), "v"(a[RPT - 1][W - 1])); MI32_PSTAMP(pg.tag_base, 42); }
    // -- pivotElements == exchange of two position labels: the row that held `slot` takes p ...
    if (p != slot) {
#pragma unroll
        for (int k = 0; k < RPT; ++k) npl[k] = (npl[k] == ~(unsigned)slot) ? ~(unsigned)p : npl[k];
    }
    // ... and the winner's candidate row (its wave knows lane and row) becomes the pivot row: normalised
    // values, label `slot`, no longer a candidate
    if (my_group_won && wave_u == wv) {
        // the winner's own pivot entry decides "singular" (zero, NaN or infinite pivot); its normalised row is
        // still in lanes 0..W-1 -- no LDS read on the slowest wave's way to the next barrier
        if (cand_bad) singular = true;
        if constexpr (TRI) {
            // qv: lanes < R the candidate's multipliers as found, lanes R .. W-1 its normalised row, lane W its pivot.
            // One LDS store on the slowest wave's way to the next barrier, as in the full step: the address differs.
            float *dst = &sh.prn_all[R][lane];
            if (lane < R) dst = &sh.raw[R][lane];
            if (lane == W) dst = &sh.raw[R][R];
            if (lane <= W) *dst = qv;
        } else if (!MULTI && lane < W) {
            sh.prn_all[R][lane] = qv;
        }
#pragma unroll
        for (int k = 0; k < RPT; ++k)
            if (own_k == k) {
                if (lane == own_lane) {
#pragma unroll
                    for (int c = TRI ? R + 1 : 0; c < W; ++c) a[k][c] = prn[c];
                    npl[k] = (unsigned)slot;
                }
            }
    }
    MI32_PSTAMP(pg.tag_base, 3 + R);
}

template <int NT, int RPT, int W, bool MULTI, bool LBL, int... Rs>
__device__ __forceinline__ void panel_steps(float (&a)[RPT][W], unsigned (&npl)[RPT],
                                            const int (&moff)[LBL ? RPT : 1],
                                            PanelShared<NT / 64, W, panel_tri(NT, RPT, W, MULTI, LBL)> &sh,
                                            int wave_u, int c0, bool wave_active, bool &singular, PanelGroup &pg,
                                            float *mtp, int mtld, std::integer_sequence<int, Rs...>)
{
    (panel_step<NT, RPT, W, Rs, MULTI, LBL>(a, npl, moff, sh, wave_u, c0, wave_active, singular, pg, mtp, mtld), ...);
}

// Triangular steps, after the last one: the entries the W pivot rows hold LEFT of their pivot column, which no step
// computed.  The row that won step R entered it with
//     x[c] = fmaf(-f_{R-1}, prn_{R-1}[c], ... fmaf(-f_{c+1}, prn_{c+1}[c], fmaf(-f_c, prn_c[c], 0)) ...),   c < R,
// (fixColumn of the steps c .. R-1 on its column c, which held the identity column's 0 when step c ran; f_m = the
// multiplier it kept in column m = raw[R][m]) and fixRow made prn_R[c] = x[c] / pivot (IEEE division, as in the
// step).  Lane c owns column c: what it needs of the earlier pivot rows, prn_m[c], c < m < R, it has computed itself;
// prn_c[c] = 1/pivot_c is in prn_all already.  One wave; no step of the chain waits for another lane.
template <int W, int R>
__device__ __forceinline__ void tri_left_row(float (&pl)[W], const float (&raw)[W][W], int c)
{
    if constexpr (R == 0) return;  // the first pivot row has nothing left of its pivot
    float v = 0.0f;
#pragma unroll
    for (int m = 0; m < R; ++m) {
        const float t = __builtin_fmaf(-raw[R][m], pl[m], v);
        v = (m >= c) ? t : v;
    }
    const float q = v / raw[R][R];
    pl[R] = (c < R) ? q : pl[R];
}
template <int W, int... Rs>
__device__ __forceinline__ void tri_left_rows(float (&pl)[W], const float (&raw)[W][W], int c,
                                              std::integer_sequence<int, Rs...>)
{
    (tri_left_row<W, Rs>(pl, raw, c), ...);
}

template <int NW, int W, bool TRI>
constexpr size_t panel_shared_bytes()
{
    return (sizeof(PanelShared<NW, W, TRI>) + 15) & ~(size_t)15;
}

// panel(s) of one matrix: the whole workgroup.  smem: panel_shared_bytes + 2 * RPT * NT ints.
// FUSED = false compiles the pending-update prologue (and the labels-at-entry indirection) out: the instances
// with 4 and more rows per lane have no registers to spare for code they never run.
// MULTI: the panel is shared by A.ngroups workgroups; this one (grp) holds the rows
// [row_lo + grp * NT * RPT, row_lo + (grp + 1) * NT * RPT) and takes part in the per-step exchange (panel_step).
template <int NT, int RPT, int W, bool FUSED, bool MULTI>
__device__ __forceinline__ void panel_body(const SubpanelArgs &A, int b, int grp, unsigned char *smem)
{
    static_assert(!(FUSED && MULTI), "multi-workgroup panels are never fused");
    if (matrix_given_up(A.guard, b)) return;
    const bool has_prev = FUSED && A.has_prev;
    constexpr int V = panel_vec<RPT>();
    constexpr int NW = NT / 64;
    typedef float vecV __attribute__((ext_vector_type(V)));
    typedef int ivecV __attribute__((ext_vector_type(V)));
    constexpr bool TRI = panel_tri(NT, RPT, W, MULTI, FUSED);
    PanelShared<NW, W, TRI> &sh = *reinterpret_cast<PanelShared<NW, W, TRI> *>(smem);
    int *s_park = reinterpret_cast<int *>(smem + panel_shared_bytes<NW, W, TRI>());  // [2][RPT][NT]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave_u = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int np = A.np, c0 = A.c0;
    const int row_lo = A.row_lo + (MULTI ? grp * (NT * RPT) : 0);  // first row THIS workgroup holds
    const float *pt = A.pt_in + (size_t)b * A.tstride;
    const int *invsub_prev = A.invsub_prev + (size_t)b * np;
    float *mt = A.mt_out + (size_t)b * A.mtstride;
    const int mtld = A.mtld;
    if (tid < W) sh.key[tid] = 0ull;
    if (tid == 0) sh.lost = 0;
    MI32_PSTAMP(A.tag_base, 0);

    // -- the slab and every row's label at entry (its position after the previous sub-panel's swaps)
    float a[RPT][W];
    unsigned npl[RPT];
#pragma unroll
    for (int g = 0; g < RPT / V; ++g) {
        const int row = row_lo + panel_row<NT, RPT>(tid, g * V);  // first of V consecutive rows
        ivecV p0;
#pragma unroll
        for (int j = 0; j < V; ++j) p0[j] = row + j;
        if (has_prev && row < np) p0 = *reinterpret_cast<const ivecV *>(invsub_prev + row);
#pragma unroll
        for (int c = 0; c < W; ++c) {
            vecV v;
            if (row < np) v = *reinterpret_cast<const vecV *>(pt + (size_t)c * np + row);
            else v = (vecV)(0.0f);
#pragma unroll
            for (int j = 0; j < V; ++j) a[g * V + j][c] = v[j];
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            // A candidate is a row of the matrix at or below the block.  The identity padding comes first
            // (mi32_blocked.hip): its rows are retired by their own steps before the first real column is
            // searched, so a real column only ever takes its pivot from the real rows.
            // Rows beyond the matrix (row >= np) are dead and are never written back.
            const bool live = (row + j < np) && (p0[j] >= c0);
            npl[g * V + j] = live ? ~(unsigned)p0[j] : (unsigned)p0[j];
        }
    }
    // the row maps this workgroup will permute: fetched now (by label), so their latency hides behind the
    // steps, and parked in thread-private LDS slots (the 1024-thread instances have no registers to spare)
    const int *rowsrc_in = A.rowsrc_in + (size_t)b * np;
    int *rowsrc = A.rowsrc_out + (size_t)b * np;
    int *orig = A.orig + (size_t)b * np;
    // All 2 * RPT loads are requested before the first is used (addresses clamped instead of guarded: behind a
    // condition hipcc waits for each load before it issues the next -- eight dependent round trips in front of the
    // first pivot step of a 4-rows-per-lane panel).
    {
        int pr[RPT], po[RPT];
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
            const int row = row_lo + panel_row<NT, RPT>(tid, k);
            const int p0 = (int)(npl[k] ^ (unsigned)((int)npl[k] >> 31));
            const int pi = row < np ? p0 : 0;
            pr[k] = rowsrc_in[pi];
            po[k] = orig[pi];
        }
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
            const int row = row_lo + panel_row<NT, RPT>(tid, k);
            const int p0 = (int)(npl[k] ^ (unsigned)((int)npl[k] >> 31));
            s_park[k * NT + tid] = (A.first_in_block || row >= np) ? p0 : pr[k];  // composite map so far
            s_park[(RPT + k) * NT + tid] = row < np ? po[k] : 0;
        }
    }
    // rows above the block keep their place: identity entries in the maps the update kernels read
    if (A.first_in_block && grp == 0) {
        for (int i = tid; i < row_lo; i += NT) rowsrc[i] = i;
        if (A.rowsrc_alt != nullptr) {
            int *alt = A.rowsrc_alt + (size_t)b * np;
            for (int i = tid; i < row_lo; i += NT) alt[i] = i;
        }
    }

#ifdef MI32_PANEL_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    MI32_PSTAMP(A.tag_base, 1);
    if (has_prev) {
        // -- update(s-1) on this sub-panel's columns, which nobody has applied yet: the W pivot steps of s-1 as
        //    every column outside that sub-panel sees them (strip_step above).  First the strip on the W pivot rows
        //    of s-1, which this workgroup holds (one wave: W columns x 4 lanes); then every other row takes
        //      a[row][c] = fmaf(-f_m[row], u_m[c], a[row][c]),  m ascending
        //    -- one fmaf per element and step from the old value: the reference's own order (mat_inv_32.cpp:28-38).
        constexpr int CPT = W / 4;
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
            const int rel = (int)npl[k] - A.c0_prev;  // dead rows carry their position itself
            if ((unsigned)rel < (unsigned)W && row_lo + panel_row<NT, RPT>(tid, k) < np) {
#pragma unroll
                for (int c = 0; c < W; ++c) sh.bprev[rel][c] = a[k][c];
            }
        }
        {   // the multipliers of those W rows in the W steps of s-1, negated, [step][row]: Mt_{s-1} is stored by the
            // rows' labels at the entry of panel(s-1), submap_{s-1} says which label the pivot row of each step had
            const float *mtp = A.mt_prev + (size_t)b * A.mtstride;
            const int *smp = A.submap_prev + (size_t)b * np;
            for (int i = tid; i < W * W; i += NT)
                sh.lt[i % W][i / W] = -mtp[(size_t)(i % W) * mtld + smp[A.c0_prev + i / W]];
        }
        __syncthreads();
        if (tid < 4 * W) {
            const int c = tid >> 2, g = tid & 3;
            float x[CPT];
#pragma unroll
            for (int j = 0; j < CPT; ++j) x[j] = sh.bprev[CPT * g + j][c];
            strip_steps<W>(x, &sh.lt[0][0], W + 4, g, &sh.uprev[0][c], W, std::make_integer_sequence<int, W>{});
#pragma unroll
            for (int j = 0; j < CPT; ++j) sh.bprev[CPT * g + j][c] = x[j];
        }
        __syncthreads();
        const float *mtp = A.mt_prev + (size_t)b * A.mtstride;
        // registers of multipliers per round (32: hipcc hoists every LDS read of the round and spills them -- 892 B
        // of scratch per lane in the 1024 x 2 instance)
        constexpr int kProRegs = 16;
        constexpr int KC = (kProRegs / RPT) < 1 ? 1 : ((kProRegs / RPT) > W ? W : (kProRegs / RPT));  // k's per round of loads
        // a ROLLED loop over the rounds: unrolled, hipcc hoists every round's loads to the top and the whole of
        // Mt_{s-1} (RPT * W registers) is live beside the slab
#pragma unroll 1
        for (int k0 = 0; k0 < W; k0 += KC) {
            vecV gv[KC][RPT / V];
#pragma unroll
            for (int kk = 0; kk < KC; ++kk)
#pragma unroll
                for (int g = 0; g < RPT / V; ++g) {
                    const int row = row_lo + panel_row<NT, RPT>(tid, g * V);
                    gv[kk][g] = (row < np) ? *reinterpret_cast<const vecV *>(mtp + (size_t)(k0 + kk) * mtld + row)
                                           : (vecV)(0.0f);
                }
#pragma unroll
            for (int kk = 0; kk < KC; ++kk)
#pragma unroll
                for (int c4 = 0; c4 < W; c4 += 4) {
                    const float4 bq = *reinterpret_cast<const float4 *>(&sh.uprev[k0 + kk][c4]);
#pragma unroll
                    for (int g = 0; g < RPT / V; ++g)
#pragma unroll
                        for (int j = 0; j < V; ++j) {
                            const float nf = -gv[kk][g][j];
                            a[g * V + j][c4 + 0] = __builtin_fmaf(nf, bq.x, a[g * V + j][c4 + 0]);
                            a[g * V + j][c4 + 1] = __builtin_fmaf(nf, bq.y, a[g * V + j][c4 + 1]);
                            a[g * V + j][c4 + 2] = __builtin_fmaf(nf, bq.z, a[g * V + j][c4 + 2]);
                            a[g * V + j][c4 + 3] = __builtin_fmaf(nf, bq.w, a[g * V + j][c4 + 3]);
                        }
                }
        }
        // the pivot rows of s-1 themselves: what the strip left
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
            const int rel = (int)npl[k] - A.c0_prev;
            if ((unsigned)rel < (unsigned)W && row_lo + panel_row<NT, RPT>(tid, k) < np) {
#pragma unroll
                for (int c = 0; c < W; ++c) a[k][c] = sh.bprev[rel][c];
            }
        }
    }
    bool singular = false;
    __syncthreads();  // sh.key[] zeroed before any wave's first atomicMax; all map reads issued
    PanelGroup pg = {A.ngroups, grp, A.xch + (size_t)b * kXchGranules, A.tag_base, false};
    MI32_PSTAMP(A.tag_base, 2);
    // Mt_s: by the rows' labels at entry (order after s-1, what update(s) and the next fused panel index it by).
    // Unfused panels hold their rows in that very order: this lane's first slot in row 0 of Mt (rows beyond np land
    // in the padding of the mtld-wide rows).  Fused panels hold them in the order after s-2: one offset per row.
    int moff[FUSED ? RPT : 1];
    if constexpr (FUSED) {
#pragma unroll
        for (int g = 0; g < RPT / V; ++g) {
            const int row = row_lo + panel_row<NT, RPT>(tid, g * V);
#pragma unroll
            for (int j = 0; j < V; ++j) moff[g * V + j] = row + j;  // rows beyond np: a slot in the row's padding
            if (has_prev && row < np) {
                const ivecV p0 = *reinterpret_cast<const ivecV *>(invsub_prev + row);
#pragma unroll
                for (int j = 0; j < V; ++j) moff[g * V + j] = p0[j];
            }
        }
    }
    float *mt_lane = FUSED ? mt : mt + row_lo;  // wave-uniform; the lane's part is added by the store
    panel_steps<NT, RPT, W, MULTI, FUSED>(a, npl, moff, sh, wave_u, c0, true, singular, pg, mt_lane, mtld,
                                          std::make_integer_sequence<int, W>{});
    // The thread index, recomputed behind an opaque instruction: everything the epilogue addresses hangs on it, so
    // hipcc cannot compute those addresses in front of the steps and carry them through (it spilled them).
    int tid_e;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(tid_e));
    tid_e += wave_u * 64;
    int pos[RPT];  // final position of every register row
#pragma unroll
    for (int k = 0; k < RPT; ++k) pos[k] = (int)(npl[k] ^ (unsigned)((int)npl[k] >> 31));

    // -- for the rows above the block (update(s) computes their G_s): the W normalised pivot rows, and the
    //    pivot rows of s-1 restricted to this sub-panel's columns
    __syncthreads();
    MI32_PSTAMP(A.tag_base, 48);
    float *aux = A.aux_out + (size_t)b * kAuxFloats;
    if constexpr (TRI) {
        // one wave completes the pivot rows left of their pivots (tri_left_rows) and exports them; the others are
        // on their way to the map stores
        if (wave_u == 0) {
            const int c = tid_e < W ? tid_e : W - 1;
            const float diag = sh.prn_all[c][c];
            float pl[W];  // pl[m] = prn_m[c]: the diagonal to start with, the rows below it as they are found
#pragma unroll
            for (int m = 0; m < W; ++m) pl[m] = (m == c) ? diag : 0.0f;
            tri_left_rows<W>(pl, sh.raw, c, std::make_integer_sequence<int, W>{});
            if (tid_e < W) {
#pragma unroll
                for (int m = 1; m < W; ++m)
                    if (c < m) sh.prn_all[m][c] = pl[m];
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            for (int i = tid_e; i < W * W; i += 64) aux[i] = sh.prn_all[i / W][i % W];
        }
    } else if (grp == 0) {
        for (int i = tid_e; i < W * W; i += NT) {
            aux[i] = sh.prn_all[i / W][i % W];
            if (has_prev) aux[kMaxW * kMaxW + i] = sh.uprev[i / W][i % W];
        }
    }
    // -- the row maps; panels with full steps: G_s too, by label at entry (order after s-1: what update(s) reads the
    //    working copy in).  Triangular steps leave G_s to the update tiles: it is a function of Mt_s and aux.
    [[maybe_unused]] float *gt = A.gt_out + (size_t)b * A.tstride;
    int *submap = A.submap_out + (size_t)b * np;
    int *invsub = A.invsub_out + (size_t)b * np;
    // positions retired since this map buffer was last written: identity (any earlier position already is)
    if (grp == 0 && tid_e < 4 * kMaxW && row_lo - 4 * kMaxW + tid_e >= 0)
        submap[row_lo - 4 * kMaxW + tid_e] = row_lo - 4 * kMaxW + tid_e;
#pragma unroll
    for (int g = 0; g < RPT / V; ++g) {
        const int row = row_lo + panel_row<NT, RPT>(tid_e, g * V);
        if (row < np) {
            ivecV p0;  // the labels at entry, again (no registers were kept for them)
#pragma unroll
            for (int j = 0; j < V; ++j) p0[j] = row + j;
            if (has_prev) p0 = *reinterpret_cast<const ivecV *>(invsub_prev + row);
            if constexpr (!TRI) {
                bool contiguous = (p0[0] % V) == 0;
#pragma unroll
                for (int j = 1; j < V; ++j) contiguous = contiguous && (p0[j] == p0[0] + j);
                if (contiguous) {
#pragma unroll
                    for (int c = 0; c < W; ++c) {
                        vecV v;
#pragma unroll
                        for (int j = 0; j < V; ++j) v[j] = a[g * V + j][c];
                        *reinterpret_cast<vecV *>(gt + (size_t)c * np + p0[0]) = v;
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < W; ++c)
#pragma unroll
                        for (int j = 0; j < V; ++j) gt[(size_t)c * np + p0[j]] = a[g * V + j][c];
                }
            }
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const int k = g * V + j;
                submap[pos[k]] = p0[j];  // position pos[k] now holds what lies at index p0[j] of the order after s-1
                invsub[p0[j]] = pos[k];
                rowsrc[pos[k]] = s_park[k * NT + tid_e];
                orig[pos[k]] = s_park[(RPT + k) * NT + tid_e];
            }
        }
    }
    // only the wave that won a step has looked at that step's pivot: any wave may raise the flag
#ifdef MI32_PANEL_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    MI32_PSTAMP(A.tag_base, 49);
    if (g_panel_stamps && threadIdx.x == 0 && blockIdx.x == 0) {
        unsigned long long *q = g_panel_stamps + (size_t)(A.tag_base & 1023u) * 64;
        q[50] = __builtin_amdgcn_s_memrealtime();
        q[51] = ((unsigned long long)NT << 32) | ((unsigned)RPT << 16) | ((unsigned)(FUSED ? 1 : 0) << 8) | (unsigned)W;
        q[52] = (unsigned long long)(np - row_lo);
    }
#endif
    // (atomicMax: a later "singular" must not hide "a partner workgroup never showed up")
    if (singular && lane == 0 && A.status) atomicMax(&A.status[b], (int)MI32_SINGULAR);
    if (pg.timed_out && lane == 0 && A.status) atomicMax(&A.status[b], (int)MI32_RUNTIME_ERROR);
}

}  // namespace mi32
