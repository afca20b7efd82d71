// mi32_blocked_internal.h -- what more than one file of the blocked fp32 path needs (gfx950 only): the constants, the
// argument structs of the launches and the host helpers of the launchers (mi32_blocked.hip's header comment maps the files).
#pragma once
#include <mutex>
#include <set>
#include <type_traits>
#include <utility>

#include "mi32_internal.h"

namespace mi32 {

typedef float float16v __attribute__((ext_vector_type(16)));

// k-tile depth and waves/SIMD of the rank-bw update (mi32_rank_bw.h)
static constexpr int kBwBK = 16;
static constexpr int kBwWPS = 3;
// (kMaxBW, kMaxW, kMaxPanelGroups, kPanelGroupRows and kFusedRows: beside the route, mi32_internal.h)
static constexpr int kXchGranules = 2 * kMaxPanelGroups * 32;  // 8-byte granules per matrix: [parity][group][32]
// how long a workgroup of a shared panel waits for a partner's record before it gives the matrix up
// (MI32_RUNTIME_ERROR, output poisoned with NaN): 0.25 s of the 100 MHz s_memrealtime clock
static constexpr unsigned long long kPanelXchTimeoutTicks = 25000000ull;
static constexpr int kAuxFloats = 2 * kMaxW * kMaxW;  // per matrix and sub-panel: what a panel leaves for the rows above the block

// Where a wide kernel exports freshly computed columns for the panel workgroup: columns
// [col, col + w * count) go to `count` consecutive compact panels (w columns each) starting at `base`.
struct PanelExport {
    float *base;     // first compact panel, matrix 0
    size_t bstride;  // floats between consecutive compact panels
    int col, w, count;
};
__device__ __forceinline__ void panel_export_store(const PanelExport &e, size_t tstride, int b, int np, int col, int grow,
                                                   float v)
{
    const int idx = col - e.col;
    if ((unsigned)idx < (unsigned)(e.w * e.count))
        e.base[(size_t)(idx / e.w) * e.bstride + (size_t)b * tstride + (size_t)(idx % e.w) * np + grow] = v;
}

// four consecutive rows (grow4 a multiple of 4) of one exported column: one 16-byte store
__device__ __forceinline__ void panel_export_store4(const PanelExport &e, size_t tstride, int b, int np, int col,
                                                    int grow4, float v0, float v1, float v2, float v3)
{
    const int idx = col - e.col;
    if ((unsigned)idx < (unsigned)(e.w * e.count)) {
        typedef float pe_f4v __attribute__((ext_vector_type(4)));
        pe_f4v v;
        v[0] = v0; v[1] = v1; v[2] = v2; v[3] = v3;
        *reinterpret_cast<pe_f4v *>(e.base + (size_t)(idx / e.w) * e.bstride + (size_t)b * tstride +
                                    (size_t)(idx % e.w) * np + grow4) = v;
    }
}

// Everything one fused sub-panel launch needs (passed by value).
struct SubpanelArgs {
    int np, n, ld, batch;
    size_t mstride, tstride;
    // ---- panel(s): workgroup b < batch of the grid (absent when panel_on == 0)
    int panel_on;
    int c0;        // first column of sub-panel s
    int has_prev;  // update(s-1) is still pending on this sub-panel's columns: apply it in the prologue
    int c0_prev;   // first column of sub-panel s-1
    int row_lo;    // the workgroup holds the rows [row_lo, np) of its input order
    int first_in_block;
    const float *pt_in;      // Pt_s: this sub-panel's columns, updates up to s-2 applied, order after s-2
    const float *mt_prev;    // Mt_{s-1}: the multipliers of sub-panel s-1, same order
    float *gt_out;           // Gt_s, order after s-1 (not written by a panel with triangular steps: panel_tri, mi32_internal.h)
    float *mt_out;           // Mt_s: the multipliers of this sub-panel's W steps (fused: order after s-1; else slab order = the same)
    size_t mtstride; int mtld;
    const int *submap_prev;  // submap of sub-panel s-1: position after s-1 -> index in order after s-2
    const int *invsub_prev;  // index in order after s-2 -> position after s-1 (the row's label at entry)
    int *submap_out;         // position after s -> index in order after s-1
    int *invsub_out;         // its inverse
    const int *rowsrc_in;    // position after s-1 -> row index at the start of the block
    int *rowsrc_out;         // the same after s (fused blocks: the other buffer -- update(s-1) still reads rowsrc_in)
    int *rowsrc_alt;         // fused blocks, first sub-panel: the second buffer, whose rows above the block are set too
    int *orig;
    float *aux_out;          // [kAuxFloats] per matrix: normalised pivot rows of s; U_{s-1} x columns of s
    int *status;
    const int *guard;        // non-null for plans with shared panels: status words; a matrix flagged
                             // MI32_RUNTIME_ERROR (a panel lost a partner: its row maps are not to be trusted)
                             // is skipped by every later launch and comes out as NaN
    int ngroups;             // workgroups per panel (> 1: MULTI instances, kPanelGroupRows rows each)
    unsigned long long *xch; // [batch][kXchGranules] exchange granules of the multi-workgroup panels
    unsigned tag_base;       // unique per panel launch within a call
    // ---- update(t), t = s-1: the other workgroups (absent when upd_on == 0)
    int upd_on;
    int u_c0;        // first column of sub-panel t
    int u_has_prev;  // sub-panel t itself had a pending update (t >= 1 within its block)
    int u_above_hi;  // positions below this were not in panel(t): their G_t is computed by the update tile
    int u_panel_hi;  // ... and positions from this on neither (np with pivoting; no-pivot variant: only the W pivot rows
                     // go through the "panel", gj_diag_panel_kernel)
    int C0, kb;      // the outer block
    const float *x;  // working copy in order after t-1
    float *y;        // working copy written in order after t
    const float *u_gt;     // Gt_t
    int u_tri;             // panel(t) ran triangular steps (panel_tri): it wrote no Gt_t, the column-tile-0 tiles
                           // compute G_t of its rows from Mt_t and aux_t
    const float *u_mt;     // Mt_t
    const int *u_rowsrc;   // position after t -> row index at the start of the block
    float *u_mf;           // the block's negated multipliers by block-start row index, [np][mf_ld]
    size_t mfstride; int mf_ld;
    const int *u_submap;   // submap_t
    const float *u_pt_in;  // Pt_t (for the rows above the block)
    const float *u_aux;    // aux_t
    PanelExport u_exp;     // the columns of sub-panel t+2 -> its compact panel input
    int upd_wgs;           // workgroups of the launch that run update tiles
    // ---- strip(t) of the columns outside the block (absent when os_on == 0): uses the u_ fields of sub-panel t
    int os_on;
    int os_first, os_ntiles;  // the tiles' columns: os_ntiles x 64 from os_first on (os_first == 0: the block's own are skipped)
    const float *os_cur;   // the working copy the columns outside the block are still valid in
    float *os_ub, *os_xs;  // the block's u rows / its pivot rows after their own sub-panel, kb x np each
    size_t ubstride;
    int drop_groups;       // tests only: panel workgroups left out of a multi-workgroup panel launch
};

// gj_block_strip_kernel's parameters (the block's strips, sub-panels [g_lo, g_hi), for the columns outside the block
// that lie in [col_lo, col_hi) (inside) / that do not)
struct BlockStripArgs {
    const float *src; size_t mstride; int np, ld;
    const float *mf; size_t mfstride; int mf_ld;
    float *ub, *xs, *xst; size_t ubstride;
    int C0, kb;
    const int *map;
    int col_lo, col_hi, inside, g_lo, g_hi;
    const int *guard;
};

// What the launches of a block's rank-bw update share (filled once per block): the multiplier transposition, the update
// of all columns outside the block (whole, or the persistent look-ahead half) and the update of the next block's columns.
struct RankUpdateArgs {
    const float *src; float *dst;  // the working copy every column outside the block is valid in, and the one written
    const float *panel;            // the working copy that holds the block's own columns (copy_panel: dst takes them)
    int copy_panel;
    size_t mstride; int np, ld;    // floats per matrix in src / dst / panel
    const float *mf; size_t mfstride; int mf_ld;  // the block's negated multipliers by block-start row index
    float *gk; size_t gkstride;    // ... transposed and in final row order (floats per matrix in gk / ub / xs)
    const float *ub, *xs;
    int C0, kb, w;                 // the outer block and its sub-panel width
    const int *map;                // position after the block -> row index at its start
    size_t tstride;
    const int *guard;
};

// f(std::integral_constant<int, V>{}) for the V of Vs that equals v: a run-time value as a template argument
template <int... Vs, class F>
static hipError_t with_constant(int v, F &&f)
{
    hipError_t e = hipErrorInvalidValue;
    (void)((v == Vs && ((e = f(std::integral_constant<int, Vs>{})), true)) || ...);
    return e;
}

// Raises a kernel's dynamic-LDS limit to `bytes`, once per device (function attributes are per device; any thread may
// be the first to launch).
inline hipError_t raise_lds_limit(const void *kernel, size_t bytes)
{
    static std::mutex mu;
    static std::set<std::pair<const void *, int>> done;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(mu);
    if (done.count({kernel, dev})) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) done.insert({kernel, dev});
    return e;
}

}  // namespace mi32
