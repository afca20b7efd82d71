// mi32_blocked.hip -- blocked Gauss-Jordan with delayed rank-k updates on the
// fp32 matrix cores (gfx950: v_mfma_f32_32x32x2_f32).
//
// Same elimination as mi32_sweep.hip (and as the reference's step loop,
// /root/reference/Matlab/mat_inv_32/mat_inv_32/mat_inv_32.cpp:317-362), with the
// column updates of a block of pivots delayed:
//
//   for each outer block K = [C0, C0+kb) of pivot columns:
//     for each sub-panel s, Ks = [c0, c0+W) of K:
//       panel(s)   -- ONE workgroup per matrix holds the rows that can still be
//                     chosen as pivots, W columns each, in registers and runs the W
//                     pivot steps on them: column arg-max (DPP + one LDS atomic), row
//                     swap (= exchange of two position labels), IEEE-division
//                     normalise, eliminate.  Result: G_s = the W transformed columns
//                     (the inverse columns of these pivots) and the multipliers f_m[i] of
//                     its steps (the entry row i had in the pivot column when step m ran).
//       update(s)  -- every other column j of the block, 64-column tiles: the tile's W pivot
//                     rows run the W steps alone (the strip: u_m[j] = pivot row of step m over
//                     its pivot, W dependent IEEE divisions), then every other row takes
//                     M[i][j] = fmaf(-f_m[i], u_m[j], M[i][j]), m ascending, as ONE chain from
//                     its old value (v_mfma_f32_32x32x2_f32 with the old value as C operand):
//                     the reference's own operation order.
//       strip(s)   -- the columns outside the block: only their W pivot rows, which first
//                     take the block's earlier steps; u_m is kept (ub) for the rank-bw update.
//     rank-bw update (K = kb, mi32_rank_bw.h) -- every column outside the block: the same
//                     chain from the old value over all kb steps, A = the block's multipliers,
//                     B = u.
//
// strip(s-1) rides in the launch of panel(s).  In blocks of at most kFusedRows rows,
// panel(s) and update(s-1) are ONE launch too (gj_subpanel_kernel: workgroup 0 of a
// matrix is the panel, the others are update tiles): update(s-1) no longer sits
// between two panels on the critical path of the N pivot steps.  What panel(s)
// needs from update(s-1) -- its own W columns -- it computes itself in a prologue
// (the same k-ascending fmaf chain the MFMA update runs), from the panel input
// that update(s-2) exported one launch earlier.
//
// Row swaps are never applied as data movement of their own: the updates read
// their C rows and their B (pivot-row) operand THROUGH a row map and write
// out-of-place into the second working copy, so swap + snapshot + update are
// one launch and no launch has a read-after-write hazard between workgroups.
// The two working copies alternate roles exactly like the reference's
// ping-pong buffers (mat_inv_32.cpp:318,353-360).
//
// The panel workgroup only ever touches COMPACT, TRANSPOSED panels: it reads
// Pt[c][row] (W x np, exported by whichever wide kernel produced those columns)
// and writes Gt[c][row], with coalesced accesses.  (Letting the one workgroup
// gather 64-byte chunks of np rows itself cost 18 us per launch, more than its 16
// pivot steps.)
//
// Row orders.  "Order after t" = the rows arranged by the position they hold after
// sub-panel t's swaps.  update(t) writes the working copy and its exports in order
// after t.  panel(s) therefore receives its input Pt_s (exported by update(s-2)) in
// order after s-2 and the previous panel's output Gt_{s-1} in that same order;
// what it needs on top is every row's position after s-1, its label at entry
// (invsub_{s-1}).  It writes Gt_s by those labels, i.e. in order after s-1, which
// is the order update(s) reads the working copy in.
//
// The working matrix is the N x N in-place form (see mi32_sweep.hip), padded
// with an identity block to a multiple of 128 so that no tile needs bounds
// checks: inv(diag(I, A)) = diag(I, inv(A)).  The padding comes FIRST (rows and
// columns [0, np - n)), so its steps run while every entry is finite -- pivot 1,
// multipliers 0, exact no-ops -- and its rows are retired before the first real
// step: a padded row still takes fmaf(-0, u, 0) in the real steps (NaN where an
// overflowed pivot row holds an infinity), but nothing reads it any more.  With
// the padding behind the matrix those NaNs came back through the padded steps
// and an inverse that overflows lost its infinities to NaN, column by column.
//
// Where things are.  How a call runs -- blocking, sub-panel widths, fused blocks, shared panels, look-ahead, split,
// where the strips go -- is decided in mi32_plan.hip (plan_route) and arrives as a BlockedRoute (mi32_internal.h).  This
// file is the translation unit of every kernel of the path: the workspace layout, the init and un-permute kernels and
// the schedule (blocked_invert), which walks the route and launches everything else through the launchers of
//   mi32_blocked_subpanel.h          once per sub-panel: dispatch_subpanel, the multi-workgroup panel, the in-block update
//                                    alone, the no-pivot variant's diagonal panel; the test and diagnostic hooks
//   mi32_blocked_block.h             once per block: the block's strips in one launch, the multiplier transposition, the
//                                    rank-bw update (mi32_rank_bw.h) and the update of the next block's columns alone
// on top of
//   mi32_subpanel.h                  gj_subpanel_kernel: panel(s) || update(s-1) || strip(s-1), its instances
//   mi32_panel.h                     panel(s): the pivot step and the panel workgroup's body
//   mi32_update_tile.h               update(t) and strip(t): the 64-column tiles of the sub-panel launches
//   mi32_strip.h, mi32_dpp.h         the pivot-row strip; DPP reductions and row helpers
//   mi32_blocked_internal.h          constants, the launches' argument structs, host helpers
#include "mi32_blocked_block.h"
#include "mi32_blocked_subpanel.h"
#include "mi32_det_large.h"

namespace mi32 {

// (the update tiles address a matrix with 32-bit byte offsets from its base: mi32_rank_bw.h, inblock_update_body)
static_assert(16384ull * (16384 + 64) * sizeof(float) < (1ull << 32), "a working copy must stay below 4 GiB");

struct BlockedWs {
    float *m0, *m1;     // the two working copies, np x ld each
    float *pt[3];       // compact transposed panel inputs, kMaxW x np each: sub-panel s of a block uses pt[s % 3]
    float *gt[2];       // compact transposed panel outputs G_s (the new values of the sub-panel's own columns): gt[s & 1]
    float *mt[2];       // compact transposed MULTIPLIERS of sub-panel s, kMaxW x mtld each: mt[s & 1]
    float *aux[2];      // per sub-panel, kAuxFloats per matrix: the W normalised pivot rows; the previous sub-panel's
                        // pivot rows as its steps saw them (U_{s-1}) restricted to this sub-panel's columns; the W x W
                        // multipliers of the sub-panel's own pivot rows
    unsigned long long *xch;  // exchange granules of the multi-workgroup panels, kXchGranules per matrix
    float *mf[2];       // the block's NEGATED multipliers, np x bw row-major BY BLOCK-START ROW INDEX (never permuted);
                        // double-buffered across blocks (the look-ahead half reads block b's while block b+1 runs)
    float *ub[2];       // the block's pivot rows as their own steps saw them (U), bw x np: B operand of the rank-bw update
    float *xs[2];       // the block's pivot rows after their own sub-panel's last step, bw x np: where their
                        // accumulation starts in the rank-bw update
    float *xst;         // gj_block_strip_kernel: the pivot rows of the groups a call leaves to the next one
    float *gk;          // the block's multipliers transposed and in final row order, bw x np: its A operand
    size_t gkstride;    // floats per matrix in gk / ub
    size_t mfstride;    // floats per matrix in mf
    int *submap[2], *invsub[2];  // per sub-panel: position after s -> index in order after s-1, and its inverse
    int *rowsrc[4], *orig, *invp;  // rowsrc[2 * (blk & 1) + (fused ? s & 1 : 0)]: double-buffered across blocks
                                   // (look-ahead) and, in fused blocks, across sub-panels (update(s-1) reads the map
                                   // panel(s) rewrites in the same launch)
    size_t mstride;     // floats per matrix in m0/m1
    size_t tstride;     // floats per matrix in pt/gt
    size_t mtstride;    // floats per matrix in mt
    int mtld;           // row stride of mt: every register row of a panel workgroup has a slot (rows >= np too)
    size_t pt_bstride;  // floats between pt[i] and pt[i + 1]: the kernels address the three as one array (PanelExport)
    size_t ibytes;      // bytes of each index map (submap ... invp)
};
static size_t blocked_carve(const BlockedRoute &p, int batch, void *base, BlockedWs &o, WsRegions *regions = nullptr)
{
    static const char *const kPt[] = {"pt0", "pt1", "pt2"}, *const kGt[] = {"gt0", "gt1"}, *const kMt[] = {"mt0", "mt1"},
                             *const kAux[] = {"aux0", "aux1"}, *const kUb[] = {"ub0", "ub1"}, *const kXs[] = {"xs0", "xs1"},
                             *const kMf[] = {"mf0", "mf1"}, *const kSubmap[] = {"submap0", "submap1"},
                             *const kInvsub[] = {"invsub0", "invsub1"},
                             *const kRowsrc[] = {"rowsrc0", "rowsrc1", "rowsrc2", "rowsrc3"};
    const size_t mbytes = align256((size_t)p.np * p.ld * sizeof(float));
    const size_t tbytes = align256((size_t)kMaxW * p.np * sizeof(float));
    const size_t ibytes = align256((size_t)p.np * sizeof(int) * batch);
    const size_t abytes = align256((size_t)kAuxFloats * sizeof(float) * batch);
    const int mtld = 2 * p.np + 256;  // row_lo + NT * RPT <= 2 np + 256 for every panel geometry
    const size_t mtbytes = align256((size_t)kMaxW * mtld * sizeof(float));
    const size_t gkbytes = align256((size_t)(p.bw < kMaxBW ? p.bw : kMaxBW) * p.np * sizeof(float));
    const size_t mfbytes = align256((size_t)p.np * p.bw * sizeof(float));
    o.mstride = mbytes / sizeof(float);
    o.tstride = tbytes / sizeof(float);
    o.mtstride = mtbytes / sizeof(float);
    o.mtld = mtld;
    o.gkstride = gkbytes / sizeof(float);
    o.mfstride = mfbytes / sizeof(float);
    o.ibytes = ibytes;
    WsCarver c(base, regions);
    o.m0 = c.take<float>(mbytes * batch, WS_VALUES, "m0");
    o.m1 = c.take<float>(mbytes * batch, WS_VALUES, "m1");
    for (int i = 0; i < 3; ++i) o.pt[i] = c.take<float>(tbytes * batch, WS_VALUES, kPt[i]);
    // what lies between two of them, a red zone of the guard mode included: the carver's own step
    o.pt_bstride = (tbytes * batch + c.guard) / sizeof(float);
    for (int i = 0; i < 2; ++i) o.gt[i] = c.take<float>(tbytes * batch, WS_VALUES, kGt[i]);
    for (int i = 0; i < 2; ++i) o.mt[i] = c.take<float>(mtbytes * batch, WS_VALUES, kMt[i]);
    for (int i = 0; i < 2; ++i) o.aux[i] = c.take<float>(abytes, WS_VALUES, kAux[i]);
    o.xch = c.take<unsigned long long>(align256((size_t)kXchGranules * sizeof(unsigned long long) * batch), WS_RECORDS, "xch");
    o.gk = c.take<float>(gkbytes * batch, WS_VALUES, "gk");
    for (int i = 0; i < 2; ++i) {
        o.ub[i] = c.take<float>(gkbytes * batch, WS_VALUES, kUb[i]);
        o.xs[i] = c.take<float>(gkbytes * batch, WS_VALUES, kXs[i]);
    }
    o.xst = c.take<float>(gkbytes * batch, WS_VALUES, "xst");
    for (int i = 0; i < 2; ++i) o.mf[i] = c.take<float>(mfbytes * batch, WS_VALUES, kMf[i]);
    for (int i = 0; i < 2; ++i) o.submap[i] = c.take<int>(ibytes, WS_INDICES, kSubmap[i]);
    for (int i = 0; i < 2; ++i) o.invsub[i] = c.take<int>(ibytes, WS_INDICES, kInvsub[i]);
    for (int i = 0; i < 4; ++i) o.rowsrc[i] = c.take<int>(ibytes, WS_INDICES, kRowsrc[i]);
    o.orig = c.take<int>(ibytes, WS_INDICES, "orig");
    o.invp = c.take<int>(ibytes, WS_INDICES, "invp");
    return c.off;
}
size_t blocked_workspace_bytes(const BlockedRoute &r, int batch, WsRegions *regions)
{
    BlockedWs ws;
    return blocked_carve(r, batch, nullptr, ws, regions);
}

// ---- init: A -> diag(I, A) in the first working copy (makeAugmentedMatrix counterpart,
//      mat_inv_32.cpp:177-192) + the compact copies of the first two sub-panels' columns ------
__global__ __launch_bounds__(256) void blocked_init_kernel(const float *__restrict__ in, int n, int np, int ld,
                                                            size_t mstride, float *__restrict__ m0, PanelExport ex,
                                                            size_t tstride, int *__restrict__ orig,
                                                            int *__restrict__ status)
{
    const int b = blockIdx.z;
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int i0 = blockIdx.y * 16;
    const float *a = in + (size_t)b * n * n;
    float *m = m0 + (size_t)b * mstride;
    const int pad = np - n;  // the identity padding comes first
    bool nonfinite = false;  // boundary rule: a NaN / inf anywhere in the input is an invalid matrix
    if (j < np) {
#pragma unroll 4
        for (int u = 0; u < 16; ++u) {
            const int i = i0 + u;
            if (i >= np) break;
            float v;
            if (i >= pad && j >= pad) v = a[(size_t)(i - pad) * n + (j - pad)];
            else v = (i == j) ? 1.0f : 0.0f;
            nonfinite = nonfinite || (v - v != 0.0f);
            m[(size_t)i * ld + j] = v;
            panel_export_store(ex, tstride, b, np, j, i, v);
        }
    }
    if (blockIdx.y == 0 && j < np) orig[(size_t)b * np + j] = j;
    // status[b] was zeroed (MI32_OK) by the host before this launch; every writer stores the same value
    if (nonfinite && status) status[b] = MI32_SINGULAR;
}

// ---- getInvertedMatrix counterpart: undo the column permutation ----------------
// Whole rows go through LDS: the global read (all np columns of R rows) and the global write (n columns)
// are both coalesced; the column gather happens inside LDS.  (A direct gather from global memory read
// 4 scattered bytes per lane: 1.35 ms for 64 x 2048^2, i.e. 1.5 TB/s.)
__global__ __launch_bounds__(256) void unpermute_columns_ld_kernel(const float *__restrict__ w_all, int ld, int np,
                                                                    size_t wstride, const int *__restrict__ invp,
                                                                    int istride, int n, int rows_per_block,
                                                                    float *__restrict__ out,
                                                                    const int *__restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) float s_rows[];  // [rows_per_block][np]
    const int b = blockIdx.y;
    const int tid = threadIdx.x;
    const float *w = w_all + (size_t)b * wstride;
    float *o = out + (size_t)b * n * n;
    const int i0 = blockIdx.x * rows_per_block;
    const int nr = (n - i0 < rows_per_block) ? (n - i0) : rows_per_block;
    const int pad = np - n;  // the matrix lies behind the identity padding: rows and columns [pad, np)
    // a matrix whose shared panel lost a partner workgroup went on with stale data: hand out NaN, not numbers
    if (status != nullptr && __builtin_amdgcn_readfirstlane(status[b]) == MI32_RUNTIME_ERROR) {
        for (int r = 0; r < nr; ++r)
            for (int j = tid; j < n; j += 256) o[(size_t)(i0 + r) * n + j] = __builtin_nanf("");
        return;
    }
    for (int r = 0; r < nr; ++r)
        for (int c4 = tid * 4; c4 < np; c4 += 1024)
            *reinterpret_cast<float4 *>(&s_rows[(size_t)r * np + c4]) =
                *reinterpret_cast<const float4 *>(w + (size_t)(pad + i0 + r) * ld + c4);
    __syncthreads();
    for (int j = tid; j < n; j += 256) {
        const int c = invp[(size_t)b * istride + pad + j];
        for (int r = 0; r < nr; ++r) o[(size_t)(i0 + r) * n + j] = s_rows[(size_t)r * np + c];
    }
}

// Look-ahead: the rank-bw update of block b is split into (A) the columns of block b+1, which the next
// panel phase needs at once, and (B) all other columns.  (A) stays on the main stream; (B) runs on a
// second stream and overlaps with block b+1's panel phase, which is latency bound on a few CUs.  The
// next rank-bw update (and the final un-permutation) wait for (B) through an event.
hipError_t blocked_invert(const BlockedRoute &p, int part, const float *d_a, float *d_inv, int *d_status, void *wsp,
                          const BlockedExec &ex, const DetRec &det)
{
    const int batch = p.part_batch[part];
    const bool lookahead = p.lookahead;  // (never for a half of a split batch: plan_route)
    if (lookahead && (ex.aux == nullptr || ex.n_events < 4 || ex.aux_workgroups <= 0)) return hipErrorInvalidValue;
    BlockedWs ws;
    blocked_carve(p, batch, wsp, ws);
    const int np = p.np;
    hipStream_t stream = ex.stream;
    Profiler *prof = ex.prof;
    hipError_t e;
    const PanelExport no_export = {ws.pt[0], ws.pt_bstride, -(1 << 30), 1, 0};
    if (d_status) {  // MI32_OK; the init kernel flags non-finite input, the panels bad pivots and lost partners
        if ((e = hipMemsetAsync(d_status, 0, sizeof(int) * (size_t)batch, stream)) != hipSuccess) return e;
    }
    {
        // the first two sub-panels of the first block are exported as they are: the first has no pending
        // update at all, the second gets the first one's update in its panel's prologue
        ProfScope ps(prof, KC_INIT, stream);
        const PanelExport ex0 = {ws.pt[0], ws.pt_bstride, 0, (int)p.wblk[0], p.fused(0) ? 2 : 1};
        hipLaunchKernelGGL(blocked_init_kernel, dim3((np + 255) / 256, (np + 15) / 16, batch), dim3(256), 0, stream,
                           d_a, p.n, np, p.ld, ws.mstride, ws.m0, ex0, ws.tstride, ws.orig, d_status);
    }
    if (lookahead) {  // whatever still runs on the second stream from an earlier call shares this workspace
        if ((e = hipEventRecord(ex.events[0], ex.aux)) != hipSuccess) return e;
        if ((e = hipStreamWaitEvent(stream, ex.events[0], 0)) != hipSuccess) return e;
    }
    // dynamic LDS of the rank-bw kernels: operand stages + maps; the persistent flavour asks for more than half
    // a CU's LDS so that at most one of its workgroups is resident per CU
    // "exclusive": nearly all of a CU's LDS, so that no workgroup of the main stream fits beside a look-ahead workgroup.
    // The dispatcher deals a grid's workgroups to the XCDs and shader engines in turn and puts each on the FIRST CU of
    // its engine that has room -- with 84 KB the in-block update tiles and the small panels land on the CUs the
    // look-ahead half keeps busy although whole CUs are idle (in-block update 12.2 instead of 6.4 us while the half
    // runs).  Where the half is short against the panel phase (up to ~8192 rows) it gets fewer CUs, all to itself.
    const size_t lds_persistent = (ex.aux_exclusive ? 156 : 84) * 1024;
    if ((e = raise_lds_limit((const void *)gj_rank_bw2_kernel<kBwBK, kBwWPS>, rank_bw2_lds_bytes<kBwBK>(kMaxBW))) != hipSuccess ||
        (e = raise_lds_limit((const void *)gj_rank_bw2_persistent_kernel<kBwBK>, 156 * 1024)) != hipSuccess ||
        (e = raise_lds_limit((const void *)gj_panel_multi_kernel<16>, subpanel_lds_bytes<1024, 4, 16, false>())) != hipSuccess)
        return e;
    // plans with shared panels (multi-workgroup panels, pivoting only): every launch skips a matrix whose panel lost
    // a partner (SubpanelArgs::guard)
    const int *guard = p.shared_panels ? d_status : nullptr;
    unsigned panel_launches = 0;  // tags of the multi-workgroup panels' exchange granules: unique per launch
    if (p.shared_panels) {  // no stale tag of an earlier call may match
        if ((e = hipMemsetAsync(ws.xch, 0, (size_t)kXchGranules * sizeof(unsigned long long) * batch, stream)) != hipSuccess)
            return e;
        // A matrix that was given up is skipped by its panels from then on, so its row maps are no longer written --
        // but where the strip(t) tiles ride in the panel launches they still run for it (ostrip_body: the 256-thread
        // groups of a workgroup share its barriers; computed, not stored) and address its rows THROUGH submap and
        // rowsrc.  Whatever an earlier call or another owner left in the workspace must not reach them: 0 is a valid
        // position.  The eight maps, ws.ibytes each (orig is the init kernel's): one memset per run of maps that lie side
        // by side -- all eight as they are carved, one each with the guard mode's red zones between them.
        int *const maps[] = {ws.submap[0], ws.submap[1], ws.invsub[0], ws.invsub[1],
                             ws.rowsrc[0], ws.rowsrc[1], ws.rowsrc[2], ws.rowsrc[3]};
        const size_t nmaps = sizeof(maps) / sizeof(maps[0]);
        for (size_t i = 0, j; i < nmaps; i = j) {
            for (j = i + 1; j < nmaps && (char *)maps[j] == (char *)maps[j - 1] + ws.ibytes; ++j) {}
            if ((e = hipMemsetAsync(maps[i], 0, ws.ibytes * (j - i), stream)) != hipSuccess) return e;
        }
    }
    const bool strips_at_end = p.part_strips_at_end[part];  // else the strip(t) tiles ride in the panel launches
    // what every sub-panel launch shares
    SubpanelArgs base = {};
    base.np = np; base.n = p.n; base.ld = p.ld; base.batch = batch;
    base.mstride = ws.mstride; base.tstride = ws.tstride;
    base.mtstride = ws.mtstride; base.mtld = ws.mtld;
    base.mfstride = ws.mfstride; base.mf_ld = p.bw;
    base.u_exp = no_export;
    base.guard = guard;
    float *cur = ws.m0, *oth = ws.m1;
    bool pending_b = false;  // a (B) half is in flight on the second stream
    int blk = 0, ev = 0;
    for (int C0 = 0; C0 < np; C0 += p.bw, ++blk) {
        const int kb = (C0 + p.bw <= np) ? p.bw : np - C0;
        int **rsb = &ws.rowsrc[2 * (blk & 1)];
        float *mf = ws.mf[blk & 1], *ub = ws.ub[blk & 1], *xs = ws.xs[blk & 1];
        // sub-panel width of this block and of the next one
        const int w = p.wblk[blk];
        const int w_next = (blk + 1 < p.nblk) ? (int)p.wblk[blk + 1] : w;
        const int S = kb / w;                                            // sub-panels of this block (even)
        // Fused mode: launch s = panel(s) || update(s-1), the panel applies update(s-1) to its own columns in a
        // prologue; the other blocks keep panel(s) and update(s) apart.
        const bool fused = p.fused(blk);
        const int os_ntiles = strips_at_end ? 0 : (np - kb) / 64;
        float *x = cur, *y = oth;  // the block's panel columns alternate between the two copies
        // Each builder fills its own fields of a launch's arguments.  panel(s): sub-panel s's pivot steps.
        auto panel = [&](SubpanelArgs &A, int s) {
            A.panel_on = 1;
            A.c0 = C0 + s * w;
            A.has_prev = fused && (s > 0);
            A.c0_prev = A.c0 - w;
            A.row_lo = A.has_prev ? A.c0_prev : A.c0;  // fused: the W pivot rows of s-1 are needed once more
            A.first_in_block = (s == 0);
            A.pt_in = ws.pt[s % 3];
            A.mt_prev = ws.mt[(s + 1) & 1];
            A.gt_out = ws.gt[s & 1];
            A.mt_out = ws.mt[s & 1];
            A.submap_prev = ws.submap[(s + 1) & 1];
            A.invsub_prev = ws.invsub[(s + 1) & 1];
            A.submap_out = ws.submap[s & 1];
            A.invsub_out = ws.invsub[s & 1];
            A.rowsrc_in = rsb[fused ? (s + 1) & 1 : 0];
            A.rowsrc_out = rsb[fused ? s & 1 : 0];
            A.rowsrc_alt = (fused && s == 0) ? rsb[1] : nullptr;
            A.orig = ws.orig;
            A.aux_out = ws.aux[s & 1];
            A.status = d_status;
            A.ngroups = p.panel_groups(np - A.row_lo);  // by the rows the panel holds
            A.xch = ws.xch;
            A.tag_base = ++panel_launches;
        };
        // what the update and the strip tiles of sub-panel t both read
        auto tile_inputs = [&](SubpanelArgs &A, int t) {
            A.u_c0 = C0 + t * w;
            A.C0 = C0; A.kb = kb;
            A.u_mt = ws.mt[t & 1];
            A.u_rowsrc = p.pivoting ? rsb[fused ? t & 1 : 0] : ws.orig;  // no pivoting: no row ever moves
            A.u_submap = p.pivoting ? ws.submap[t & 1] : ws.orig;
            A.u_mf = mf;
        };
        // update(t): the columns of the block that are not sub-panel t's own
        auto update = [&](SubpanelArgs &A, int t) {
            tile_inputs(A, t);
            A.upd_on = 1;
            A.u_has_prev = fused && (t > 0);
            A.u_above_hi = A.u_has_prev ? A.u_c0 - w : A.u_c0;  // = the first row panel(t) held
            A.u_panel_hi = p.pivoting ? np : A.u_c0 + w;
            A.x = x; A.y = y;
            A.u_gt = ws.gt[t & 1];
            A.u_tri = p.pivoting && panel_instance(p, blk, t).tri;  // panel(t) wrote no Gt_t
            A.u_pt_in = ws.pt[t % 3];
            A.u_aux = ws.aux[t & 1];
            // fused: sub-panel t+2's columns (t+1's are brought up to date by its own panel);
            // otherwise sub-panel t+1's, fully up to date
            const int tx = fused ? t + 2 : t + 1;
            if (tx < S) A.u_exp = PanelExport{ws.pt[tx % 3], ws.pt_bstride, C0 + tx * w, w, 1};
        };
        // strip(t): the columns outside the block; needs panel(t)'s output and the strips before it
        auto strip = [&](SubpanelArgs &A, int t) {
            tile_inputs(A, t);
            A.os_on = 1;
            A.os_first = 0;
            A.os_ntiles = os_ntiles;
            A.os_cur = cur;
            A.os_ub = ub; A.os_xs = xs; A.ubstride = ws.gkstride;
        };
        for (int s = 0; s <= S; ++s) {
            const int t = s - 1;
            // strip(s-1) rides in the launch of panel(s), in the block's last in-block update for the last sub-panel
            const bool with_strip = s > 0 && os_ntiles > 0;
            if (fused) {  // one launch: panel(s) || update(s-1) || strip(s-1)
                SubpanelArgs A = base;
                if (s < S) panel(A, s);
                if (s > 0) update(A, t);
                if (with_strip) strip(A, t);
                // a fused launch is accounted to the panel while there is one (it is the critical path)
                ProfScope ps(prof, A.panel_on ? KC_PANEL : KC_UPDATE_IN, stream);
                if ((e = dispatch_subpanel(p, w, A, stream)) != hipSuccess) return e;
            } else {
                if (s > 0) {  // update(s-1) first: panel(s) reads the columns it exports
                    SubpanelArgs U = base;
                    update(U, t);
                    if (with_strip && s == S) strip(U, t);
                    ProfScope ps(prof, KC_UPDATE_IN, stream);
                    if ((e = dispatch_subpanel(p, w, U, stream)) != hipSuccess) return e;
                }
                if (s < S) {
                    SubpanelArgs P = base;
                    panel(P, s);
                    if (with_strip) strip(P, t);
                    ProfScope ps(prof, KC_PANEL, stream);
                    if (!p.pivoting) {
                        // the no-pivot variant: the W x W diagonal block alone (+ the strip tiles that ride with a panel)
                        launch_diag_panel(P, stream);
                    } else if ((e = dispatch_subpanel(p, w, P, stream)) != hipSuccess) {
                        return e;
                    }
                }
            }
            if (s > 0) { float *t2 = x; x = y; y = t2; }
        }
        // A det call: the block's pivots into the per-matrix list, pivot(C0 + m) = -mf[rowsrc[C0 + m]][m].  update(t)'s
        // column-tile-0 tiles wrote the rows of mf for every sub-panel t of the block (single-block plans included), and
        // the pivot rows of t keep their positions after t.  On this stream, so in front of block blk + 2's update
        // tiles, the next writers of mf[blk & 1]; the look-ahead half only reads it.
        if (det.on()) {
            ProfScope ps(prof, KC_FINISH, stream);
            launch_det_gather(mf, ws.mfstride, p.bw, p.pivoting ? rsb[fused ? (S - 1) & 1 : 0] : ws.orig, np, C0, kb,
                              (float *)det.piv, det.pstride, batch, guard, stream);
        }
        // x now holds the block's own columns; every other column is still valid in `cur` only
        if (kb < np) {
            const int next = C0 + kb;  // first column of the next block
            const bool has_next = next < np;
            const int kb_next = has_next ? ((next + p.bw <= np) ? p.bw : np - next) : 0;
            // position after the block -> row index at its start
            const int *rowsrc = p.pivoting ? rsb[fused ? (S - 1) & 1 : 0] : ws.orig;
            // the next block's first two sub-panels, fully updated, for its first two panels
            const PanelExport exn =
                has_next ? PanelExport{ws.pt[0], ws.pt_bstride, next, w_next, p.fused(blk + 1) ? 2 : 1}
                         : no_export;
            const int copy = (x != oth) ? 1 : 0;
            if (pending_b) {  // this update reads all of `cur` and overwrites `oth`: the previous (B) must be done
                if ((e = hipStreamWaitEvent(stream, ex.events[ev], 0)) != hipSuccess) return e;
                pending_b = false;
            }
            const bool split_update = lookahead && has_next;
            // what the launches of this block's rank-bw update share
            const RankUpdateArgs ru = {cur, oth, x, copy, ws.mstride, np, p.ld, mf, ws.mfstride, p.bw, ws.gk, ws.gkstride,
                                       ub, xs, C0, kb, w, rowsrc, ws.tstride, guard};
            auto launch_transpose = [&](hipStream_t st) {  // A operand of the rank-bw update, k-major (mi32_rank_bw.h)
                ProfScope ps(prof, KC_TRANSPOSE, st);
                launch_mult_transpose(ru, batch, st);
            };
            // the block's strips in one launch, for the columns outside it in [col_lo, col_hi) (inside) / not in it
            auto launch_strips = [&](hipStream_t st, int col_lo, int col_hi, int inside) {
                ProfScope ps(prof, KC_TRANSPOSE, st);
                const BlockStripArgs a = {cur, ws.mstride, np, p.ld, mf, ws.mfstride, p.bw, ub, xs, ws.xst, ws.gkstride,
                                          C0, kb, rowsrc, col_lo, col_hi, inside, 0, S, guard};
                return launch_block_strip(w, batch, st, a);
            };
            if (split_update) {
                {   // (A): the next block's columns, on the main stream; exports the next sub-panels
                    if ((e = launch_strips(stream, next, next + kb_next, 1)) != hipSuccess) return e;
                    ProfScope ps(prof, KC_UPDATE_OUT, stream);
                    launch_rank_update_cols(ru, exn, next, kb_next, batch, stream);
                }
                // (B): everything else, on the second stream, after this block's panel phase
                ev = (ev + 1) % (ex.n_events / 2);
                hipEvent_t e_panel = ex.events[ex.n_events / 2 + ev];
                if ((e = hipEventRecord(e_panel, stream)) != hipSuccess) return e;
                if ((e = hipStreamWaitEvent(ex.aux, e_panel, 0)) != hipSuccess) return e;
                // the strips of every column the strip(t) tiles could not follow
                if ((e = launch_strips(ex.aux, next, next + kb_next, 0)) != hipSuccess) return e;
                launch_transpose(ex.aux);  // only half (B) reads the transposed multipliers: off the main stream
                {
                    ProfScope ps(prof, KC_UPDATE_OUT, ex.aux);
                    // persistent flavour: aux_workgroups (< number of CUs) workgroups, with so much dynamic LDS
                    // that one CU holds at most one of them -> the remaining CUs stay free for the main stream
                    launch_rank_bw_persistent(ru, no_export, next, next + kb_next, ex.aux_workgroups, lds_persistent, batch,
                                              ex.aux);
                }
                if ((e = hipEventRecord(ex.events[ev], ex.aux)) != hipSuccess) return e;
                pending_b = true;
            } else {
                if (strips_at_end) {  // no strip(t) tiles ran
                    if ((e = launch_strips(stream, 0, 0, 0)) != hipSuccess) return e;
                }
                launch_transpose(stream);
                ProfScope ps(prof, KC_UPDATE_OUT, stream);
                launch_rank_bw(ru, exn, batch, stream);
            }
            float *t = cur; cur = oth; oth = t;
        } else {
            cur = x;  // single block: the panel is the whole matrix
        }
    }
    if (pending_b) {
        if ((e = hipStreamWaitEvent(stream, ex.events[ev], 0)) != hipSuccess) return e;
    }
    ProfScope ps(prof, KC_FINISH, stream);
    // a det call: every exchanging step is one transposition, so their parity is the parity of the final row map
    if (det.on() && p.pivoting) launch_det_parity(ws.orig, np, batch, det.parity, guard, stream);
    if (!d_inv) return hipGetLastError();  // determinant only (det calls): nothing to un-permute
    // over ALL np entries: orig is a permutation of [0, np), so every invp[j] is defined and in range
    launch_invert_perm(ws.orig, ws.invp, np, batch, guard, stream);
    {
        int rpb = (64 * 1024) / (np * (int)sizeof(float));  // rows per workgroup: at most 64 KiB of LDS
        if (rpb < 1) rpb = 1;
        if (rpb > 8) rpb = 8;
        hipLaunchKernelGGL(unpermute_columns_ld_kernel, dim3((p.n + rpb - 1) / rpb, batch), dim3(256),
                           (size_t)rpb * np * sizeof(float), stream, cur, p.ld, np, ws.mstride, ws.invp, np, p.n, rpb,
                           d_inv, d_status);
    }
    return hipGetLastError();
}

}  // namespace mi32
