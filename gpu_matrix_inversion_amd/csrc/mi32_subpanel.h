// mi32_subpanel.h -- gj_subpanel_kernel of the blocked fp32 path (gfx950 only), the one launch per sub-panel, with the
// list of its instances and their launcher.
#pragma once
#include "mi32_panel.h"
#include "mi32_update_tile.h"

namespace mi32 {

// ---- one launch per sub-panel: panel(s) || update(s-1) || strip(s-1) ------------------------------
template <int NT, int RPT, int W, bool FUSED>
constexpr size_t subpanel_lds_bytes(bool with_strip_tiles = true)
{
    const size_t pb =
        panel_shared_bytes<NT / 64, W, panel_tri(NT, RPT, W, false, FUSED)>() + (size_t)2 * RPT * NT * sizeof(int);
    const size_t ub = FUSED ? sizeof(UpdateTileShared<W>) * (NT / 256) : 0;
    const size_t ob = with_strip_tiles ? sizeof(OStripShared<W>) * (NT / 256) : 0;  // (they cost the update tiles occupancy)
    const size_t m = pb > ub ? pb : ub;
    return m > ob ? m : ob;
}

// Workgroups [0, batch) (where panel_on) are the panels of sub-panel s; FUSED: the next A.upd_wgs are the update
// tiles of sub-panel s-1 (NT / 256 tiles each); the rest are strip tiles of sub-panel s-1 (NT / 256 each).
template <int NT, int RPT, int W, bool FUSED>
__global__ __launch_bounds__(NT) void gj_subpanel_kernel(SubpanelArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char sp_smem[];
    const int npanel = A.panel_on ? A.batch : 0;
    int u = (int)blockIdx.x;
    if (u < npanel) {
        panel_body<NT, RPT, W, FUSED, false>(A, u, 0, sp_smem);
        return;
    }
    u -= npanel;
    if constexpr (FUSED) {
        if (u < A.upd_wgs) {
            inblock_update_body<W, NT / 256>(A, u, sp_smem);
            return;
        }
        u -= A.upd_wgs;
    }
    const int grp = threadIdx.x >> 8;
    ostrip_body<W>(A, u * (NT / 256) + grp, sp_smem + (size_t)grp * sizeof(OStripShared<W>), threadIdx.x & 255);
}

// The instances of gj_subpanel_kernel: every panel geometry plan_route can give a block -- one row per lane at
// 256 threads; at 512 threads at most 8 rows per lane and 128 floats of slab, at 1024 threads at most 64 floats
// (three rows per lane: at 1024 threads only).
constexpr bool subpanel_instance(int nt, int rpt, int w, bool fused)
{
    const bool fits = nt == 256 ? rpt == 1 : nt == 512 ? (rpt != 3 && rpt <= 8 && rpt * w <= 128) : rpt * w <= 64;
    return fits && (!fused || nt * rpt <= kFusedRows);
}

template <int NT, int RPT, int W, bool FUSED>
static hipError_t launch_subpanel(const SubpanelArgs &A, int nwgs, hipStream_t stream)
{
    if constexpr (!subpanel_instance(NT, RPT, W, FUSED)) {
        return hipErrorInvalidValue;
    } else {
        constexpr size_t lds = subpanel_lds_bytes<NT, RPT, W, FUSED>();
        if (lds > 48 * 1024) {  // more dynamic LDS than the default limit
            const hipError_t e = raise_lds_limit((const void *)gj_subpanel_kernel<NT, RPT, W, FUSED>, lds);
            if (e != hipSuccess) return e;
        }
        const size_t lds_now = subpanel_lds_bytes<NT, RPT, W, FUSED>(A.os_on != 0);
        hipLaunchKernelGGL((gj_subpanel_kernel<NT, RPT, W, FUSED>), dim3(nwgs), dim3(NT), lds_now, stream, A);
        return hipSuccess;
    }
}

}  // namespace mi32
