// mi32_blocked_subpanel.h -- the launches of the blocked fp32 path that happen once per sub-panel (gfx950 only):
// dispatch_subpanel picks the kernel of a launch of the sub-panel pipeline -- an instance of gj_subpanel_kernel
// (mi32_subpanel.h), the multi-workgroup panel or the in-block update alone -- and launch_diag_panel is the no-pivot
// variant's panel.  The test and diagnostic hooks of the panel code live here too.
//
// Not a translation unit of its own: mi32_blocked.hip includes it, once.  hipcc's code for the panel kernels depends on
// which other kernels share their translation unit (measured: with the per-block kernels in a unit of their own, 11
// gj_subpanel_kernel instances come out with another schedule and register allocation; with one unit per workgroup
// size, 38 kernels), and changes that only move code are accepted on an unchanged disassembly
// (tools/code_object_diff.py).
#pragma once
#include <atomic>

#include "mi32_subpanel.h"

namespace mi32 {

// ---- the no-pivot variant's "panel" (matrix_inversion_no_pivots.cpp:10: findCrr / fixRow / fixColumn, no search,
//      no swap): the W x W diagonal block alone ------------------------------------------------------------------
// Without a pivot search the W pivot rows of a sub-panel are known in advance -- rows c0 .. c0+W-1 -- and what every
// OTHER row does in the W steps depends on those rows only: it is the update tiles that take each of them through the
// steps (above_rows_step, with the normalised pivot rows this kernel exports), thousands of rows in parallel on the
// whole chip instead of one workgroup.  This kernel runs the W steps on the W x W block of the pivot rows themselves
// (one thread per entry, two LDS hand-overs per step) and leaves what the panel kernel leaves for its rows: their new
// entries (gt), their multipliers (mt; own step: the pivot), the normalised pivot rows (aux) and the status.
// Workgroups past the matrices are strip(t) tiles, as in the other panel launches.
template <int W>
__global__ __launch_bounds__(256) void gj_diag_panel_kernel(SubpanelArgs A)
{
    constexpr size_t kBytes = sizeof(OStripShared<W>) > (3 * W * W + 2 * W) * sizeof(float) ? sizeof(OStripShared<W>)
                                                                                          : (3 * W * W + 2 * W) * sizeof(float);
    __shared__ __attribute__((aligned(16))) unsigned char dp_smem[kBytes];
    if ((int)blockIdx.x >= A.batch) {
        ostrip_body<W>(A, (int)blockIdx.x - A.batch, dp_smem, threadIdx.x);
        return;
    }
    float *s_d = reinterpret_cast<float *>(dp_smem);  // [W][W] the block
    float *s_prn = s_d + W * W;                       // [W][W] normalised pivot rows
    float *s_mt = s_prn + W * W;                      // [W][W] multipliers [step][row]
    const int b = blockIdx.x, tid = threadIdx.x, np = A.np, c0 = A.c0;
    if (matrix_given_up(A.guard, b)) return;
    const float *pt = A.pt_in + (size_t)b * A.tstride;
    for (int i = tid; i < W * W; i += 256) s_d[i] = pt[(size_t)(i % W) * np + c0 + i / W];  // s_d[row][col]
    __syncthreads();
    bool singular = false;
    for (int m = 0; m < W; ++m) {
        const float piv = s_d[m * W + m];
        if (pivot_unusable(piv)) singular = true;
        // fixRow (IEEE division); the identity column's entry 1 becomes 1/piv
        for (int c = tid; c < W; c += 256) s_prn[m * W + c] = (c == m ? 1.0f : s_d[m * W + c]) / piv;
        __syncthreads();
        // fixColumn on the other W-1 rows of the block; the pivot column holds the implicit identity column (0)
        constexpr int EPT = (W * W + 255) / 256;
        float vv[EPT];
#pragma unroll
        for (int q = 0; q < EPT; ++q) {
            const int i = tid + q * 256;
            vv[q] = 0.0f;
            if (i < W * W) {
                const int k = i / W, c = i % W;
                const float f = s_d[k * W + m];
                if (k == m) vv[q] = s_prn[m * W + c];
                else vv[q] = __builtin_fmaf(-f, s_prn[m * W + c], (c == m) ? 0.0f : s_d[i]);
                if (c == 0) s_mt[m * W + k] = f;  // own step: the pivot itself
            }
        }
        __syncthreads();  // every thread has read column m of its rows before anyone overwrites it
#pragma unroll
        for (int q = 0; q < EPT; ++q) {
            const int i = tid + q * 256;
            if (i < W * W) s_d[i] = vv[q];
        }
        __syncthreads();
    }
    float *gt = A.gt_out + (size_t)b * A.tstride;
    float *mt = A.mt_out + (size_t)b * A.mtstride;
    float *aux = A.aux_out + (size_t)b * kAuxFloats;
    for (int i = tid; i < W * W; i += 256) {
        gt[(size_t)(i % W) * np + c0 + i / W] = s_d[i];               // gt[col][row]
        mt[(size_t)(i / W) * A.mtld + c0 + i % W] = s_mt[i];           // mt[step][row]
        aux[i] = s_prn[i];
    }
    if (singular && tid == 0 && A.status) atomicMax(&A.status[b], (int)MI32_SINGULAR);
}

// A panel of more than kPanelGroupRows rows: A.ngroups workgroups per matrix (all must be resident at once:
// the host only uses this for small batches), kPanelGroupRows rows each; then the strip tiles of the sub-panel before.
template <int W>
__global__ __launch_bounds__(1024) void gj_panel_multi_kernel(SubpanelArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char sp_smem[];
    static_assert(1024 * 4 == kPanelGroupRows, "1024 threads x 4 rows per lane");
    const int npanel = A.batch * A.ngroups - A.drop_groups;
    if ((int)blockIdx.x < npanel) {
        panel_body<1024, 4, W, false, true>(A, (int)blockIdx.x / A.ngroups, (int)blockIdx.x % A.ngroups, sp_smem);
        return;
    }
    const int grp = threadIdx.x >> 8;
    ostrip_body<W>(A, ((int)blockIdx.x - npanel) * 4 + grp, sp_smem + (size_t)grp * sizeof(OStripShared<W>),
                   threadIdx.x & 255);
}

// update(t) alone: one 64 x 64 tile per 256-thread workgroup; then (the block's last sub-panel) its strip tiles
template <int W>
__global__ __launch_bounds__(256) void gj_inblock_update_kernel(SubpanelArgs A)
{
    constexpr size_t kBytes = sizeof(UpdateTileShared<W>) > sizeof(OStripShared<W>) ? sizeof(UpdateTileShared<W>)
                                                                                    : sizeof(OStripShared<W>);
    __shared__ __attribute__((aligned(16))) unsigned char upd_smem[kBytes];
    if ((int)blockIdx.x < A.upd_wgs) inblock_update_body<W, 1>(A, (int)blockIdx.x, upd_smem);
    else ostrip_body<W>(A, (int)blockIdx.x - A.upd_wgs, upd_smem, threadIdx.x);
}

// tests only: leave the last panel workgroup of every multi-workgroup panel launch out (see dispatch_subpanel)
static std::atomic<int> g_debug_drop_panel_group{0};
extern "C" int mi32_debug_drop_panel_group(int enable)
{
    g_debug_drop_panel_group.store(enable ? 1 : 0, std::memory_order_relaxed);
    return 0;
}

// One launch of the sub-panel pipeline:
//  * panel(s) and update(s-1) together (fused blocks): the workgroup size is the panel's, the update tiles are
//    packed NT / 256 to a workgroup;
//  * panel(s) alone: the smallest thread geometry that holds its rows (fewer waves and fewer rows per lane both
//    shorten a pivot step);
//  * update(t) alone: 256-thread workgroups, one tile each.
static hipError_t dispatch_subpanel(const BlockedRoute &p, int w, const SubpanelArgs &A0, hipStream_t stream)
{
    SubpanelArgs A = A0;
    const int tiles = A.upd_on ? (A.kb / 64) * (p.np / 64) : 0;
    const int os_tiles = A.os_on ? A.batch * A.os_ntiles : 0;  // strip tiles of columns outside the block
    if (!A.panel_on) {
        A.upd_wgs = A.batch * tiles;
        return with_constant<4, 8, 16, 32>(w, [&](auto W) {
            hipLaunchKernelGGL((gj_inblock_update_kernel<W>), dim3(A.upd_wgs + os_tiles), dim3(256), 0, stream, A);
            return hipSuccess;
        });
    }
    if (A.ngroups > 1) {  // multi-workgroup panel: never fused, W = 16 (what the plan gives every block then)
        if (A.upd_on || w != 16) return hipErrorInvalidValue;
        constexpr size_t lds = subpanel_lds_bytes<1024, 4, 16, false>();
        // mi32_debug_drop_panel_group(1) (tests only, host side only): the last panel workgroup of the grid is never
        // launched, i.e. one panel loses a partner -- what a foreign kernel holding the CUs would cause
        A.drop_groups = g_debug_drop_panel_group.load(std::memory_order_relaxed) ? 1 : 0;
        const size_t lds_now = A.os_on ? lds : subpanel_lds_bytes<1024, 4, 16, false>(false);
        hipLaunchKernelGGL((gj_panel_multi_kernel<16>), dim3(A.batch * A.ngroups - A.drop_groups + (os_tiles + 3) / 4),
                           dim3(1024), lds_now, stream, A);
        return hipSuccess;
    }
    int nt, rpt;
    panel_geometry(p, p.np - A.row_lo, nt, rpt);
    A.upd_wgs = A.batch * (tiles / (nt / 256));
    const int nwgs = A.batch + A.upd_wgs + (os_tiles + nt / 256 - 1) / (nt / 256);
    return with_constant<256, 512, 1024>(nt, [&](auto NT) {
        return with_constant<1, 2, 3, 4, 8, 16>(rpt, [&](auto RPT) {
            return with_constant<4, 8, 16, 32>(w, [&](auto W) {
                return with_constant<0, 1>(A.upd_on, [&](auto FUSED) {
                    return launch_subpanel<NT, RPT, W, FUSED != 0>(A, nwgs, stream);
                });
            });
        });
    });
}

static void launch_diag_panel(const SubpanelArgs &P, hipStream_t stream)
{
    const int os_tiles = P.os_on ? P.batch * P.os_ntiles : 0;
    hipLaunchKernelGGL((gj_diag_panel_kernel<16>), dim3(P.batch + os_tiles), dim3(256), 0, stream, P);
}

// the self-test of the DPP row helpers (cases and layout: mi32_dpp.h)
__global__ __launch_bounds__(64) void dpp_selftest_kernel(const unsigned *__restrict__ in, unsigned *__restrict__ out)
{
    const int lane = (int)threadIdx.x;
    const unsigned *q = in + (size_t)blockIdx.x * 3 * 64;
    // (the loads' s_waitcnt stands between them and the first DPP read)
    const float row = __uint_as_float(q[lane]), f = __uint_as_float(q[64 + lane]), acc = __uint_as_float(q[128 + lane]);
    const int pick = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 7u) & 63);
    dpp_selftest_cases(row, f, acc, lane, pick, out + (size_t)blockIdx.x * 16 * 4 * 64,
                       std::make_integer_sequence<int, 16>{});
}

// tests only: runs dpp_selftest_kernel on `ncases` waves.  dev_in: ncases x 3 x 64 words, dev_out: ncases x 16 x 4 x 64.
extern "C" int mi32_debug_dpp_selftest(const unsigned *dev_in, unsigned *dev_out, int ncases, void *stream)
{
    if (dev_in == nullptr || dev_out == nullptr || ncases < 1) return 1;
    hipLaunchKernelGGL(dpp_selftest_kernel, dim3(ncases), dim3(64), 0, (hipStream_t)stream, dev_in, dev_out);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

#ifdef MI32_PANEL_STAMPS
// diagnostic builds only: where the panel kernels write their stamps (device buffer of 1024 x 64 u64, or NULL)
extern "C" int mi32_debug_panel_stamps(unsigned long long *dev_buf)
{
    return hipMemcpyToSymbol(HIP_SYMBOL(g_panel_stamps), &dev_buf, sizeof(dev_buf)) == hipSuccess ? 0 : 3;
}
#endif

}  // namespace mi32
