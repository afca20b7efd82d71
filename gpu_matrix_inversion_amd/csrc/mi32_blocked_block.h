// mi32_blocked_block.h -- the launches of the blocked fp32 path that happen once per block (gfx950 only): the block's
// pivot-row strips in one launch, the multiplier transposition, and the rank-bw update of the columns outside the block
// (mi32_rank_bw.h; the next block's columns alone: gj_rank_update_kernel).
//
// Not a translation unit of its own: mi32_blocked.hip includes it, once.  hipcc's code for the panel kernels depends on
// which other kernels share their translation unit (measured: with the per-block kernels in a unit of their own, 11
// gj_subpanel_kernel instances come out with another schedule and register allocation; with one unit per workgroup
// size, 38 kernels), and changes that only move code are accepted on an unchanged disassembly
// (tools/code_object_diff.py).
#pragma once
#include "mi32_rank_bw.h"
#include "mi32_strip.h"

namespace mi32 {

// ---- the block's pivot-row strips in ONE launch, for the columns strip(t) could not follow -----
// With the look-ahead, the columns outside the block are still being written by the previous block's second-stream
// update while this block's panels run: their strips can only start when that is done.  One workgroup per CT-column
// tile keeps the kb pivot rows x CT columns in the accumulator registers of its 16 waves (one 32 x 32 tile each) and
// runs the block's pivot steps on them, G (= the block's sub-panel width) at a time: the G rows of a group go
// through LDS and strip_step (u_m; G dependent IEEE divisions), then every LATER pivot row takes its G fmaf (one
// v_mfma_f32_32x32x2_f32 chain with the old value as C operand, k ascending).  Out, exactly what the strip(t) tiles
// leave: ub[m][j] = u_m[j], and xs[k][j] = pivot row k after its own sub-panel's last step.
// The groups [g_lo, g_hi) of one call: a block's strips can start before its last panels have run -- the rows of the
// groups still to come are parked in xst in between.  mf[q][m] = -f_m of the row whose index at the start of the
// block was q (own step: -pivot); map = rowsrc.
template <int CT, int G>
constexpr size_t block_strip_lds_bytes(int kb)
{
    return ((size_t)G * (CT + 4) + (size_t)G * (kb + 4) + (size_t)2 * G * (CT + 4)) * sizeof(float) + (size_t)kb * sizeof(int);
}
// kb <= 256 runs CT = 64, wider blocks CT = 32: at most 16 tiles of 32 x 32.  SNT threads: 1024 (16 waves, one tile
// each: a single matrix, where the launch is a chain of rounds on few workgroups) or 512 (8 waves, two tiles each:
// GPU-filling batches -- a round is latency, so two of these per CU, 4 waves per SIMD either way, do twice the tiles).
template <int CT, int G, int SNT>
__global__ __launch_bounds__(SNT, 4) void gj_block_strip_kernel(const float *__restrict__ src_all, size_t mstride, int np, int ld,
                                                              const float *__restrict__ mf_all, size_t mfstride, int mf_ld,
                                                              float *__restrict__ ub_all, float *__restrict__ xs_all,
                                                              float *__restrict__ xst_all, size_t ubstride, int C0, int kb,
                                                              const int *__restrict__ map_all, int col_lo, int col_hi,
                                                              int inside, int g_lo, int g_hi,
                                                              const int *__restrict__ guard)
{
    extern __shared__ __attribute__((aligned(16))) float bs_smem[];
    constexpr int LDX = CT + 4;
    constexpr int NT = SNT;
    constexpr int kStripTPW = 16 / (SNT / 64);  // tiles per wave
    constexpr int CTT = CT / 32;  // tiles per row of tiles
    const int LT = kb + 4;
    float *s_x = bs_smem;                  // [G][LDX]   the rows of the current group
    float *s_lt = s_x + G * LDX;           // [G][LT]    -f of the current G steps, [step][pivot row]
    float *s_u = s_lt + G * LT;            // [2][G][LDX]  u_m of the current G steps (and of the previous G)
    int *s_q = reinterpret_cast<int *>(s_u + 2 * G * LDX);  // [kb] block-start row index of every pivot row

    const int b = blockIdx.y;
    if (matrix_given_up(guard, b)) return;
    const int col0 = blockIdx.x * CT;
    if (col0 >= C0 && col0 < C0 + kb) return;  // the block's own columns are up to date already
    if ((col0 >= col_lo && col0 < col_hi) != (inside != 0)) return;  // the look-ahead splits the columns between two launches
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const float *src = src_all + (size_t)b * mstride;
    const float *mf = mf_all + (size_t)b * mfstride;
    float *ub = ub_all + (size_t)b * ubstride;
    float *xs = xs_all + (size_t)b * ubstride;
    float *xst = xst_all + (size_t)b * ubstride;
    const int *map = map_all + (size_t)b * np;
    const int lcol = lane & 31, lhalf = lane >> 5;
    const int ntiles = (kb / 32) * CTT;

    for (int i = tid; i < kb; i += NT) s_q[i] = map[C0 + i];
    __syncthreads();
    // this wave's tiles of the pivot rows: from the working copy (through the row map) or from where the call for
    // the earlier groups parked them
    float16v acc[kStripTPW];
    // (the source is chosen once, not per value: per value hipcc emits a branch pair and an LDS round trip for the map
    // entry in front of every load; 32-bit byte offsets from the scalar base)
    if (g_lo == 0) {
        const unsigned ld4 = (unsigned)ld * 4u;
        const char *srcb = reinterpret_cast<const char *>(src);
#pragma unroll
        for (int ti = 0; ti < kStripTPW; ++ti) {
            const int t = wave + ti * (NT / 64);
            if (t < ntiles) {
                const int rt = t / CTT;
                const unsigned col4 = (unsigned)(col0 + (t % CTT) * 32 + lcol) * 4u;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int4 m4 = *reinterpret_cast<const int4 *>(&s_q[rt * 32 + 8 * q + 4 * lhalf]);
                    const int mm[4] = {m4.x, m4.y, m4.z, m4.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[ti][4 * q + j] = *reinterpret_cast<const float *>(srcb + ((unsigned)mm[j] * ld4 + col4));
                }
            }
        }
    } else {
#pragma unroll
        for (int ti = 0; ti < kStripTPW; ++ti) {
            const int t = wave + ti * (NT / 64);
            if (t < ntiles) {
                const int rt = t / CTT, col = col0 + (t % CTT) * 32 + lcol;
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int r = rt * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * lhalf;
                    acc[ti][reg] = xst[(size_t)r * np + col];
                }
            }
        }
    }
    // the multipliers of G steps, all kb pivot rows: requested one round ahead (registers), so that a round is the
    // strip and the update, not a dependent global round trip on top
    constexpr int NL = ((CT == 128 ? 128 : CT == 64 ? 256 : kMaxBW) * (G / 4) + NT - 1) / NT;
    float4 lreg[NL];
    auto load_l = [&](int s0) {
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int idx = tid + i * NT;
            if (idx < kb * (G / 4))
                lreg[i] = *reinterpret_cast<const float4 *>(mf + (size_t)s_q[idx / (G / 4)] * mf_ld + s0 + (idx % (G / 4)) * 4);
        }
    };
    auto store_l = [&]() {
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int idx = tid + i * NT;
            if (idx < kb * (G / 4)) {
                const int k = idx / (G / 4), m4 = (idx % (G / 4)) * 4;
                s_lt[(m4 + 0) * LT + k] = lreg[i].x;
                s_lt[(m4 + 1) * LT + k] = lreg[i].y;
                s_lt[(m4 + 2) * LT + k] = lreg[i].z;
                s_lt[(m4 + 3) * LT + k] = lreg[i].w;
            }
        }
    };
    // u_m of G steps -> the rank-bw update's B operand.  Stored one round late, in front of the next request for
    // multipliers: a wave's memory operations complete in order, and the wait for those multipliers at the end of a
    // round must not have to wait for a store issued a moment ago to be acknowledged.
    auto store_u = [&](int s0) {
        const float *su = s_u + ((s0 / G) & 1) * G * LDX;
        for (int idx = tid; idx < G * (CT / 4); idx += NT) {
            const int m = idx / (CT / 4), c4 = (idx % (CT / 4)) * 4;
            *reinterpret_cast<float4 *>(ub + (size_t)(s0 + m) * np + col0 + c4) =
                *reinterpret_cast<const float4 *>(&su[m * LDX + c4]);
        }
    };
    // the rows [O, O + G) of a 32-row tile -> s_x (O a compile-time constant: no run-time index into the registers)
    auto park_group = [&](auto OFF, int rt_o) {
        constexpr int O = decltype(OFF)::value;
#pragma unroll
        for (int ti = 0; ti < kStripTPW; ++ti) {
            const int t = wave + ti * (NT / 64);
            if (t < ntiles && t / CTT == rt_o) {
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int r = (reg & 3) + 8 * (reg >> 2) + 4 * lhalf;
                    if (r >= O && r < O + G) s_x[(r - O) * LDX + (t % CTT) * 32 + lcol] = acc[ti][reg];
                }
            }
        }
    };
    load_l(g_lo * G);
    store_l();
    for (int gi = g_lo; gi < g_hi; ++gi) {
        const int s0 = gi * G;
        float *su = s_u + (gi & 1) * G * LDX;
        if (gi > g_lo) store_u(s0 - G);
        if (gi + 1 < g_hi) load_l(s0 + G);
        {
            const int rt_o = s0 / 32;
            switch ((s0 % 32) / G) {  // 32 / G cases
            case 0: park_group(std::integral_constant<int, 0>{}, rt_o); break;
            case 1: park_group(std::integral_constant<int, (G < 32 ? G : 0)>{}, rt_o); break;
            case 2: park_group(std::integral_constant<int, (2 * G < 32 ? 2 * G : 0)>{}, rt_o); break;
            case 3: park_group(std::integral_constant<int, (3 * G < 32 ? 3 * G : 0)>{}, rt_o); break;
            case 4: park_group(std::integral_constant<int, (4 * G < 32 ? 4 * G : 0)>{}, rt_o); break;
            case 5: park_group(std::integral_constant<int, (5 * G < 32 ? 5 * G : 0)>{}, rt_o); break;
            case 6: park_group(std::integral_constant<int, (6 * G < 32 ? 6 * G : 0)>{}, rt_o); break;
            default: park_group(std::integral_constant<int, (7 * G < 32 ? 7 * G : 0)>{}, rt_o); break;
            }
        }
        __syncthreads();  // the group's rows and s_lt are in LDS
        if (tid < 4 * CT) {
            constexpr int CPT = G / 4;
            const int c = tid >> 2, q4 = tid & 3;
            float x[CPT];
#pragma unroll
            for (int j = 0; j < CPT; ++j) x[j] = s_x[(CPT * q4 + j) * LDX + c];
            strip_steps<G>(x, s_lt + s0, LT, q4, &su[c], LDX, std::make_integer_sequence<int, G>{});
#pragma unroll
            for (int j = 0; j < CPT; ++j) s_x[(CPT * q4 + j) * LDX + c] = x[j];
        }
        __syncthreads();
        // the group's rows after their own sub-panel: where their accumulation starts in the rank-bw update
        for (int idx = tid; idx < G * (CT / 4); idx += NT) {
            const int k = idx / (CT / 4), c4 = (idx % (CT / 4)) * 4;
            *reinterpret_cast<float4 *>(xs + (size_t)(s0 + k) * np + col0 + c4) =
                *reinterpret_cast<const float4 *>(&s_x[k * LDX + c4]);
        }
        // every later pivot row: x[k][c] = fmaf(-f_m[k], u_m[c], x[k][c]), m ascending (rows of this and of earlier
        // groups in a tile take the same instructions: they are never read again)
#pragma unroll
        for (int ti = 0; ti < kStripTPW; ++ti) {
            const int t = wave + ti * (NT / 64);
            if (t < ntiles && (t / CTT) * 32 + 32 > s0 + G) {
                const int rt = t / CTT, ctl = t % CTT;
#pragma unroll
                for (int kk = 0; kk < G; kk += 2) {
                    const float af = s_lt[(kk + lhalf) * LT + rt * 32 + lcol];
                    const float bf = su[(kk + lhalf) * LDX + ctl * 32 + lcol];
                    acc[ti] = __builtin_amdgcn_mfma_f32_32x32x2f32(af, bf, acc[ti], 0, 0, 0);
                }
            }
        }
        __syncthreads();  // before s_lt, s_x are overwritten
        if (gi + 1 < g_hi) store_l();
    }
    store_u((g_hi - 1) * G);
    if (g_hi * G < kb) {  // the rows of the groups still to come: parked for the next call
#pragma unroll
        for (int ti = 0; ti < kStripTPW; ++ti) {
            const int t = wave + ti * (NT / 64);
            if (t < ntiles && (t / CTT) * 32 + 32 > g_hi * G) {
                const int rt = t / CTT, col = col0 + (t % CTT) * 32 + lcol;
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int r = rt * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * lhalf;
                    xst[(size_t)r * np + col] = acc[ti][reg];
                }
            }
        }
    }
}

// Gk[k][row] = mf[map[row]][k], k < kdim: the block's negated multipliers, transposed and in the new row order
// (A operand of the rank-bw update); 64 x 64 tiles through LDS, both global sides coalesced.
// The block's own pivot rows (rows C0 .. C0+kdim-1 of the new order) enter the update with the value the strip of
// their sub-panel left (xs): everything up to the end of that sub-panel is applied already, so their multipliers of
// those steps are replaced by 0 -- fmaf(0, u, x) == x -- and only the later sub-panels' steps reach them.
__global__ __launch_bounds__(256) void gj_mult_transpose_kernel(const float *__restrict__ mf_all, size_t mfstride, int mf_ld,
                                                                 int np, const int *__restrict__ map_all,
                                                                 float *__restrict__ gk_all, size_t gkstride, int C0,
                                                                 int kdim, int w, const int *__restrict__ guard)
{
    __shared__ float t[64][65];
    __shared__ int s_q[64];
    const int b = blockIdx.z;
    if (matrix_given_up(guard, b)) return;
    const int row0 = blockIdx.x * 64, k0 = blockIdx.y * 64;
    const int tid = threadIdx.x;
    const float *mf = mf_all + (size_t)b * mfstride;
    float *gk = gk_all + (size_t)b * gkstride;
    if (tid < 64) s_q[tid] = (map_all + (size_t)b * np)[row0 + tid];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = (tid >> 4) + 16 * q, c4 = (tid & 15) * 4;
        const float4 v = *reinterpret_cast<const float4 *>(mf + (size_t)s_q[r] * mf_ld + k0 + c4);
        const int rel = row0 + r - C0;  // a pivot row of the block: steps below `lim` are applied already
        const int lim = ((unsigned)rel < (unsigned)kdim) ? (rel / w + 1) * w : 0;
        t[r][c4] = (k0 + c4 < lim) ? 0.0f : v.x;
        t[r][c4 + 1] = (k0 + c4 + 1 < lim) ? 0.0f : v.y;
        t[r][c4 + 2] = (k0 + c4 + 2 < lim) ? 0.0f : v.z;
        t[r][c4 + 3] = (k0 + c4 + 3 < lim) ? 0.0f : v.w;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int k = (tid >> 4) + 16 * q, r4 = (tid & 15) * 4;
        *reinterpret_cast<float4 *>(gk + (size_t)(k0 + k) * np + row0 + r4) =
            make_float4(t[r4][k], t[r4 + 1][k], t[r4 + 2][k], t[r4 + 3][k]);
    }
}

// ---- rank-k update of the next block's columns (look-ahead half (A) of a rank-bw update) -----
//   dst[i][j] = src[map[i]][j] - sum_m f_m[i] * u_m[j]    for the rows i outside the block
// for the 64-column tiles starting at col_lo.  Same arithmetic as the rank-bw kernel of mi32_rank_bw.h (one fmaf
// chain per element from the old value, m ascending), on 64 x 64 tiles because the few columns of one block would
// otherwise make too few workgroups; -f is read from the block's multiplier matrix through the row map, u_m from ub.
template <int BK>
__global__ __launch_bounds__(256) void gj_rank_update_kernel(const float *__restrict__ src_all,
                                                              float *__restrict__ dst_all,
                                                              const float *__restrict__ mf_all, size_t mfstride, int mf_ld,
                                                              const float *__restrict__ ub_all,
                                                              const float *__restrict__ xs_all, size_t ubstride,
                                                              int np, int ld, size_t mstride, int c0, int kdim, int w,
                                                              int col_lo, const int *__restrict__ map_all,
                                                              PanelExport ex, size_t tstride,
                                                              const int *__restrict__ guard)
{
    constexpr int BM = 64, BN = 64;
    constexpr int PADA = (32 / BK) > 0 ? (32 / BK) : 1;
    constexpr int LDA = BM + PADA;
    constexpr int LDB = BN + 4;
    __shared__ float s_a[BK * LDA];
    __shared__ __attribute__((aligned(16))) float s_b[BK * LDB];
    __shared__ int s_map[BM];

    const int b = blockIdx.z;
    if (matrix_given_up(guard, b)) return;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int row0 = blockIdx.y * BM;
    // the block's own pivot rows start from what the strip of their sub-panel left (xs) and only take the later
    // sub-panels' steps (see gj_mult_transpose_kernel)
    const bool tile_in_block = (row0 >= c0 && row0 < c0 + kdim);
    const int col0 = col_lo + blockIdx.x * BN;
    const float *src = src_all + (size_t)b * mstride;
    float *dst = dst_all + (size_t)b * mstride;
    const float *mf = mf_all + (size_t)b * mfstride;
    const float *ub = ub_all + (size_t)b * ubstride;
    const float *xs = xs_all + (size_t)b * ubstride;
    const int *map = map_all + (size_t)b * np;

    for (int i = tid; i < BM; i += 256) s_map[i] = map[row0 + i];
    __syncthreads();

    float16v acc;
    const int lcol = lane & 31;
    const int lhalf = lane >> 5;
    {
        const int col = col0 + wc * 32 + lcol;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int lr = wr * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * lhalf;
            acc[reg] = tile_in_block ? xs[(size_t)(row0 + lr - c0) * np + col] : src[(size_t)s_map[lr] * ld + col];
        }
    }
    for (int kt = 0; kt < kdim; kt += BK) {
        // stage A: BM x BK of the row-major multiplier matrix (rows through the map), transposed
#pragma unroll
        for (int q = 0; q < (BM * BK / 4 + 255) / 256; ++q) {
            const int idx = tid + q * 256;
            if (idx < BM * BK / 4) {
                const int rr = idx / (BK / 4), k4 = (idx % (BK / 4)) * 4;
                const float4 v = *reinterpret_cast<const float4 *>(mf + (size_t)s_map[rr] * mf_ld + kt + k4);
                const int lim = tile_in_block ? ((row0 + rr - c0) / w + 1) * w : 0;
                s_a[(k4 + 0) * LDA + rr] = (kt + k4 + 0 < lim) ? 0.0f : v.x;
                s_a[(k4 + 1) * LDA + rr] = (kt + k4 + 1 < lim) ? 0.0f : v.y;
                s_a[(k4 + 2) * LDA + rr] = (kt + k4 + 2 < lim) ? 0.0f : v.z;
                s_a[(k4 + 3) * LDA + rr] = (kt + k4 + 3 < lim) ? 0.0f : v.w;
            }
        }
        // stage B: BK rows of u x BN columns
#pragma unroll
        for (int q = 0; q < (BK * BN / 4 + 255) / 256; ++q) {
            const int idx = tid + q * 256;
            if (idx < BK * BN / 4) {
                const int kk = idx / (BN / 4), c4 = (idx % (BN / 4)) * 4;
                *reinterpret_cast<float4 *>(&s_b[kk * LDB + c4]) =
                    *reinterpret_cast<const float4 *>(ub + (size_t)(kt + kk) * np + col0 + c4);
            }
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {
            const float af = s_a[(kk + lhalf) * LDA + wr * 32 + lcol];
            const float bf = s_b[(kk + lhalf) * LDB + wc * 32 + lcol];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af, bf, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    {
        const int col = col0 + wc * 32 + lcol;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int grow = row0 + wr * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * lhalf;
            dst[(size_t)grow * ld + col] = acc[reg];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            panel_export_store4(ex, tstride, b, np, col, row0 + wr * 32 + 8 * q + 4 * lhalf, acc[4 * q], acc[4 * q + 1],
                                acc[4 * q + 2], acc[4 * q + 3]);
    }
}

template <int CT, int G, int SNT>
static hipError_t launch_block_strip_t(const BlockStripArgs &a, int batch, hipStream_t st)
{
    const hipError_t e = raise_lds_limit((const void *)gj_block_strip_kernel<CT, G, SNT>,
                                         block_strip_lds_bytes<CT, G>(CT == 128 ? 128 : CT == 64 ? 256 : kMaxBW));
    if (e != hipSuccess) return e;
    const size_t lds = block_strip_lds_bytes<CT, G>(a.kb);
    hipLaunchKernelGGL((gj_block_strip_kernel<CT, G, SNT>), dim3(a.np / CT, batch), dim3(SNT), lds, st, a.src, a.mstride,
                       a.np, a.ld, a.mf, a.mfstride, a.mf_ld, a.ub, a.xs, a.xst, a.ubstride, a.C0, a.kb, a.map, a.col_lo,
                       a.col_hi, a.inside, a.g_lo, a.g_hi, a.guard);
    return hipSuccess;
}
static hipError_t launch_block_strip(int w, int batch, hipStream_t st, const BlockStripArgs &a)
{
    return with_constant<4, 8, 16, 32>(w, [&](auto G) {
        if (batch * (a.np / 64) > 512) {  // GPU-filling: small workgroups
            if (a.kb <= 128 && a.C0 % 128 == 0 && a.np % 128 == 0)  // 128 columns: the strip uses all 512 threads
                return launch_block_strip_t<128, G, 512>(a, batch, st);
            return a.kb <= 256 ? launch_block_strip_t<64, G, 512>(a, batch, st) : launch_block_strip_t<32, G, 512>(a, batch, st);
        }
        return a.kb <= 256 ? launch_block_strip_t<64, G, 1024>(a, batch, st) : launch_block_strip_t<32, G, 1024>(a, batch, st);
    });
}

static void launch_mult_transpose(const RankUpdateArgs &a, int batch, hipStream_t st)
{
    hipLaunchKernelGGL(gj_mult_transpose_kernel, dim3(a.np / 64, a.kb / 64, batch), dim3(256), 0, st, a.mf, a.mfstride,
                       a.mf_ld, a.np, a.map, a.gk, a.gkstride, a.C0, a.kb, a.w, a.guard);
}

// all columns outside the block; `ex`: the next block's first sub-panels
static void launch_rank_bw(const RankUpdateArgs &a, const PanelExport &ex, int batch, hipStream_t st)
{
    hipLaunchKernelGGL((gj_rank_bw2_kernel<kBwBK, kBwWPS>), dim3((a.np / 128) * (a.np / 128), batch), dim3(256),
                       rank_bw2_lds_bytes<kBwBK>(a.kb), st, a.src, a.dst, a.panel, a.mstride, a.gk, a.gkstride, a.ub, a.xs,
                       a.np, a.ld, a.mstride, a.C0, a.kb, a.map, a.copy_panel, ex, a.tstride, 0, 0, a.guard);
}

// ... but those in [skip_lo, skip_hi), by `workgroups` persistent workgroups with lds_bytes of dynamic LDS each
static void launch_rank_bw_persistent(const RankUpdateArgs &a, const PanelExport &ex, int skip_lo, int skip_hi,
                                      int workgroups, size_t lds_bytes, int batch, hipStream_t st)
{
    hipLaunchKernelGGL((gj_rank_bw2_persistent_kernel<kBwBK>), dim3(workgroups, batch), dim3(256), lds_bytes, st, a.src,
                       a.dst, a.panel, a.mstride, a.gk, a.gkstride, a.ub, a.xs, a.np, a.ld, a.mstride, a.C0, a.kb, a.map,
                       a.copy_panel, ex, a.tstride, skip_lo, skip_hi, a.guard);
}

// the ncols columns from col_lo on (the next block's)
static void launch_rank_update_cols(const RankUpdateArgs &a, const PanelExport &ex, int col_lo, int ncols, int batch,
                                    hipStream_t st)
{
    // small tiles: only ncols columns, so 64x64 gives 4x the workgroups of 128x128
    hipLaunchKernelGGL((gj_rank_update_kernel<32>), dim3(ncols / 64, a.np / 64, batch), dim3(256), 0, st, a.src, a.dst,
                       a.mf, a.mfstride, a.mf_ld, a.ub, a.xs, a.gkstride, a.np, a.ld, a.mstride, a.C0, a.kb, a.w, col_lo,
                       a.map, ex, a.tstride, a.guard);
}

}  // namespace mi32
