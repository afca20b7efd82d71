// mi32_nopivot64.hip -- blocked Gauss-Jordan in double WITHOUT pivoting: the reference's matrix_inversion_no_pivots
// (matrix_inversion_no_pivots.cpp:10, headers.h:11) in the reference's own order, element by element, with its O(N^3)
// part on the fp64 matrix cores (gfx950: v_mfma_f64_16x16x4_f64).
//
// Step r of the in-place form (oracle/gj_oracle.c: inv64_inplace_impl with pivoting off, gjo_matrix_inv_64_nopivot):
//   piv = X[r][r];  X[r][j] /= piv for every j, then X[r][r] = 1 / piv;
//   every other row i: f = X[i][r], X[i][r] = 0, X[i][j] = fma(-f, X[r][j], X[i][j]) for every j.
// For a block K = [c0, c0 + bw) of steps, r = c0 + m: U[m][j] = row r right after its division, f_m[i] = X[i][r] when
// step r runs.  Per block, four launches; every element goes through exactly the chain above:
//   (a) np64_diag_kernel: one workgroup per matrix runs the bw steps on X[K][K] (register-resident); it yields piv_m,
//       U[m][K], the in-block multipliers -f_m[c0 + i] and the final X[K][K], and flags a bad pivot;
//   (b) np64_block_kernel, row part: every row i outside K goes through the bw steps on its block columns and stores
//       -f_m[i] k-major (the A operand of (d));
//   (c) np64_block_kernel, column part: every column j outside K -- the pivot rows' entries y = X[r][j] go through the
//       steps k < m, U[m][j] = y / piv_m (IEEE division), then through the steps k > m; U is the B operand of (d);
//   (d) np64_rank_update_kernel: X[i][j] = fma(-f_m[i], U[m][j], X[i][j]) for m ascending, i and j outside K: one
//       k-ascending chain of v_mfma_f64_16x16x4_f64 per element whose C operand is the old value.
// One departure from the reference: a zero multiplier is multiplied through rather than skipped
// (matrix_inversion_no_pivots.cpp:29).  With every intermediate finite only the sign of a zero entry can differ; once a
// pivot row holds an infinity (an inverse that overflows: status 0, the pivots are finite) fma(-0, +-inf, x) is a NaN
// where the reference keeps x.  The result is then, entry by entry, that of the oracle's steps with the zero multiplier
// multiplied through (oracle/gj_oracle.c, GJO_ZEROS_THROUGH): tests/test_gpu_overflow.py, test_no_pivot_blocked.
//
// Working matrix: diag(I, A), the N x N in-place form BEHIND an identity block that pads it to a multiple of bw, so
// that no kernel needs a bounds check.  The padded steps come first: each divides an identity row by 1 and multiplies
// exact zeros through finite rows, which changes no bit.  By the time a real pivot row holds an infinity the padded
// rows are retired -- they take the NaN of 0 * inf, and so do the padded columns, but nothing reads either again.
// (With the padding behind the matrix its steps ran last, on rows that held those NaNs, and carried them into every
// real row of the column.)  No row is ever swapped: the result is copied out of the corner through the identity map.
#include "mi32_internal.h"
#include "mi32_sweep_common.h"

namespace mi32 {

typedef double np64_d4v __attribute__((ext_vector_type(4)));

NoPivot64Plan make_nopivot64_plan(int n, int bw)
{
    NoPivot64Plan p;
    p.n = n;
    // block width 64 (default) or 128; larger requests are capped (the diagonal block of (a) lives in registers, and
    // the block columns of one row take 2 doubles per lane at 128).  Measured ms per inversion, bw 64 / 128:
    // N = 1024 1.15 / 1.71, 2048 2.73 / 3.67, 4096 7.98 / 9.52 (the diagonal blocks: 2.3 / 5.2 ms of it)
    bw = (bw >= 128) ? 128 : 64;
    if (bw > ((n + 63) & ~63)) bw = 64;
    p.bw = bw;
    p.np = ((n + bw - 1) / bw) * bw;
    p.ld = p.np;
    return p;
}

struct NP64Ws {
    double *w, *ft, *ub, *piv;
    int *orig, *invp;
    size_t wstride, fstride;
};
static size_t np64_carve(const NoPivot64Plan &p, int batch, void *base, NP64Ws &o, WsRegions *regions = nullptr)
{
    const size_t wbytes = align256((size_t)p.np * p.ld * sizeof(double));
    const size_t fbytes = align256((size_t)p.bw * p.np * sizeof(double));
    const size_t ibytes = align256((size_t)p.np * sizeof(int) * batch);
    WsCarver c(base, regions);
    o.wstride = wbytes / sizeof(double);
    o.fstride = fbytes / sizeof(double);
    o.w = c.take<double>(wbytes * batch, WS_VALUES, "w");
    o.ft = c.take<double>(fbytes * batch, WS_VALUES, "ft");   // -f_m[i], [m][i] (k-major): A operand of the rank-bw update
    o.ub = c.take<double>(fbytes * batch, WS_VALUES, "ub");   // U[m][j], [m][j]: B operand
    o.piv = c.take<double>(align256((size_t)p.bw * sizeof(double) * batch), WS_VALUES, "piv");
    o.orig = c.take<int>(ibytes, WS_INDICES, "orig");
    o.invp = c.take<int>(ibytes, WS_INDICES, "invp");
    return c.off;
}
size_t nopivot64_workspace_bytes(const NoPivot64Plan &p, int batch, WsRegions *regions)
{
    NP64Ws ws;
    return np64_carve(p, batch, nullptr, ws, regions);
}

__device__ __forceinline__ double np64_readlane(double v, int lane)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), lane);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// ---- (a) the bw steps on the diagonal block X[K][K] --------------------------------------------------------------
// 8 BW threads; thread (g, c) holds column c of the rows [g * RPT, (g + 1) * RPT) of the block in registers (RPT = BW / 8).  Before
// step m, the owners of row m publish its raw entries (s_row) and the owners of column m publish the multipliers
// (s_col) and zero their copies (X[i][r] = 0 of the reference, the fma below then adds -f / piv); one barrier per
// step, the two publish buffers alternate.
template <int BW>
__global__ __launch_bounds__(8 * BW) void np64_diag_kernel(double *__restrict__ w_all, int ld, size_t wstride, int c0,
                                                         double *__restrict__ ft_all, double *__restrict__ ub_all, int np,
                                                         size_t fstride, double *__restrict__ piv_all,
                                                         int *__restrict__ status)
{
    constexpr int G = 8, RPT = BW / G;
    static_assert(RPT % 2 == 0, "the publish buffers alternate with the parity of the step");
    __shared__ double s_row[2][BW];
    __shared__ double s_col[2][BW];
    const int b = blockIdx.x;
    const int t = threadIdx.x;
    const int c = t % BW, g = __builtin_amdgcn_readfirstlane(t / BW);  // g is wave-uniform
    double *w = w_all + (size_t)b * wstride + (size_t)c0 * ld + c0;
    // row m of U and of the multipliers (uniform, advanced by np per step; the lanes add their column)
    double *ftm = ft_all + (size_t)b * fstride + c0 + g * RPT;
    double *ubm = ub_all + (size_t)b * fstride + c0;
    double *pv = piv_all + (size_t)b * BW;

    double x[RPT];
#pragma unroll
    for (int q = 0; q < RPT; ++q) x[q] = w[(size_t)(g * RPT + q) * ld + c];
    if (g == 0) s_row[0][c] = x[0];
    if (c == 0) {
#pragma unroll
        for (int q = 0; q < RPT; ++q) { s_col[0][g * RPT + q] = x[q]; x[q] = 0.0; }
    }
    __syncthreads();
    bool bad = false;
    for (int gm = 0; gm < G; ++gm) {
#pragma unroll
        for (int s = 0; s < RPT; ++s) {
            const int m = gm * RPT + s;
            const int buf = s & 1;  // == m & 1 (RPT is even)
            const double piv = s_row[buf][m];
            // fixRow: X[r][j] / piv (IEEE division), the identity entry 1 / piv
            const double u = (c == m ? 1.0 : s_row[buf][c]) / piv;
            const bool mine = (g == gm);
#pragma unroll
            for (int q = 0; q < RPT; ++q) x[q] = __builtin_fma(-s_col[buf][g * RPT + q], u, x[q]);
            if (mine) {
                x[s] = u;
                ubm[c] = u;
            }
            if (c < RPT) ftm[c] = -s_col[buf][g * RPT + c];  // (-piv at row m: never read)
            ubm += np;
            ftm += np;
            if (t == 0) {
                pv[m] = piv;
                bad = bad || pivot_unusable(piv);
            }
            if (m + 1 < BW) {
                const int s1 = (s + 1) % RPT, g1 = (s + 1 == RPT) ? gm + 1 : gm;
                if (g == g1) s_row[buf ^ 1][c] = x[s1];
                if (c == m + 1) {
#pragma unroll
                    for (int q = 0; q < RPT; ++q) { s_col[buf ^ 1][g * RPT + q] = x[q]; x[q] = 0.0; }
                }
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int q = 0; q < RPT; ++q) w[(size_t)(g * RPT + q) * ld + c] = x[q];
    if (bad && status) status[b] = MI32_SINGULAR;  // status[b] was zeroed by the host; same value from every writer
}

// ---- (b) + (c): the block columns of every other row, the pivot rows' strip of every other column -----------------
// One wave per NPR rows (b) or NPR consecutive columns (c); lane l holds the entries l + 64 s (s < BW / 64) of the
// block: columns c0 + l + 64 s of its rows, or rows c0 + l + 64 s of its columns.  Workgroups [0, np / (4 NPR)) take
// rows, the rest columns; a workgroup whose rows / columns lie in K has nothing to do.
static constexpr int kNp64Npr = 4;

template <int BW>
__device__ __forceinline__ void np64_rows(double *__restrict__ w, double *__restrict__ ft, const double *__restrict__ ub,
                                          int np, int ld, int c0, int i0, int lane)
{
    constexpr int S = BW / 64, R = kNp64Npr;
    double x[R][S], nf[R][S];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int s = 0; s < S; ++s) {
            x[r][s] = w[(size_t)(i0 + r) * ld + c0 + lane + 64 * s];
            nf[r][s] = 0.0;
        }
#pragma unroll
    for (int sm = 0; sm < S; ++sm) {
#pragma unroll 4
        for (int lm = 0; lm < 64; ++lm) {
            const int m = sm * 64 + lm;
            double u[S];
#pragma unroll
            for (int s = 0; s < S; ++s) u[s] = ub[(size_t)m * np + c0 + lane + 64 * s];
            const bool own = lane == lm;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double f = np64_readlane(x[r][sm], lm);  // f_m[i] = X[i][c0 + m] when step c0 + m runs
                nf[r][sm] = own ? -f : nf[r][sm];
                x[r][sm] = own ? 0.0 : x[r][sm];
#pragma unroll
                for (int s = 0; s < S; ++s) x[r][s] = __builtin_fma(-f, u[s], x[r][s]);
            }
        }
    }
#pragma unroll
    for (int s = 0; s < S; ++s) {
#pragma unroll
        for (int r = 0; r < R; ++r) w[(size_t)(i0 + r) * ld + c0 + lane + 64 * s] = x[r][s];
        *reinterpret_cast<Vec4<double> *>(ft + (size_t)(lane + 64 * s) * np + i0) =
            Vec4<double>{nf[0][s], nf[1][s], nf[2][s], nf[3][s]};
    }
}

template <int BW>
__device__ __forceinline__ void np64_cols(double *__restrict__ w, const double *__restrict__ ft, double *__restrict__ ub,
                                          const double *__restrict__ pv, int np, int ld, int c0, int j0, int lane)
{
    constexpr int S = BW / 64, R = kNp64Npr;
    double x[R][S], us[R][S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const Vec4<double> v = *reinterpret_cast<const Vec4<double> *>(w + (size_t)(c0 + lane + 64 * s) * ld + j0);
        x[0][s] = v.x; x[1][s] = v.y; x[2][s] = v.z; x[3][s] = v.w;
#pragma unroll
        for (int r = 0; r < R; ++r) us[r][s] = 0.0;
    }
#pragma unroll
    for (int sk = 0; sk < S; ++sk) {
#pragma unroll 2
        for (int lk = 0; lk < 64; ++lk) {
            const int k = sk * 64 + lk;
            const double piv = pv[k];
            double nf[S];  // -f_k[c0 + m] of this lane's rows m
#pragma unroll
            for (int s = 0; s < S; ++s) nf[s] = ft[(size_t)k * np + c0 + lane + 64 * s];
            const bool own = lane == lk;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double u = np64_readlane(x[r][sk], lk) / piv;  // U[k][j] (IEEE division)
#pragma unroll
                for (int s = 0; s < S; ++s) x[r][s] = __builtin_fma(nf[s], u, x[r][s]);
                x[r][sk] = own ? u : x[r][sk];
                us[r][sk] = own ? u : us[r][sk];
            }
        }
    }
#pragma unroll
    for (int s = 0; s < S; ++s) {
        *reinterpret_cast<Vec4<double> *>(w + (size_t)(c0 + lane + 64 * s) * ld + j0) =
            Vec4<double>{x[0][s], x[1][s], x[2][s], x[3][s]};
        *reinterpret_cast<Vec4<double> *>(ub + (size_t)(lane + 64 * s) * np + j0) =
            Vec4<double>{us[0][s], us[1][s], us[2][s], us[3][s]};
    }
}

template <int BW>
__global__ __launch_bounds__(256) void np64_block_kernel(double *__restrict__ w_all, double *__restrict__ ft_all,
                                                          double *__restrict__ ub_all, const double *__restrict__ piv_all,
                                                          int np, int ld, size_t wstride, size_t fstride, int c0)
{
    constexpr int PER_WG = 4 * kNp64Npr;  // rows / columns per workgroup (divides BW)
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int half = np / PER_WG;
    const bool rows = (int)blockIdx.x < half;
    const int base = (rows ? (int)blockIdx.x : (int)blockIdx.x - half) * PER_WG;
    if (base >= c0 && base < c0 + BW) return;
    double *w = w_all + (size_t)b * wstride;
    double *ft = ft_all + (size_t)b * fstride;
    double *ub = ub_all + (size_t)b * fstride;
    if (rows)
        np64_rows<BW>(w, ft, ub, np, ld, c0, base + wave * kNp64Npr, lane);
    else
        np64_cols<BW>(w, ft, ub, piv_all + (size_t)b * BW, np, ld, c0, base + wave * kNp64Npr, lane);
}

// ---- (d) the rank-bw update on the fp64 matrix cores, in place -------------------------------------------------
//   X[i][j] = fma(-f_m[i], U[m][j], X[i][j]) for m = 0 .. kdim-1, every 64 x 64 tile with rows and columns outside K.
// Tile and operand maps of b64_rank_update_kernel (mi32_blocked64.hip): 256 threads = 4 waves (2 x 2), each 32 x 32 =
// 2 x 2 tiles of v_mfma_f64_16x16x4_f64; A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15],
// C/D[row = (lane >> 4) + 4 * reg][col = lane & 15].  Both operands are k-major in global memory.
__global__ __launch_bounds__(256) void np64_rank_update_kernel(double *__restrict__ w_all, const double *__restrict__ ft_all,
                                                                const double *__restrict__ ub_all, int np, int ld,
                                                                size_t wstride, size_t fstride, int c0, int kdim)
{
    constexpr int BK = 16, LDT = 64 + 2;
    __shared__ double s_a[BK * LDT];  // -f of the tile's rows, [k][row]
    __shared__ double s_b[BK * LDT];  // U of the tile's columns, [k][col]
    const int b = blockIdx.z;
    const int row0 = blockIdx.y * 64, col0 = blockIdx.x * 64;
    if ((row0 >= c0 && row0 < c0 + kdim) || (col0 >= c0 && col0 < c0 + kdim)) return;  // (a), (b), (c) own those
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    double *w = w_all + (size_t)b * wstride;
    const double *ft = ft_all + (size_t)b * fstride;
    const double *ub = ub_all + (size_t)b * fstride;

    const int l15 = lane & 15, l4 = lane >> 4;
    np64_d4v acc[2][2];
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int grow = row0 + wr * 32 + tm * 16 + l4 + 4 * reg;
                const int col = col0 + wc * 32 + tn * 16 + l15;
                acc[tm][tn][reg] = w[(size_t)grow * ld + col];
            }
    const int kk_ld = tid >> 4, c4 = (tid & 15) * 4;  // staging: 16 k x 64 rows / columns, 4 per thread
    for (int kt = 0; kt < kdim; kt += BK) {
        {
            const Vec4<double> va = *reinterpret_cast<const Vec4<double> *>(ft + (size_t)(kt + kk_ld) * np + row0 + c4);
            const Vec4<double> vb = *reinterpret_cast<const Vec4<double> *>(ub + (size_t)(kt + kk_ld) * np + col0 + c4);
            double *pa = s_a + kk_ld * LDT + c4;
            double *pb = s_b + kk_ld * LDT + c4;
            pa[0] = va.x; pa[1] = va.y; pa[2] = va.z; pa[3] = va.w;
            pb[0] = vb.x; pb[1] = vb.y; pb[2] = vb.z; pb[3] = vb.w;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < BK; kk += 4) {
            double af[2], bf[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                af[q] = s_a[(kk + l4) * LDT + wr * 32 + q * 16 + l15];
                bf[q] = s_b[(kk + l4) * LDT + wc * 32 + q * 16 + l15];
            }
#pragma unroll
            for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                for (int tn = 0; tn < 2; ++tn)
                    acc[tm][tn] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[tm], bf[tn], acc[tm][tn], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int grow = row0 + wr * 32 + tm * 16 + l4 + 4 * reg;
                const int col = col0 + wc * 32 + tn * 16 + l15;
                w[(size_t)grow * ld + col] = acc[tm][tn][reg];
            }
}

template <int BW>
static hipError_t np64_run_blocks(const NoPivot64Plan &p, const NP64Ws &ws, int batch, int *d_status, hipStream_t stream,
                                  Profiler *prof, const DetRec &det)
{
    const int np = p.np;
    for (int c0 = 0; c0 < np; c0 += BW) {
        {
            ProfScope ps(prof, KC_PANEL, stream);
            hipLaunchKernelGGL((np64_diag_kernel<BW>), dim3(batch), dim3(8 * BW), 0, stream, ws.w, p.ld, ws.wstride, c0,
                               ws.ft, ws.ub, np, ws.fstride, ws.piv, d_status);
        }
        if (det.on()) {  // a det call: the block's pivots (ws.piv, BW per matrix) into the per-matrix list, before the
                         // next block's diagonal kernel overwrites them
            ProfScope ps(prof, KC_FINISH, stream);
            const hipError_t e = hipMemcpy2DAsync((double *)det.piv + c0, det.pstride * sizeof(double), ws.piv,
                                                  (size_t)BW * sizeof(double), (size_t)BW * sizeof(double), batch,
                                                  hipMemcpyDeviceToDevice, stream);
            if (e != hipSuccess) return e;
        }
        if (np == BW) break;  // one block: nothing outside it
        {
            ProfScope ps(prof, KC_UPDATE_IN, stream);
            hipLaunchKernelGGL((np64_block_kernel<BW>), dim3(2 * np / (4 * kNp64Npr), batch), dim3(256), 0, stream, ws.w,
                               ws.ft, ws.ub, ws.piv, np, p.ld, ws.wstride, ws.fstride, c0);
        }
        {
            ProfScope ps(prof, KC_UPDATE_OUT, stream);
            hipLaunchKernelGGL(np64_rank_update_kernel, dim3(np / 64, np / 64, batch), dim3(256), 0, stream, ws.w, ws.ft,
                               ws.ub, np, p.ld, ws.wstride, ws.fstride, c0, BW);
        }
    }
    return hipSuccess;
}

hipError_t nopivot64_invert(const NoPivot64Plan &p, const double *d_a, double *d_inv, int batch, int *d_status, void *wsp,
                            hipStream_t stream, Profiler *prof, const DetRec &det)
{
    NP64Ws ws;
    np64_carve(p, batch, wsp, ws);
    hipError_t e;
    if (d_status) {
        if ((e = hipMemsetAsync(d_status, 0, sizeof(int) * (size_t)batch, stream)) != hipSuccess) return e;
    }
    {
        ProfScope ps(prof, KC_INIT, stream);  // diag(I, A) into the working copy, non-finite input -> MI32_SINGULAR
        launch_b64_init(d_a, p.n, p.np, p.ld, ws.wstride, ws.w, ws.orig, batch, d_status, stream, p.np - p.n);
    }
    e = p.bw == 128 ? np64_run_blocks<128>(p, ws, batch, d_status, stream, prof, det)
                    : np64_run_blocks<64>(p, ws, batch, d_status, stream, prof, det);
    if (e != hipSuccess) return e;
    if (!d_inv) return hipGetLastError();  // determinant only (det calls): nothing to copy out
    ProfScope ps(prof, KC_FINISH, stream);  // orig is the identity: a plain copy-out of the N x N corner behind the padding
    const int pad = p.np - p.n;
    launch_unpermute(ws.w + (size_t)pad * p.ld + pad, p.ld, ws.wstride, ws.orig, ws.invp, p.np, p.n, batch, d_inv, stream);
    return hipGetLastError();
}

}  // namespace mi32
