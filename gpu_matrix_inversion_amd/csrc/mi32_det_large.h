// mi32_det_large.h -- the determinant beside the inverse above order kWorkgroupMaxOrder (mi32_inv_det_any_device*), on
// the sweep and blocked paths.  The pivots of those paths are spread over launches: every route records them, in step
// order, into a per-matrix list the context owns for det calls, and one finish kernel runs the recurrence of
// mi32_internal.h (det_accumulate) over the list.  A plain call runs the kernels it always ran: the step kernels that
// hold a pivot in a register only (sweep, fp64 blocked with pivoting) have a det twin, a second __global__ entry point
// of the same body (sweep_step in mi32_sweep.hip, b64_step in mi32_blocked64.hip: one template with a bool DET, the
// det lines under `if constexpr (DET)`).
//
// Two facts about the sign.  (1) IEEE multiplication and frexp are sign-symmetric, so the per-step flips `if (swap) m =
// -m` may all be applied at the end as one parity: the pair is bit-identical.  (2) Every exchanging step is one
// transposition, so the parity of the number of exchanging steps is the parity of the final row map.
#pragma once
#include "mi32_internal.h"

namespace mi32 {

// (DetRec, what a det call hands to a route: mi32_internal.h)

// flag[b] <- 1 when an entry of member b's input is not finite (flag was zeroed on the stream before)
template <typename T>
void launch_det_scan(const T *d_a, int n, int batch, int *flag, hipStream_t stream);

// blocked fp32: the pivots of the outer block [C0, C0 + kb), piv[b][C0 + m] = -mf[rowsrc[b][C0 + m]][m] (mf: the
// block's negated multipliers by block-start row index, own step: -pivot; rowsrc: position after the block -> row
// index at its start).  A matrix whose guard word is MI32_RUNTIME_ERROR is skipped (guard may be null).
void launch_det_gather(const float *mf, size_t mfstride, int mf_ld, const int *rowsrc, int np, int C0, int kb, float *piv,
                       size_t pstride, int batch, const int *guard, hipStream_t stream);

// parity[b] <- (np - number of cycles of orig[b]) mod 2: the parity of the row map, one workgroup per matrix, the map
// in LDS (np <= 16384)
void launch_det_parity(const int *orig, int np, int batch, int *parity, const int *guard, hipStream_t stream);

// The recurrence over the steps first ... first + n - 1 of every list, one wave per matrix; then the parity, the input
// flag and the status word; the pair to det.mant[b], det.exp[b].
template <typename T>
void launch_det_finish(const T *piv, size_t pstride, int first, int n, const int *parity, const int *flag,
                       const int *status, bool pivoting, DetOut det, int batch, hipStream_t stream);

// The context's det memory for `batch` lists of `np` elements: [flag][parity][piv], carved like a workspace (WsCarver).
struct DetMem {
    int *flag, *parity;
    void *piv;
    size_t pstride;
    size_t wbytes;  // bytes of flag and of parity, each
    size_t bytes;   // of the whole carve
};
DetMem det_carve(void *base, int np, int batch, size_t elem_bytes, WsRegions *regions = nullptr);
// the size-only pass of det_carve
size_t det_bytes(int np, int batch, size_t elem_bytes, WsRegions *regions = nullptr);

}  // namespace mi32
