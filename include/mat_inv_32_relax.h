/* mat_inv_32_relax.h -- a solver-level use of the stored block inverses: the residual of the block rows of a CSR
 * matrix, and one fused block-Jacobi relaxation sweep  x' = x + omega blockdiag(A)^-1 (b - A x)  from the CSR matrix and
 * the store of mat_inv_32_stored.h.  A header of its own beside mat_inv_32_c.h, mat_inv_32_csr.h and
 * mat_inv_32_stored.h, which it includes for the handle, the plan, the status codes and the storage formats; same
 * library, same conventions.
 *
 * INPUTS (T is float or double).  The matrix is square, N x N, in CSR on the device as in mi32_csr_blocks_device:
 * d_row_ptr[N + 1] and d_col[nnz] of ONE index type, int32_t (index_bytes 4) or int64_t (index_bytes 8), d_val[nnz] in
 * T.  The plan holds members of orders 1 ... 128; d_first (device int64[batch]) puts member b at rows and columns
 * d_first[b] ... d_first[b] + n_b - 1, which must lie inside the matrix.  d_x and d_b are N-vectors in T.
 *
 * THE RESIDUAL OF ROW g is fixed bit for bit.  Let the stored entries of row g be e = 0 ... c-1 IN STORED ORDER
 * (columns need no order, c may be 0).  Eight partial sums p_0 ... p_7 start at +0; for e ascending
 *     p_{e mod 8} = fma(val_e, x[col_e], p_{e mod 8}),
 * one fused multiply-add in T per entry, no term skipped.  Three butterfly levels follow, whose additions are
 * commutative, so that every position holds the same bits:
 *     q_s = p_s + p_{s xor 4},   t_s = q_s + q_{s xor 2},   sum = t_0 + t_1,
 * and  r_g = b_g - sum,  one rounding.  Eight is the width of the smallest lane class, so one rule holds for every
 * block order: the bits depend on the row's entries and on x alone, not on the block's order, its neighbours in the
 * wave, the grid or the index type.  A column outside [0, N) is the caller's error, as is a d_row_ptr that is not that
 * of a CSR matrix.
 *
 * THE SWEEP.  With r_b the residuals of member b's rows, z_b is exactly what mi32_apply_stored_device returns for
 * member b on r_b with nrhs = 1 -- one chain of fused multiply-adds over j ascending from +0 on the widened stored
 * elements, no term skipped --, and
 *     x'[d_first[b] + i] = fma(omega, z_b[i], x[d_first[b] + i]).
 * Rows in no block are not written.  The blocks must not overlap one another, and d_xnew must not meet d_x, d_b, the
 * matrix or the store: this is a Jacobi sweep, every block reads the old x.  The residual never goes to global memory.
 *
 * Both calls take the handle's mutex and stream and are asynchronous on the context's stream, under profiling class 3:
 * one launch per lane class that has members -- the list of mi32_vbatch_apply_launches, at most five -- no workspace,
 * no memset, no atomics, no status.  A NULL required pointer (every pointer below is required), an index_bytes other
 * than 4 or 8 or a plan of another device is MI32_BAD_SHAPE, decided before the context is touched. */
#ifndef MAT_INV_32_RELAX_H
#define MAT_INV_32_RELAX_H

#include "mat_inv_32_stored.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The residual alone: d_r is a DEVICE array of `batch` device pointers, member b's n_b residuals dense at d_r[b] (the
 * packed right-hand side of mi32_apply_stored_device with nrhs = 1).  Blocks may overlap here; the members of d_r must
 * not overlap one another or any input. */
int mi32_csr_block_residual_device(mi32_handle_t h, mi32_vbatch_t p, const void *d_row_ptr, const void *d_col,
                                   int index_bytes, const float *d_val, const long long *d_first, const float *d_x,
                                   const float *d_b, float *const *d_r);
int mi32_csr_block_residual_device_f64(mi32_handle_t h, mi32_vbatch_t p, const void *d_row_ptr, const void *d_col,
                                       int index_bytes, const double *d_val, const long long *d_first, const double *d_x,
                                       const double *d_b, double *const *d_r);

/* One sweep: d_store, d_offset and d_format as in mi32_apply_stored_device. */
int mi32_csr_relax_stored_device(mi32_handle_t h, mi32_vbatch_t p, const void *d_row_ptr, const void *d_col,
                                 int index_bytes, const float *d_val, const long long *d_first, const void *d_store,
                                 const long long *d_offset, const int *d_format, const float *d_x, const float *d_b,
                                 float omega, float *d_xnew);
int mi32_csr_relax_stored_device_f64(mi32_handle_t h, mi32_vbatch_t p, const void *d_row_ptr, const void *d_col,
                                     int index_bytes, const double *d_val, const long long *d_first, const void *d_store,
                                     const long long *d_offset, const int *d_format, const double *d_x, const double *d_b,
                                     double omega, double *d_xnew);

#ifdef __cplusplus
}
#endif
#endif
