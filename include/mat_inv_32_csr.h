/* mat_inv_32_csr.h -- the sparse set-up calls of libmat_inv_32.so: from a CSR matrix to the blocks that
 * mi32_inv_device_vbatched inverts and mi32_apply_device_vbatched applies.  A header of its own beside
 * mat_inv_32_c.h, which it includes for the handle, the plan and the status codes; same library, same conventions. */
#ifndef MAT_INV_32_CSR_H
#define MAT_INV_32_CSR_H

#include "mat_inv_32_c.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Gather square blocks of a sparse matrix into the members of a plan (mixed orders 1 ... 128, order 128 included): the
 * set-up half of a block-Jacobi preconditioner, from the CSR matrix to the blocks mi32_inv_device_vbatched inverts in
 * place and mi32_apply_device_vbatched applies.  No dense N x N copy exists at any point.  The matrix is square, N x N,
 * in CSR on the device: d_row_ptr[N + 1] and d_col[nnz] of ONE index type, int32_t (index_bytes 4) or int64_t
 * (index_bytes 8), d_val[nnz].  d_first: device int64[batch]; member b is the block of rows AND columns
 * d_first[b] ... d_first[b] + n_b - 1, which must lie inside the matrix.  Consecutive diagonal blocks have d_first equal
 * to the exclusive prefix sum of the orders; any other d_first is allowed, overlapping blocks included (additive-Schwarz
 * subdomains).  d_out: DEVICE array of `batch` device pointers; member b is row-major with rows d_ldout[b] elements
 * apart (device int[batch]; a NULL d_ldout means the member's order).  Element alignment is all a member needs.
 *
 * The result is fixed bit for bit:
 *     out[b][i * ld + j] = the stored value of entry (d_first[b] + i, d_first[b] + j), copied -- a stored -0.0, NaN,
 *                          infinity or subnormal arrives as stored --, and +0.0 where the CSR stores no such entry.
 * Column indices inside a row need no order and a row may be empty.  An entry whose column lies outside the block, or
 * outside [0, N), is skipped.  Duplicate (row, column) pairs are the caller's error: which one arrives is unspecified.
 * Every element of every member is written exactly once; nothing between n_b and d_ldout[b] and nothing outside the
 * members is written.  Of the matrix only d_row_ptr[r], d_row_ptr[r + 1] and the d_col and d_val entries between them
 * are read, for the rows r of the blocks.  Offsets into d_col, d_val and the members are 64-bit.  Members that overlap
 * one another in memory, or the matrix, are undefined.
 *
 * One launch per lane class that has members -- the list of mi32_vbatch_apply_launches, at most five -- no workspace,
 * no memset, no status (a copy cannot fail) and no atomics.  A group of 8 / 16 / 32 / 64 lanes owns one member (256 /
 * lanes members per workgroup), the two waves of a 128-thread workgroup one of order 65 ... 128; per block row a group
 * zeroes a row buffer in LDS, scans the CSR row with consecutive lanes on consecutive entries, and writes the buffer
 * out, four rows in flight at a time.  A NULL h, p, d_row_ptr, d_col, d_val, d_first or d_out, an index_bytes other than 4 or 8 or
 * a plan of another device is MI32_BAD_SHAPE, decided before the context is touched.  The context's mutex and stream;
 * its algorithm and pivoting settings are ignored.  Asynchronous on the context's stream under profiling class 3. */
int mi32_csr_blocks_device(mi32_handle_t h, mi32_vbatch_t p, const void *d_row_ptr, const void *d_col, int index_bytes,
                           const float *d_val, const long long *d_first, float *const *d_out, const int *d_ldout);
int mi32_csr_blocks_device_f64(mi32_handle_t h, mi32_vbatch_t p, const void *d_row_ptr, const void *d_col,
                               int index_bytes, const double *d_val, const long long *d_first, double *const *d_out,
                               const int *d_ldout);

#ifdef __cplusplus
}
#endif
#endif
