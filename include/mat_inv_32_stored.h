/* mat_inv_32_stored.h -- block inverses stored in reduced precision per block, and applied from that store: the
 * per-block adaptive-precision block-Jacobi of Anzt, Dongarra, Flegar, Higham and Quintana-Orti.  A header of its own
 * beside mat_inv_32_c.h, which it includes for the handle, the plan and the status codes; same library, same
 * conventions.
 *
 * STORAGE FORMATS.  A member's format code is an int:
 *     code  format                                       bytes  unit roundoff  smallest normal  largest finite
 *     0     native: the working type T, float or double  4 / 8
 *     1     IEEE float32 (working type double only)      4      2^-24          2^-126           (2 - 2^-23) 2^127
 *     2     IEEE float16                                 2      2^-11          2^-14            65504
 *     3     bfloat16                                     2      2^-8           2^-126           (2 - 2^-7) 2^127
 * Narrowing is round-to-nearest-even with IEEE results: overflow gives +-inf, gradual underflow gives subnormals and
 * signed zeros, a NaN stays a NaN (payload unspecified).  From double to a 16-bit format the value goes through float
 * first: two roundings, part of the definition (1 + 2^-11 + 2^-30 becomes 1.0 in float16).  bfloat16 from float is
 * (u + 0x7FFF + ((u >> 16) & 1)) >> 16 on the bits of a non-NaN.  Widening to T is exact.
 *
 * THE STORE is one byte buffer: member b starts at byte offset off_b, off_0 = 0 and off_{b+1} = round_up_8(off_b +
 * n_b^2 bytes(F_b)), in the caller's member order, row-major and dense (leading dimension n_b), each member in its own
 * format.  Bytes between members are never written and never read.  d_store must be aligned to 8 bytes.
 *
 * Every call below takes the handle's mutex and stream and is asynchronous on the context's stream, under profiling
 * class 3: one launch per lane class that has members -- the list of mi32_vbatch_apply_launches, at most five -- no
 * workspace, no memset, no atomics, no status.  A NULL required pointer, nrhs <= 0 or a plan of another device is
 * MI32_BAD_SHAPE, decided before the context or the plan is read.  A format code the working type does not take is
 * the caller's error.  All arrays are device memory of `batch` entries in the caller's member order. */
#ifndef MAT_INV_32_STORED_H
#define MAT_INV_32_STORED_H

#include "mat_inv_32_c.h"

#define MI32_STORE_NATIVE 0
#define MI32_STORE_FLOAT32 1
#define MI32_STORE_FLOAT16 2
#define MI32_STORE_BFLOAT16 3

#ifdef __cplusplus
extern "C" {
#endif

/* Block statistics: d_stats[3 b ... 3 b + 2] = norm1, absmax, absmin of member b (row-major at d_a[b], rows d_lda[b]
 * elements apart; a NULL d_lda means the member's order).  norm1 = max_j c_j where each column sum c_j starts at +0 and
 * adds |a_ij| in double for i = 0 ... n-1 ascending; absmax = max |a_ij|; absmin = min |a_ij| over the nonzero
 * entries, +inf where every entry is zero.  If any entry is a NaN all three are NaN; infinities propagate.  Padding
 * behind a row is never read. */
int mi32_block_stats_device(mi32_handle_t h, mi32_vbatch_t p, const float *const *d_a, const int *d_lda,
                            double *d_stats);
int mi32_block_stats_device_f64(mi32_handle_t h, mi32_vbatch_t p, const double *const *d_a, const int *d_lda,
                                double *d_stats);

/* Narrow member b (row-major at d_x[b], rows d_ldx[b] elements apart, NULL: its order) to format d_format[b] and write
 * its n_b^2 elements at d_store + d_offset[b].  Every element is written exactly once, nothing else is. */
int mi32_store_inverses_device(mi32_handle_t h, mi32_vbatch_t p, const float *const *d_x, const int *d_ldx,
                               const int *d_format, const long long *d_offset, void *d_store);
int mi32_store_inverses_device_f64(mi32_handle_t h, mi32_vbatch_t p, const double *const *d_x, const int *d_ldx,
                                   const int *d_format, const long long *d_offset, void *d_store);

/* Z_b = widen(X_b) R_b from the store, with the arithmetic of mi32_apply_device_vbatched unchanged: per component one
 * chain of fused multiply-adds in T over j ascending from +0, no term skipped.  The result is bit-identical to
 * mi32_apply_device_vbatched on the widened members.  R, Z, d_ldr, d_ldz and nrhs as there; a member may be applied in
 * place (z[b] == r[b], ldz[b] == ldr[b]); Z must not meet the store. */
int mi32_apply_stored_device(mi32_handle_t h, mi32_vbatch_t p, const void *d_store, const long long *d_offset,
                             const int *d_format, const float *const *d_r, const int *d_ldr, int nrhs,
                             float *const *d_z, const int *d_ldz);
int mi32_apply_stored_device_f64(mi32_handle_t h, mi32_vbatch_t p, const void *d_store, const long long *d_offset,
                                 const int *d_format, const double *const *d_r, const int *d_ldr, int nrhs,
                                 double *const *d_z, const int *d_ldz);

#ifdef __cplusplus
}
#endif
#endif
