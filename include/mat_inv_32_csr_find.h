/* mat_inv_32_csr_find.h -- finding the block-Jacobi blocks of a sparse matrix: the stage in front of the sparse set-up
 * calls of mat_inv_32_csr.h, which take the block orders from the caller.  A header of its own beside that one (whose
 * two gather calls it leaves as they are), on mat_inv_32_c.h for the handle and the status codes; same library, same
 * conventions. */
#ifndef MAT_INV_32_CSR_FIND_H
#define MAT_INV_32_CSR_FIND_H

#include <stddef.h>

#include "mat_inv_32_c.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Supervariable agglomeration (Anzt, Dongarra, Flegar, Higham, Quintana-Orti; Ginkgo's find_natural_blocks plus
 * agglomerate_supervariables) on the sparsity pattern of a square N x N matrix in CSR on the device: d_row_ptr[N + 1]
 * and d_col[nnz] of ONE index type, int32_t (index_bytes 4) or int64_t (index_bytes 8), N >= 1.  Values are not read.
 *
 * The result is fixed bit for bit, integers only:
 *   1. nat[0] = 1; for i >= 1, nat[i] = 0 if rows i - 1 and i hold the same number of entries and the same column
 *      indices IN STORED ORDER, else 1.  Two empty rows are equal.  Rows that hold the same set in a different stored
 *      order are DIFFERENT: a caller whose rows are not sorted sorts them first (torch's CSR tensors are sorted).
 *      Indices are compared as stored and are not range-checked.
 *   2. A natural run is cut every max_order rows: with run(i) the largest j <= i that has nat[j] = 1,
 *      sv[i] = nat[i] or ((i - run(i)) % max_order == 0).
 *   3. agglomerate == 0: start = sv.  Otherwise the block starts are the orbit of row 0 under
 *      next(i) = the largest p in (i, i + max_order] with (p == N or sv[p]):
 *      a block takes consecutive supervariables while their rows sum to at most max_order.
 * d_start[N], one byte per row: 1 where a block begins, else 0; every element is written exactly once.  The block orders
 * are the gaps between the ones (and from the last one to N): they sum to N and each is in 1 ... max_order.
 *
 * d_work is the caller's temporary memory, 16-byte aligned, of at least the bytes mi32_csr_find_blocks_work_bytes
 * answers for n: 2 bytes per row, 8 per tile of 128 rows and 140 per chunk of 3968 rows, 2.1 bytes per row in all.  The
 * query is pure host code, linear and monotone in n; MI32_BAD_SHAPE for n < 1 or a NULL bytes.  What the memory holds
 * before and after a call is unspecified; two calls in flight on different streams need a d_work each.  The context's
 * workspace is not used.  d_start and d_work must not overlap the matrix or one another.
 *
 * Five launches (three without agglomeration), no atomics, no memset, no status: rows are compared pairwise, a group of
 * 16 lanes on a row pair and five rows' entries in flight per group; run starts are a prefix maximum per tile, then
 * over the tile summaries; the orbit is found per chunk for every one of the at most 128 rows it can enter the chunk
 * at, by pointer jumping in LDS, one workgroup chains the chunks, and every chunk marks its part from its real entry.
 * A NULL h, d_row_ptr, d_col, d_start or d_work, n < 1, an index_bytes other than 4 or 8, a max_order outside
 * 1 ... 128, a work_bytes below the query's answer or a d_work that is not 16-byte aligned is MI32_BAD_SHAPE, decided
 * before the context is touched.  The context's mutex and stream; its algorithm and pivoting settings are ignored.
 * Asynchronous on the context's stream under profiling class 3, that of the CSR gather. */
int mi32_csr_find_blocks_work_bytes(long long n, size_t *bytes);
int mi32_csr_find_blocks_device(mi32_handle_t h, long long n, const void *d_row_ptr, const void *d_col,
                                int index_bytes, int max_order, int agglomerate,
                                unsigned char *d_start, void *d_work, size_t work_bytes);
/* the rows of a chunk: what a caller that wants to test the seams between chunks places its cases by */
int mi32_csr_find_blocks_chunk_rows(void);

#ifdef __cplusplus
}
#endif
#endif
