/*
 * mat_inv_32_c.h -- C ABI of libmat_inv_32.so (MI355X / gfx950).
 *
 * The reference exposes exactly one entry point for this path,
 *     std::vector<float> matrix_inv_32(std::vector<float>, int)
 *     (/root/reference/Matlab/mat_inv_32.h:4, body mat_inv_32.cpp:11-395),
 * a C++-ABI function that MATLAB binds through clibgen (README.md:31-52).
 * mi32_matrix_inv_32() below is its flat-pointer twin (what a ctypes / cgo /
 * JNI / MEX binding would call); include/mat_inv_32.h keeps the original C++
 * signature on top of it.  Everything else here is additive: a handle so that
 * the device context, stream and workspace outlive a call (the reference
 * rebuilds platform/context/queue/programs per call, mat_inv_32.cpp:238-290),
 * device-pointer entry points for device-resident batches, and a device-side
 * residual check (the reference's matrix_multiply.cpp verification helper).
 *
 * Plain pointers and sizes only; no C++ or torch types.  All functions
 * return an mi32_status unless stated otherwise.
 */
#ifndef MAT_INV_32_C_H
#define MAT_INV_32_C_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The status looks at the input's entries and at the pivots only.  MI32_OK therefore does not say that the inverse is
 * finite: where the RESULT overflows with every pivot finite it holds +-inf and NaN.  With every intermediate finite
 * all routes return the oracle's bits.  Once a pivot row holds an infinity they part in a documented way
 * (tests/test_gpu_overflow.py): the sweep and the one-launch routes skip an exact-zero multiplier, as the reference
 * does; the blocked fp32 route and the blocked fp64 no-pivot route multiply it through, and fma(-0, +-inf, x) is a NaN
 * -- on a block-structured input they can return NaN columns where the sweep returns zeros and infinities; the
 * blocked fp64 route follows its composite order (oracle: gjo_matrix_inv_64_blocked), which near that boundary can
 * meet a non-finite pivot, and report MI32_SINGULAR, on an input the sweep inverts with MI32_OK. */
typedef enum mi32_status {
    MI32_OK = 0,
    MI32_BAD_SHAPE = 1,     /* reference: returns {} (mat_inv_32.cpp:206-215)                 */
    MI32_SINGULAR = 2,      /* invalid matrix: a zero / NaN / infinite pivot was met, or the input holds a
                             * non-finite entry (reference: inf/NaN out, unchecked; README.md:54 "empty vector") */
    MI32_RUNTIME_ERROR = 3  /* HIP error (reference: unreachable catch, mat_inv_32.cpp:391); as a per-matrix
                             * status: a shared panel lost a partner workgroup, that inverse is NaN-filled */
} mi32_status;

typedef enum mi32_algo {
    MI32_ALGO_AUTO = 0,
    /* One fused launch per pivot step over the whole working matrix: the
     * literal restatement of the reference's 5-kernel step (maxPivot,
     * finalMaxPivot, pivotElements, fixRow, fixColumn; mat_inv_32.cpp:317-362).
     * HBM-bound; bit-identical to the CPU oracle. */
    MI32_ALGO_SWEEP = 1,
    /* Same elimination with the column updates delayed and applied as rank-k
     * updates on the fp32 matrix cores (v_mfma_f32_32x32x2_f32); the pivot
     * search / swap / normalise / eliminate steps run on a register-resident
     * panel.  Equal to SWEEP up to fp32 rounding. */
    MI32_ALGO_BLOCKED = 2,
    /* Large batches of small matrices (n <= 64): one launch in which a group of 8 / 16 / 32 / 64 lanes keeps one
     * matrix in registers from the first pivot search to the un-permuted inverse -- one global read and one
     * global write per element, no workspace, any batch size the buffers hold (the other two paths stop at
     * 65535 members).  The arithmetic of SWEEP, element by element: bit-identical to the CPU oracle, in fp32
     * and fp64, with and without pivoting.  Never chosen by AUTO; for n > 64 it resolves to what AUTO
     * resolves to. */
    MI32_ALGO_RESIDENT = 3,
    /* Large batches of matrices of order 65 ... 128: one launch in which one workgroup of 256 threads keeps one
     * matrix in its registers (40 / 48 / 56 / 64 rows per thread, so an order-65 matrix does not pay for 128 rows)
     * from the load to the un-permuted inverse -- one global read and one global write per element, no workspace,
     * any batch size the buffers hold.  The arithmetic of SWEEP, element by element: bit-identical to the CPU
     * oracle, in fp32 and fp64, with and without pivoting.  Never chosen by AUTO; n <= 64 resolves to RESIDENT
     * (one setting serves orders on both sides of 64), n > 128 to what AUTO resolves to. */
    MI32_ALGO_WORKGROUP = 4,
    /* Large batches of fp32 matrices of order 129 ... 256: one launch in which one workgroup of 768 (orders up to 192)
     * or 1024 threads keeps one matrix in its registers (4 slabs of 192 / 256 column lanes, 40 / 48 / 56 / 64 rows per
     * thread for orders up to 160 / 192 / 224 / 256) from the load to the un-permuted inverse -- one global read and
     * one global write per element, no workspace, any batch size the buffers hold.  The arithmetic of SWEEP, element
     * by element: bit-identical to the CPU oracle, with and without pivoting.  fp32 only: a 256 x 256 fp64 matrix is
     * the whole register file of a compute unit.  Never chosen by AUTO; n <= 64 resolves to RESIDENT and 65 ... 128 to
     * WORKGROUP (one setting serves every small order), n > 256 and every fp64 call above 128 to what AUTO resolves
     * to.  mi32_solve_device* (orders up to 127) and the variable-size calls (orders up to 128) do not reach it. */
    MI32_ALGO_WIDE = 5
} mi32_algo;

typedef struct mi32_context *mi32_handle_t;

/* ---- drop-in twin of matrix_inv_32 (host pointers) ----------------------- */
/* a_rowmajor: a_len floats, row-major n x n (the reference's integer-division
 * guard accepts a_len in [n*n, n*n+n); the tail is ignored).  inv_rowmajor: n*n
 * floats, written only on MI32_OK / MI32_SINGULAR.  Uses a process-wide default
 * context (device MI32_DEVICE or 0), created on first use, mutex-protected. */
int mi32_matrix_inv_32(const float *a_rowmajor, size_t a_len, int n, float *inv_rowmajor);

/* batch of independent n x n matrices, contiguous (batch x n x n); status may be
 * NULL, else receives one mi32_status per matrix.  Returns the worst status. */
int mi32_matrix_inv_32_batched(const float *a, int n, int batch, float *inv, int *status);

/* The same batch over ngpus GPUs of this node (ngpus <= 0: every visible device) -- what replaces the reference's
 * platforms[0] / devices[0] (Matlab/mat_inv_32/mat_inv_32/mat_inv_32.cpp:239-244) for the callers the reference has
 * (C++ and MATLAB: no launcher, no Python).  One context and one host thread per GPU; GPU g owns the matrices
 * [g * ceil(batch / ngpus), min(batch, (g + 1) * ceil(batch / ngpus))), copies ITS OWN shard host -> device, inverts it
 * and copies it back.  No data-path exchange between the GPUs (independent matrices); the return value is the worst
 * status, status[] (may be NULL) one word per matrix.  Every matrix's inverse is bit-identical to what
 * mi32_matrix_inv_32_batched gives for it alone.  ngpus > visible devices is MI32_BAD_SHAPE unless
 * MI32_MULTI_OVERSUBSCRIBE=1 maps logical GPU g onto device g % visible (tests, single-GPU hosts). */
int mi32_matrix_inv_32_batched_multi(const float *a, int n, int batch, float *inv, int *status, int ngpus);
/* the shard of GPU g of ngpus: [*lo, *hi) (empty for the GPUs a ragged batch leaves without work); needs no device */
int mi32_shard_range(int batch, int ngpus, int g, int *lo, int *hi);

/* ---- context ------------------------------------------------------------- */
int mi32_create(mi32_handle_t *out, int device /* HIP ordinal, <0 = current */);
int mi32_destroy(mi32_handle_t h);
/* hipStream_t on which every launch of this context is enqueued from now on; NULL is
 * HIP's default stream.  A new context starts on a non-blocking stream of its own.  The
 * caller keeps ownership of the stream it passes. */
int mi32_set_stream(mi32_handle_t h, void *hip_stream);
int mi32_set_algo(mi32_handle_t h, int algo);
/* tuning knobs of the blocked path: sub-panel width (4/8/16/32, capped by what fits in registers) and the outer
 * block width (multiple of the sub-panel width, <= 512); 0 keeps the default */
int mi32_set_blocking(mi32_handle_t h, int panel_width, int block_width);
/* look-ahead of the blocked path (second stream; on by default for single matrices of more than 4096 padded rows) */
int mi32_set_lookahead(mi32_handle_t h, int enable);
/* bytes of device workspace a call of this shape needs (excluding in/out) */
size_t mi32_workspace_bytes(int n, int batch, int algo);
/* allocate the workspace up front so that later calls never hipMalloc */
int mi32_reserve(mi32_handle_t h, int n, int batch);

/* ---- device-resident entry points ---------------------------------------- */
/* d_a, d_inv: device pointers, batch x n x n fp32 row-major, contiguous; d_a is
 * not modified, d_inv may not alias d_a.  d_status: device int[batch] (may be
 * NULL: the context then keeps the status words itself).  Asynchronous: everything is enqueued on the context's stream and the
 * call returns without synchronising.  The call shape, minus the host copies,
 * of mat_inv_32.cpp:292-376 (makeAugmented -> N pivot steps -> getInverted).
 *
 * The memory contract of the dense device calls -- mi32_inv_device*, mi32_inv_det_device*,
 * mi32_inv_det_any_device*, mi32_solve_device* and mi32_residual_device -- on every route (sweep, blocked, the
 * one-launch paths, either precision, with pivoting and without, a batch split in two halves included):
 *   - element alignment is all d_a, d_inv, d_b, d_x, d_status, d_det_mant and d_det_exp need;
 *   - nothing outside batch * n * n elements of d_a and d_inv (batch * n * nrhs of d_b and d_x), batch status words
 *     and batch determinant pairs is read or written: padded rows and columns, tail groups and tail workgroups stay
 *     inside the context's workspace or in registers.  With d_inv == NULL (the determinant-only forms) and with
 *     d_status == NULL nothing is stored in their place;
 *   - d_a is not modified on any route, and d_b only when d_x == d_b.
 * tests/test_gpu_memory_contract.py pins this with views carved out of larger buffers, one element off a 256-byte
 * boundary, between NaN margins (inputs) and sentinel margins (outputs, status, determinant pair). */
int mi32_inv_device(mi32_handle_t h, const float *d_a, int n, int batch, float *d_inv, int *d_status);

/* ---- fp64 (the reference's matrix_inversion_FP64, matrix_inversion/headers.h:9) ---------------- */
/* Same Gauss-Jordan step sequence in double.  N < 256: the sweep path (one fused launch per pivot step over the whole
 * matrix, 16 N (N+1) bytes per step), bit-identical to the oracle's fp64 restatement.  N >= 256: blocked -- the same
 * fused steps on a window of bw columns and one rank-bw update per block on v_mfma_f64_16x16x4_f64 (mi32_blocked64.hip),
 * bit-identical to the oracle's fp64 blocked mirror.  Host-pointer twin of the C++
 * function in mat_inv_64.h, and the device-resident batched form (asynchronous on the context's stream). */
int mi32_matrix_inv_64(const double *a_rowmajor, size_t a_len, int n, double *inv_rowmajor);
/* The reference's no-pivot variant (matrix_inversion_no_pivots.cpp:10, headers.h:11): the same steps with the
 * diagonal entry as pivot, no search and no swap -- for diagonally dominant inputs.  Host-pointer twin in double
 * (as the reference ships it); mi32_set_pivoting(h, 0) selects it for the device-resident calls of a context, in
 * either precision.  Both take a blocked path from 512 rows on (below, and under MI32_ALGO_SWEEP, the sweep kernels;
 * an explicit MI32_ALGO_BLOCKED at any order).  fp32: without a search the W pivot rows of a sub-panel are known in
 * advance, so the "panel" is their W x W diagonal block and every other row is taken through the W steps by the
 * update tiles on the whole chip (N = 4096: 5.7 ms against 92 ms for the sweep kernels).  fp64 (mi32_nopivot64.hip):
 * per block of bw steps the bw x bw diagonal block on one workgroup, the block columns of every other row and the
 * pivot rows' entries of every other column on the whole chip, one rank-bw update on v_mfma_f64_16x16x4_f64
 * (N = 4096: 8 ms against 240 ms for the sweep kernels).  Both are bit-identical to the step-by-step restatement,
 * with two caveats for fp64: a zero multiplier is multiplied through rather than skipped, so the sign of a zero
 * entry can differ, and the equality assumes finite intermediates.  A zero / non-finite diagonal entry or a
 * non-finite input entry -> MI32_SINGULAR (per batch member; a singular member's output values are unspecified). */
int mi32_matrix_inversion_no_pivots(const double *a_rowmajor, size_t a_len, int n, double *inv_rowmajor);
int mi32_set_pivoting(mi32_handle_t h, int enable);
int mi32_inv_device_f64(mi32_handle_t h, const double *d_a, int n, int batch, double *d_inv, int *d_status);
/* outer block width of the fp64 blocked path for this order (the step kernels run on a window of that many columns,
 * one rank-bw update on the fp64 matrix cores per block; 64, 128 or 256), or, with pivoting off, of the fp64 no-pivot
 * path (64 or 128); 0 where the unblocked sweep is used (N < 256, N < 512 with pivoting off, MI32_ALGO_SWEEP) */
int mi32_resolve_blocking_f64(mi32_handle_t h, int n, int *block_width);

/* ---- variable-size batches: members of mixed orders, each at its own pointer and leading dimension ---------------- */
/* One call inverts `batch` members of any orders from 1 to 128 (block-Jacobi blocks, per-element blocks, the diagonal
 * blocks of a larger matrix) on the register-resident and workgroup-resident kernels: the members are binned once by
 * order into the eight kernel classes -- orders up to 8 / 16 / 32 / 64 (lanes per matrix) and up to 80 / 96 / 112 / 128
 * (rows per thread) -- and a call enqueues one status memset and one launch per class that has members, at most eight.
 * Every member does the arithmetic of the uniform paths, so every member is bit-identical to the CPU oracle, in fp32
 * and fp64, with pivoting and without (the context's setting).
 *
 * The binning itself, pure host code (no device): perm[0 .. batch) <- the member indices in ascending order of
 * their orders, members of equal order in their original sequence (a counting sort, O(batch)); class_begin[0 .. 9)
 * <- class k takes perm[class_begin[k] .. class_begin[k + 1]).  batch <= 0, a NULL argument or an order outside
 * 1 ... 128 is MI32_BAD_SHAPE. */
int mi32_vbatch_bin(const int *orders, int batch, int *perm, int *class_begin /* int[9] */);
/* A plan: bins once and uploads the orders and the sorted member list to the context's device -- 8 bytes per member,
 * the only device memory the feature owns.  `orders` is a HOST array and may go away when the call returns.  Same
 * error rules as the binning.  The plan is immutable: it may be used any number of times, from any thread, and from
 * any context on the same device. */
typedef struct mi32_vbatch *mi32_vbatch_t;
int mi32_vbatch_create(mi32_handle_t h, const int *orders, int batch, mi32_vbatch_t *out);
/* frees the plan; safe while calls that use it are still in flight (freeing device memory waits for them) */
int mi32_vbatch_destroy(mi32_vbatch_t p);
/* *batch (may be NULL) <- the members of the plan, class_begin[0 .. 9) (may be NULL) <- its class ranges */
int mi32_vbatch_info(mi32_vbatch_t p, int *batch, int *class_begin /* int[9] */);
/* d_a, d_inv: DEVICE arrays of `batch` device pointers, member b row-major with rows d_lda[b] / d_ldinv[b] elements
 * apart; element alignment is all a member needs.  d_lda, d_ldinv: device int[batch], either may be NULL = the
 * member's order; a leading dimension below the order is the caller's error and is not checked on the device.
 * d_status: device int[batch] in the caller's member order, NULL = the context keeps the words itself.  Padding --
 * the elements between column n[b] and the leading dimension -- is never read and never written: a NaN there does
 * not flag the member.  A member may be inverted in place (d_inv[b] == d_a[b] with equal leading dimensions: every
 * element of a member is in registers before its first store); members that overlap in any other way, with
 * themselves or with one another, are undefined.  Any batch size the buffers hold.  Asynchronous on the context's
 * stream; the launches are recorded under profiling class 2.  A plan of another device is MI32_BAD_SHAPE. */
int mi32_inv_device_vbatched(mi32_handle_t h, mi32_vbatch_t p, const float *const *d_a, const int *d_lda,
                             float *const *d_inv, const int *d_ldinv, int *d_status);
int mi32_inv_device_vbatched_f64(mi32_handle_t h, mi32_vbatch_t p, const double *const *d_a, const int *d_lda,
                                 double *const *d_inv, const int *d_ldinv, int *d_status);

/* ---- the determinant beside the inverse (orders 1 ... 128) -------------------------------------------------------- */
/* The one-launch batch paths hold every pivot value and every row exchange of the elimination, and det A =
 * (-1)^swaps * prod pivots: these calls return it with the inverse, from the same launch, at 12 bytes per member.
 * The determinant is a pair like frexp's: det = d_det_mant[b] * 2^d_det_exp[b], |mantissa| in [0.5, 1); it cannot
 * overflow.  log|det| = log|mantissa| + exponent * ln 2, its sign is the mantissa's.  The pair is defined by a fixed
 * recurrence of IEEE double operations.  It starts at m = 1.0, e = 0; after pivot step r = 0 ... n-1 has chosen its
 * pivot value piv and knows whether row r and the pivot row differ (swap; never with pivoting off), while the member is
 * not flagged:
 *     (pm, pe) = frexp((double)piv);   if (swap) m = -m;   (m, k) = frexp(m * pm);   e += pe + k;
 * A member with status MI32_OK: (m, e).  A member flagged MI32_SINGULAR: the accumulation stops at the step that
 * flags it (it never starts for a non-finite input entry) and the pair is (+0.0, 0) when pivoting is on and the flag
 * was raised by an exactly zero pivot after finite input and finite earlier pivots -- the rest of that column is
 * exactly zero, so the computed determinant is 0 -- and (NaN, 0) in every other case: a non-finite input entry, a NaN
 * or infinite pivot, or any flag with pivoting off (a zero diagonal entry does not imply det = 0).
 *
 * 1 <= n <= 128.  These calls always run on the register-resident (n <= 64) or the workgroup-resident (65 ... 128)
 * kernels, whatever mi32_set_algo says: every path gives the same inverse bits, so the setting shows in no result.
 * The inverse and the status equal those of mi32_inv_device* bit for bit.  d_inv may be NULL (in the variable-size
 * call: the pointer array): the inverse is then not stored, only status and determinant.  d_det_mant: device
 * double[batch], d_det_exp: device int[batch], in the order of d_status (the caller's member order).  n > 128, a null
 * d_det_mant / d_det_exp, batch <= 0 or a plan of another device -> MI32_BAD_SHAPE.  Everything else as for
 * mi32_inv_device / mi32_inv_device_vbatched: the context's pivoting setting, a null d_status, in-place members of the
 * variable-size call, asynchronous on the context's stream under profiling class 2. */
int mi32_inv_det_device(mi32_handle_t h, const float *d_a, int n, int batch, float *d_inv, int *d_status,
                        double *d_det_mant, int *d_det_exp);
int mi32_inv_det_device_f64(mi32_handle_t h, const double *d_a, int n, int batch, double *d_inv, int *d_status,
                            double *d_det_mant, int *d_det_exp);
/* The same pair at ANY order mi32_inv_device* takes.  1 <= n <= 128: exactly mi32_inv_det_device*, same kernels, same
 * bits.  Above, the call runs the route mi32_inv_device* would run on this context -- the same algorithm setting,
 * blocking, pivoting setting, look-ahead and batch split -- and adds the determinant: every step's pivot is recorded
 * in step order (it is in global memory after each launch, or one register away in a step kernel, whose det twin
 * stores it), and one small kernel per call runs the recurrence above over a member's list.  The row exchanges enter as
 * one parity at the end, which gives the same bits as a flip per step (IEEE multiplication and frexp are
 * sign-symmetric); the identity padding's steps (pivot 1, no exchange) are left out.  A member given up with
 * MI32_RUNTIME_ERROR by a shared panel: (NaN, 0).  Inverse and status are those of mi32_inv_device* bit for bit.
 * d_inv == NULL: the elimination runs, the final un-permutation and store are skipped.  A null handle, input,
 * d_det_mant or d_det_exp, n <= 0, batch <= 0 or d_a == d_inv -> MI32_BAD_SHAPE, decided before the context is
 * touched.  The pivot lists live in memory the context owns for these calls (4 or 8 bytes per padded row and member,
 * grown on demand; mi32_workspace_bytes and mi32_reserve do not count it); calls on one context are ordered by its
 * stream.  The added launches are recorded under profiling class 5.  On a context set to MI32_ALGO_WIDE an fp32 batch
 * of order 129 ... 256 is one launch here too: that path's determinant twin accumulates the pair in its registers, as
 * the kernels below 129 do -- no pivot list, no added launch, (+0.0, 0) / (NaN, 0) for a flagged member as above. */
int mi32_inv_det_any_device(mi32_handle_t h, const float *d_a, int n, int batch, float *d_inv, int *d_status,
                            double *d_det_mant, int *d_det_exp);
int mi32_inv_det_any_device_f64(mi32_handle_t h, const double *d_a, int n, int batch, double *d_inv, int *d_status,
                                double *d_det_mant, int *d_det_exp);
int mi32_inv_det_device_vbatched(mi32_handle_t h, mi32_vbatch_t p, const float *const *d_a, const int *d_lda,
                                 float *const *d_inv, const int *d_ldinv, int *d_status, double *d_det_mant,
                                 int *d_det_exp);
int mi32_inv_det_device_vbatched_f64(mi32_handle_t h, mi32_vbatch_t p, const double *const *d_a, const int *d_lda,
                                     double *const *d_inv, const int *d_ldinv, int *d_status, double *d_det_mant,
                                     int *d_det_exp);

/* ---- A X = B without the inverse (orders 1 ... 127) ------------------------------------------------------------------ */
/* The one-launch batch paths solve A X = B for every member by Gauss-Jordan on [A | B]: in those kernels a lane or
 * column past the order is idle, and a column of B placed there takes exactly the steps an augmented column takes --
 * the row exchange with the pivot row, prn = b[p] / piv, b[i] = fma(-f, prn, b[i]) for every other row (skipped when the
 * multiplier f == 0), b[r] = prn -- with the pivot row p, pivot piv and multipliers f of the elimination of A, whose
 * arithmetic is that of mi32_inv_device.  X is B's final content; no inverse is formed or stored.  With B = I, X is
 * mi32_inv_device's inverse bit for bit; its accuracy is that of inverse-times-B, not better.
 *
 * d_a: (batch, n, n) contiguous; d_b, d_x: (batch, n, nrhs) contiguous, row-major; d_x == d_b is allowed (a member's
 * loads all precede its stores), d_x must not be d_a.  d_status: device int[batch] or NULL as for mi32_inv_device;
 * MI32_SINGULAR for a zero, NaN or infinite pivot or a non-finite entry of A or of B -- the elimination goes on
 * regardless and that member's X is unspecified.  1 <= n <= 127: order 128 has no spare column, and it, larger orders,
 * a null pointer, batch <= 0 or nrhs <= 0 are MI32_BAD_SHAPE.
 *
 * One launch holds at most 64 - n columns beside an order n <= 32 (the member stays in one 64-lane group) and
 * 128 - n beside a larger one; more columns are cut into such chunks, full ones first, one launch each, and EVERY launch
 * repeats the elimination of A.  A chunk whose width n + columns is at most 64 runs on the register-resident kernels
 * (8 / 16 / 32 / 64 lanes by the width), a wider one on the workgroup-resident ones (40 rows per thread up to order
 * 80, then 48 / 56 / 64): an order 33 ... 64 with n + nrhs > 64 moves from a 64-lane group to a 256-thread workgroup.
 * Always these kernels, whatever mi32_set_algo says; the context's pivoting setting, stream and mutex as for
 * mi32_inv_device; asynchronous; the launches are recorded under profiling class 2. */
int mi32_solve_device(mi32_handle_t h, const float *d_a, int n, int batch, const float *d_b, int nrhs, float *d_x,
                      int *d_status);
int mi32_solve_device_f64(mi32_handle_t h, const double *d_a, int n, int batch, const double *d_b, int nrhs, double *d_x,
                          int *d_status);

/* The same for a variable-size batch (a plan of mi32_vbatch_create): one call solves A_b X_b = B_b for members of mixed
 * orders 1 ... 127, each at its own pointers and leading dimensions, with ONE nrhs for the call -- what applying a
 * block-Jacobi preconditioner needs, z = blockdiag(A)^-1 r.  d_a, d_b, d_x: DEVICE arrays of `batch` device pointers;
 * member b's A is n_b x n_b with rows d_lda[b] elements apart, its B and X are n_b x nrhs with rows d_ldb[b] / d_ldx[b]
 * elements apart.  d_lda, d_ldb, d_ldx: device int[batch]; a NULL d_lda means the member's order, a NULL d_ldb or
 * d_ldx means nrhs.  Padding is never read and never written.  A member may be solved in place, d_x[b] == d_b[b] with
 * d_ldx[b] == d_ldb[b] (a member's loads all precede its stores); X over A, and members that overlap in any other way,
 * with themselves or with one another, are undefined.  d_status as for mi32_inv_device_vbatched.
 *
 * Every member is treated exactly as mi32_solve_device treats a uniform batch of its order with the same nrhs: the same
 * chunks, the same kernel class per chunk, the same arithmetic, hence the same bits.  The plan's member list is sorted
 * by order; a call enqueues one status memset and, per maximal run of consecutive sorted members whose chunk sequences
 * agree (the same first column, column count and kernel instance for every chunk), one launch per chunk.  For nrhs = 1
 * that is at most eight launches whatever the orders -- the runs are the orders 1 ... 7, 8 ... 15, 16 ... 31, 32 ... 63,
 * 64 ... 80, 81 ... 96, 97 ... 112 and 113 ... 127 -- and an order with more columns than one launch holds takes launches
 * of its own, one per chunk; every launch of a member repeats the elimination of its A.  The context's pivoting setting;
 * the algorithm setting is ignored.  A NULL h, p, d_a, d_b or d_x, nrhs <= 0, a plan of another device or a plan that
 * holds a member of order 128 (no spare column; the plan stays valid for mi32_inv_device_vbatched) is MI32_BAD_SHAPE,
 * decided before the context is touched.  Asynchronous on the context's stream under profiling class 2. */
int mi32_solve_device_vbatched(mi32_handle_t h, mi32_vbatch_t p, const float *const *d_a, const int *d_lda,
                               const float *const *d_b, const int *d_ldb, int nrhs, float *const *d_x, const int *d_ldx,
                               int *d_status);
int mi32_solve_device_vbatched_f64(mi32_handle_t h, mi32_vbatch_t p, const double *const *d_a, const int *d_lda,
                                   const double *const *d_b, const int *d_ldb, int nrhs, double *const *d_x,
                                   const int *d_ldx, int *d_status);
/* The launches of such a call, pure host code (no device; the call itself walks this very list): launches[6 * i ...]
 * <- first, count (a range of the sorted member list), col0, cols (the columns of B), lanes per member of the
 * register-resident instance (0: the workgroup-resident kernel), its rows per thread (0: the register-resident kernel),
 * ordered by first, then by col0.  At most `capacity` launches are written (launches may be NULL when capacity is 0);
 * *count is always the full number.  MI32_BAD_SHAPE: a NULL orders or count, batch <= 0, nrhs <= 0, capacity < 0, an
 * order outside 1 ... 127. */
int mi32_vbatch_solve_launches(const int *orders, int batch, int nrhs, int *launches, int capacity, int *count);

/* Apply stored matrices to right-hand sides: Z_b = X_b R_b for every member of a plan (mixed orders 1 ... 128, order 128
 * included), with ONE nrhs >= 1 for the call.  With X_b a stored inverse (mi32_inv_device_vbatched) this is the
 * per-iteration half of a block-Jacobi preconditioner, z = blockdiag(A)^-1 r, at n^2 multiply-adds per member and column
 * where mi32_solve_device_vbatched repeats the elimination.  d_x, d_r, d_z: DEVICE arrays of `batch` device pointers;
 * member b's X is n_b x n_b with rows d_ldx[b] elements apart, its R and Z are n_b x nrhs with rows d_ldr[b] / d_ldz[b]
 * elements apart.  d_ldx, d_ldr, d_ldz: device int[batch]; a NULL d_ldx means the member's order, a NULL d_ldr or d_ldz
 * means nrhs.  Element alignment is all a member needs.  Padding is never read and never written.
 *
 * The arithmetic is fixed, so the result is reproducible bit for bit and a few lines of C restate it:
 *     z[i][k] = acc after:  acc = +0;  for j = 0 ... n-1 ascending:  acc = fma(x[i][j], r[j][k], acc)
 * one fused multiply-add per term in the element type.  No term is skipped -- a zero in X is multiplied through, NaN and
 * infinity propagate by IEEE rules -- and there is no status: a product cannot fail.  The kernels' layout (lanes per
 * member, tiles, column chunks) does not enter the result.
 *
 * A member may be applied in place, d_z[b] == d_r[b] with d_ldz[b] == d_ldr[b] (a member's loads of a chunk of columns
 * all precede its stores of that chunk); Z over X, and members that overlap in any other way, are undefined.  One
 * launch per lane class that has members -- at most five, whatever nrhs is: the columns are walked inside the kernel --
 * no workspace and no memset.  A NULL h, p, d_x, d_r or d_z, nrhs <= 0 or a plan of another device is MI32_BAD_SHAPE,
 * decided before the context is touched.  The context's mutex and stream; its algorithm and pivoting settings are
 * ignored.  Asynchronous on the context's stream under profiling class 3. */
int mi32_apply_device_vbatched(mi32_handle_t h, mi32_vbatch_t p, const float *const *d_x, const int *d_ldx,
                               const float *const *d_r, const int *d_ldr, int nrhs, float *const *d_z, const int *d_ldz);
int mi32_apply_device_vbatched_f64(mi32_handle_t h, mi32_vbatch_t p, const double *const *d_x, const int *d_ldx,
                                   const double *const *d_r, const int *d_ldr, int nrhs, double *const *d_z,
                                   const int *d_ldz);
/* The launches of such a call, pure host code (no device; the call itself walks this very list): launches[4 * i ...]
 * <- first, count (a range of the sorted member list), lanes per member (8 / 16 / 32 / 64 for the orders up to 8 / 16 /
 * 32 / 64; 128: one workgroup of 128 threads per member, the orders 65 ... 128), columns per chunk (8 for elem_bytes 4,
 * 4 for 8; the same for every launch), ordered by first.  At most `capacity` launches are written (launches may be NULL
 * when capacity is 0); *count is always the full number, at most five.  MI32_BAD_SHAPE: a NULL orders or count,
 * batch <= 0, nrhs <= 0, elem_bytes other than 4 or 8, capacity < 0, an order outside 1 ... 128. */
int mi32_vbatch_apply_launches(const int *orders, int batch, int nrhs, int elem_bytes, int *launches, int capacity,
                               int *count);

/* Device-side verification (the reference's matrix_multiply.cpp:17-36,193-200 and
 * the residual BASELINE.json gates): per matrix, d_out[3*b+0] = ||A X - I||_inf,
 * d_out[3*b+1] = ||X A - I||_inf, d_out[3*b+2] = sqrt(N) - ||A X||_F, all
 * accumulated in fp64.  d_out: device double[3*batch].  Any batch size.  A NaN operand
 * entry gives NaN in all three outputs of that member (and of no other); an infinite one
 * gives +inf in the norms it reaches (NaN where it meets a zero) and -inf or NaN in the
 * third.  Asynchronous. */
int mi32_residual_device(mi32_handle_t h, const float *d_a, const float *d_x, int n, int batch, double *d_out);

/* ---- per-phase timing (the reference's FP32_bench.cpp:256-443 timing slots) ---------- */
/* When enabled, every kernel launch of this context is bracketed by two HIP events
 * recorded on the launch stream.  mi32_get_profile synchronises those events and returns,
 * per kernel class, the summed milliseconds and the number of launches since the last
 * call.  Classes (MI32_KC_*): 0 init (makeAugmented), 1 sweep step, 2 panel steps (and
 * the one launch of the register-resident and workgroup-resident paths),
 * 3 in-block rank-w update, 4 rank-bw update (fp32 MFMA), 5 finish (getInverted),
 * 6 multiplier transposition in front of each rank-bw update (its A operand). */
#define MI32_KC_COUNT 7
int mi32_set_profiling(mi32_handle_t h, int enable);
int mi32_get_profile(mi32_handle_t h, double *ms_per_class, long long *launches_per_class, int nclasses);

/* The reference's benchmark twin (Res FP32_bench(vector<float>, int), FP32_bench.cpp:11; C++ signature in
 * mat_inv_bench.h): one host-pointer inversion that also fills times10[10] with the reference's timing vector
 * (FP32_bench.cpp:256-443), seconds:
 *   [0] queue/context (the cached default context: ~0 after the first call)   [1] buffers: staging + workspace
 *   allocation and the H2D copy (the reference's CL_MEM_COPY_HOST_PTR)        [2] program build: 0 (one AOT code
 *   object)   [3] makeAugmented = init kernel   [4] pivot = the panel kernels (search + swap + normalise, and
 *   the elimination of the panel's own columns)   [5] fixRow: 0, it has no launch of its own   [6] fixColumn =
 *   in-block + rank-bw updates (+ panel transposes), or the fused step launches of the sweep path
 *   [7] compute (wall time of the device-resident inversion)   [8] getInverted = un-permutation kernels + D2H
 *   [9] total.  Slots 3-6 and the kernel part of 8 are HIP-event durations on the launch stream. */
int mi32_bench_32(const float *a_rowmajor, size_t a_len, int n, float *inv_rowmajor, double *times10);
/* the fp64 twins (Res FP64_bench / no_pivots_bench, headers.h:14,16): pivoting = 0 selects the no-pivot variant */
int mi32_bench_64(const double *a_rowmajor, size_t a_len, int n, double *inv_rowmajor, double *times10, int pivoting);
/* matrix_multiply of the reference (matrix_multiply.cpp:15): *errore = sqrt(N) - ||A * B||_F, N = sqrt(len), the product
 * accumulated in double on the fp64 matrix cores; MI32_BAD_SHAPE unless len is a perfect square */
int mi32_matrix_multiply_64(const double *a, const double *b, size_t len, double *errore);

/* ---- introspection -------------------------------------------------------- */
/* The two durations the reference prints per call ("Tempo Totale Impiegato",
 * "Tempo Computazione", mat_inv_32.cpp:385-386) for the last host-pointer call
 * on the default context: total (H2D + compute + D2H) and compute only. */
int mi32_last_timing(double *total_seconds, double *compute_seconds);
/* which algorithm a call of this shape would use after AUTO resolution */
int mi32_resolve_algo(mi32_handle_t h, int n, int batch);
/* widest sub-panel allowed and outer block width the blocked path would use for this shape */
int mi32_resolve_blocking(mi32_handle_t h, int n, int batch, int *panel_width, int *block_width);
/* The sub-panel width of every outer block (the panel kernel keeps rows x width floats in registers, so the
 * first blocks of a large matrix use narrower sub-panels): *nblocks receives the number of outer blocks,
 * widths[0 .. min(capacity, *nblocks)) their sub-panel widths. */
int mi32_resolve_panel_widths(mi32_handle_t h, int n, int batch, int *widths, int capacity, int *nblocks);
/* How a blocked fp32 call of this shape would run on this handle, answered without a device (h may be NULL: what a
 * fresh context does) from the settings, the environment and the shape -- the one description the library itself
 * enqueues the call from.  The widths of the sub-panels: mi32_resolve_panel_widths. */
typedef struct {
    int np, block_width, nblocks; /* padded order (multiple of 128), outer block width, number of outer blocks */
    int shared_panels;            /* 1: panels of more than 4096 rows are shared by several workgroups */
    int lookahead;                /* 1: all but the next block's columns of a rank-bw update run on the second stream */
    int parts;                    /* 1 or 2: a batch split in two halves runs them on two streams */
    int part_batch[2];            /* members per part (second 0 when parts == 1) */
    int part_strips_at_end[2];    /* 1: the block's strips in one launch at its end; 0: they ride in the panel launches */
    int first_fused_block;        /* blocks from this one on run panel and in-block update as one launch; nblocks when
                                   * no block is fused */
} mi32_route_t;
/* panel_groups[0 .. min(capacity, nblocks)) (may be NULL with capacity 0): workgroups per panel at the start of each
 * outer block.  MI32_BAD_SHAPE for n <= 0, batch <= 0, an order the blocked path does not take (more than 16384
 * padded rows) or a NULL route. */
int mi32_resolve_route(mi32_handle_t h, int n, int batch, mi32_route_t *route, int *panel_groups, int capacity);
/* The register-resident path (MI32_ALGO_RESIDENT), answered without a device (h may be NULL): *lanes_per_matrix =
 * lanes that hold one matrix of this order (8 / 16 / 32 / 64 for 1 <= n <= 64, 0 above: RESIDENT falls back
 * there), *max_order = the largest order it takes (64).  elem_bytes: 4 (fp32) or 8 (fp64); anything else, or
 * n <= 0, is MI32_BAD_SHAPE. */
int mi32_resolve_resident(mi32_handle_t h, int n, int elem_bytes, int *lanes_per_matrix, int *max_order);
/* The workgroup-resident path (MI32_ALGO_WORKGROUP), answered without a device (h may be NULL): *threads_per_matrix =
 * threads that hold one matrix of this order (256 for 65 <= n <= 128, 0 outside: WORKGROUP resolves to RESIDENT
 * below and to AUTO's choice above), *rows_per_thread = register rows per thread (40 / 48 / 56 / 64 for orders up to
 * 80 / 96 / 112 / 128, 0 outside), *max_order = the largest order it takes (128).  elem_bytes: 4 (fp32) or 8 (fp64);
 * anything else, or n <= 0, is MI32_BAD_SHAPE.  The output pointers are optional. */
int mi32_resolve_workgroup(mi32_handle_t h, int n, int elem_bytes, int *threads_per_matrix, int *rows_per_thread,
                           int *max_order);
/* The wide workgroup-resident path (MI32_ALGO_WIDE), answered without a device (h may be NULL): *threads_per_matrix =
 * threads that hold one matrix of this order (768 for 129 <= n <= 192, 1024 for 193 <= n <= 256 at elem_bytes 4; 0
 * outside and for every order at elem_bytes 8: WIDE resolves to RESIDENT / WORKGROUP below and to AUTO's choice above
 * and in fp64), *rows_per_thread = register rows per thread (40 / 48 / 56 / 64 for orders up to 160 / 192 / 224 / 256,
 * 0 where *threads_per_matrix is), *max_order = the largest order it takes (256).  elem_bytes: 4 (fp32) or 8 (fp64);
 * anything else, or n <= 0, is MI32_BAD_SHAPE.  The output pointers are optional. */
int mi32_resolve_wide(mi32_handle_t h, int n, int elem_bytes, int *threads_per_matrix, int *rows_per_thread,
                      int *max_order);
/* How mi32_solve_device* would run this shape, answered without a device (h may be NULL): *chunk_cols = the most columns
 * one launch takes (64 - n for n <= 32, 128 - n for 33 <= n <= 127), *launches = ceil(nrhs / *chunk_cols), and the
 * first chunk's kernel: *lanes = lanes per member (8 / 16 / 32 / 64) of the register-resident instance, 0 when the chunk
 * takes the workgroup-resident one; *rows_per_thread = that one's register rows per thread (40 / 48 / 56 / 64), 0 when
 * the chunk takes the register-resident instance.  n outside 1 ... 127, nrhs <= 0, elem_bytes other than 4 or 8, or a
 * NULL output is MI32_BAD_SHAPE. */
int mi32_resolve_solve(mi32_handle_t h, int n, int nrhs, int elem_bytes, int *chunk_cols, int *launches, int *lanes,
                       int *rows_per_thread);
/* name of the dominant device kernel of that algorithm (for rocprof filtering) */
const char *mi32_dominant_kernel(int algo);
/* thread-local description of the last MI32_RUNTIME_ERROR */
const char *mi32_last_error(void);
int mi32_version(void);

#ifdef __cplusplus
}
#endif
#endif
