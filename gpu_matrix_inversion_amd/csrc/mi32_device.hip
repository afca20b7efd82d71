// mi32_device.hip -- the device-pointer entry points of libmat_inv_32.so: what mi32_plan.hip decided, enqueued on the
// context's streams.
#include <climits>
#include <new>
#include <type_traits>
#include <vector>

#include "mi32_apply.h"
#include "mi32_context.h"
#include "mi32_csr_blocks.h"
#include "mi32_csr_find.h"
#include "mi32_det_large.h"
#include "mi32_relax.h"
#include "mi32_stored.h"

using namespace mi32;

// A uniform batch on the one-launch paths: the register-resident kernels up to kResidentMaxOrder rows, the
// workgroup-resident ones up to kWorkgroupMaxOrder, the wide ones (fp32 only) above (that the order has an instance is
// the caller's business: above kWorkgroupMaxOrder only a DenseRoute::WIDE call comes here).  det: where the
// determinants go, empty for none; d_inv may be null only with one.  The caller holds h->mu and has set the device.
template <typename T>
static int one_launch_device(mi32_context *h, bool pivoting, const T *d_a, int n, int batch, T *d_inv, int *d_status,
                             const DetOut det)
{
    MI32_TRY(zeroed_status_buffer(h, d_status, batch, &d_status));
    hipError_t e = hipErrorInvalidValue;  // (an fp64 order above kWorkgroupMaxOrder: no instance)
    if (n <= kResidentMaxOrder) e = resident_invert(d_a, d_inv, n, batch, d_status, det, h->stream, h->prof, pivoting);
    else if (n <= kWorkgroupMaxOrder) e = workgroup_invert(d_a, d_inv, n, batch, d_status, det, h->stream, h->prof, pivoting);
    else if constexpr (std::is_same<T, float>::value) e = wide_invert(d_a, d_inv, n, batch, d_status, det, h->stream, h->prof, pivoting);
    return hip_status(e, "kernel launch");
}

// the resources a blocked fp32 inversion of order n is enqueued with on this context
static BlockedExec blocked_exec(mi32_context *h, int n)
{
    BlockedExec ex;
    ex.stream = h->stream;
    ex.aux = h->aux_stream;
    ex.events = h->la_events;
    ex.n_events = h->aux_stream ? 8 : 0;
    lookahead_geometry(h->cu_count, n, &ex.aux_workgroups, &ex.aux_exclusive);
    ex.prof = h->prof;
    return ex;
}

// The two parts of a split batch, the second on the context's split stream; the workspace holds one part per half
// (DenseRoute::ws_bytes).
static int blocked_invert_split(mi32_context *h, const BlockedRoute &r, const BlockedExec &ex, const float *d_a, float *d_inv,
                                int *d_status, const DetRec &det = DetRec())
{
    const int b0 = r.part_batch[0];
    const size_t mat = (size_t)r.n * r.n;
    char *ws1 = (char *)h->ws.ptr + blocked_workspace_bytes(r, b0);
    // the second stream joins here and is joined again at the end (events 0 and 1 are free: the
    // look-ahead, their other user, only runs for single matrices)
    MI32_HIP(hipEventRecord(h->la_events[0], h->stream));
    MI32_HIP(hipStreamWaitEvent(h->split_stream, h->la_events[0], 0));
    BlockedExec ex1 = ex;
    ex1.stream = h->split_stream;
    // a det call: the second part's pivots and parities follow the first part's; its inverse may be absent
    DetRec det1 = det;
    if (det.on()) {
        det1.piv = (float *)det.piv + (size_t)b0 * det.pstride;
        det1.parity = det.parity + b0;
    }
    float *inv1 = d_inv ? d_inv + (size_t)b0 * mat : nullptr;
    hipError_t e = blocked_invert(r, 0, d_a, d_inv, d_status, h->ws.ptr, ex, det);
    if (e == hipSuccess) e = blocked_invert(r, 1, d_a + (size_t)b0 * mat, inv1, d_status + b0, ws1, ex1, det1);
    MI32_HIP(hipEventRecord(h->la_events[1], h->split_stream));
    MI32_HIP(hipStreamWaitEvent(h->stream, h->la_events[1], 0));
    return hip_status(e, "kernel launch");
}

// ---- the determinant above kWorkgroupMaxOrder: the route records its pivots, a finish kernel multiplies them ---------
// The context's det memory for this call (grown on demand, never part of the workspace), its flag and parity words
// zeroed and the input scanned on the main stream.  Two det calls back to back are ordered by that stream: the finish
// kernel of the first is enqueued there before the memset of the second.
template <typename T>
static int det_begin(mi32_context *h, const T *d_a, int n, int np, int batch, DetMem *dm, DetRec *rec)
{
    MI32_TRY(h->det.ensure(h, det_bytes(np, batch, sizeof(T))));
    *dm = det_carve(h->det.ptr, np, batch, sizeof(T));
    // the flag and the parity words: one memset while the two regions lie side by side, one each with the guard mode's
    // red zone between them
    if ((char *)dm->parity == (char *)dm->flag + dm->wbytes) {
        MI32_HIP(hipMemsetAsync(dm->flag, 0, 2 * dm->wbytes, h->stream));
    } else {
        MI32_HIP(hipMemsetAsync(dm->flag, 0, dm->wbytes, h->stream));
        MI32_HIP(hipMemsetAsync(dm->parity, 0, dm->wbytes, h->stream));
    }
    ProfScope ps(h->prof, KC_FINISH, h->stream);
    launch_det_scan(d_a, n, batch, dm->flag, h->stream);
    *rec = DetRec{dm->piv, dm->pstride, dm->parity};
    return MI32_OK;
}
// enqueued last on the main stream: the recurrence over the steps first ... first + n - 1 of every list
template <typename T>
static int det_end(mi32_context *h, const DetMem &dm, int first, int n, int batch, const int *d_status, bool pivoting,
                   const DetOut out)
{
    ProfScope ps(h->prof, KC_FINISH, h->stream);
    launch_det_finish((const T *)dm.piv, dm.pstride, first, n, dm.parity, dm.flag, d_status, pivoting, out, batch, h->stream);
    return hip_status(hipGetLastError(), "kernel launch");
}

// THE dense call: status memset (by the route, or here on the one-launch paths), det memset and input scan, the route,
// the det finish kernel.
template <typename T>
int inv_device(mi32_context *h, Settings s, const T *d_a, int n, int batch, T *d_inv, int *d_status, const DetOut det)
{
    constexpr bool f32 = std::is_same<T, float>::value;
    MI32_HIP(hipSetDevice(h->device));
    const DenseRoute dr = dense_route(h, s, n, batch, sizeof(T));
    MI32_TRY(h->ws.ensure(h, dr.ws_bytes));
    if (g_ws_guard.load(std::memory_order_relaxed) != 0 || !h->zones.empty()) {
        // the diagnostic guard mode: poison and red zones for every carve of this call, before its first launch (a
        // one-launch call carves nothing: it only forgets the zones of the call before)
        if (!det.empty() && !dr.one_launch()) MI32_TRY(h->det.ensure(h, det_bytes(dr.det_steps, batch, sizeof(T))));
        MI32_TRY(guard_arm(h, dense_carves(dr, batch, sizeof(T), !det.empty())));
    }
    if (dr.one_launch()) return one_launch_device(h, s.pivoting, d_a, n, batch, d_inv, d_status, det);
    MI32_TRY(status_buffer(h, d_status, batch, &d_status));
    DetMem dm;
    DetRec rec;  // empty: a plain call
    if (!det.empty()) MI32_TRY(det_begin(h, d_a, n, dr.det_steps, batch, &dm, &rec));
    int rc = MI32_OK;
    switch (dr.path) {
        case DenseRoute::SWEEP:
            rc = hip_status(sweep_invert(dr.sweep, d_a, d_inv, batch, d_status, h->ws.ptr, h->stream, h->prof, s.pivoting, rec),
                            "kernel launch");
            break;
        case DenseRoute::BLOCKED32:
            if constexpr (f32) {
                const BlockedExec ex = blocked_exec(h, n);
                rc = dr.blocked.parts == 2
                         ? blocked_invert_split(h, dr.blocked, ex, d_a, d_inv, d_status, rec)
                         : hip_status(blocked_invert(dr.blocked, 0, d_a, d_inv, d_status, h->ws.ptr, ex, rec), "kernel launch");
            }
            break;
        case DenseRoute::BLOCKED64:
            if constexpr (!f32)
                rc = hip_status(blocked64_invert(dr.blocked64, d_a, d_inv, batch, d_status, h->ws.ptr, h->stream, h->prof, rec),
                                "kernel launch");
            break;
        case DenseRoute::NOPIVOT64:
            if constexpr (!f32)
                rc = hip_status(nopivot64_invert(dr.nopivot64, d_a, d_inv, batch, d_status, h->ws.ptr, h->stream, h->prof, rec),
                                "kernel launch");
            break;
        case DenseRoute::RESIDENT:
        case DenseRoute::WORKGROUP:
        case DenseRoute::WIDE: break;  // (returned above)
    }
    if (rc != MI32_OK || det.empty()) return rc;
    return det_end<T>(h, dm, dr.det_first, n, batch, d_status, s.pivoting, det);
}
template int inv_device(mi32_context *, Settings, const float *, int, int, float *, int *, DetOut);
template int inv_device(mi32_context *, Settings, const double *, int, int, double *, int *, DetOut);

// the arguments are checked before the context is touched
template <typename T>
static int inv_device_checked(mi32_context *h, const T *d_a, int n, int batch, T *d_inv, int *d_status)
{
    if (!h || !d_a || !d_inv || n <= 0 || batch <= 0 || d_a == d_inv) return MI32_BAD_SHAPE;
    std::lock_guard<std::mutex> lk(h->mu);
    return inv_device(h, h->set, d_a, n, batch, d_inv, d_status);
}

// The inverse with the determinant (see the header); the arguments are checked before the context is touched.  Up to
// kWorkgroupMaxOrder the one-launch kernels run, whatever the context's algorithm, and no workspace is ensured;
// max_order bounds mi32_inv_det_device*, and above kWorkgroupMaxOrder mi32_inv_det_any_device* runs the route
// mi32_inv_device* runs on this context (the wide one-launch path's det twin included).
template <typename T>
static int inv_det_device(mi32_context *h, int max_order, const T *d_a, int n, int batch, T *d_inv, int *d_status,
                          double *d_det_mant, int *d_det_exp)
{
    if (!h || !d_a || n <= 0 || n > max_order || batch <= 0 || d_a == d_inv || !d_det_mant || !d_det_exp)
        return MI32_BAD_SHAPE;
    std::lock_guard<std::mutex> lk(h->mu);
    const DetOut out{d_det_mant, d_det_exp};
    if (n > kWorkgroupMaxOrder) return inv_device(h, h->set, d_a, n, batch, d_inv, d_status, out);
    MI32_HIP(hipSetDevice(h->device));
    return one_launch_device(h, h->set.pivoting, d_a, n, batch, d_inv, d_status, out);
}

// A X = B on the one-launch paths: one launch per chunk of columns (solve_walk); every launch repeats the elimination
// of A, and the status words are zeroed once: a launch only ever raises a member's flag.
template <typename T>
static int solve_device(mi32_context *h, const T *d_a, int n, int batch, const T *d_b, int nrhs, T *d_x, int *d_status)
{
    if (!h || !d_a || !d_b || !d_x || solve_chunk_cols(n) == 0 || batch <= 0 || nrhs <= 0 || d_x == d_a) return MI32_BAD_SHAPE;
    std::lock_guard<std::mutex> lk(h->mu);
    MI32_HIP(hipSetDevice(h->device));
    MI32_TRY(zeroed_status_buffer(h, d_status, batch, &d_status));
    hipError_t e = hipSuccess;
    solve_walk(n, batch, nrhs, [&](const SolveLaunch &l) {
        const SolveArgs<T> s{d_a, d_b, d_x, d_status, n, batch, nrhs, l.col0, l.cols};
        e = l.kernel.lanes ? resident_solve(s, h->stream, h->prof, h->set.pivoting)
                           : workgroup_solve(s, h->stream, h->prof, h->set.pivoting);
        return e == hipSuccess;
    });
    return hip_status(e, "kernel launch");
}

// DET: the det kernels, d_inv may be null
template <typename T, bool DET>
static int inv_device_vbatched(mi32_context *h, const mi32_vbatch *p, const T *const *d_a, const int *d_lda,
                               T *const *d_inv, const int *d_ldinv, int *d_status, double *d_det_mant = nullptr,
                               int *d_det_exp = nullptr)
{
    if (!h || !p || !d_a || (!DET && !d_inv) || (DET && (!d_det_mant || !d_det_exp))) return MI32_BAD_SHAPE;
    if (p->device != h->device) return MI32_BAD_SHAPE;
    std::lock_guard<std::mutex> lk(h->mu);
    MI32_HIP(hipSetDevice(h->device));
    MI32_TRY(zeroed_status_buffer(h, d_status, p->batch, &d_status));
    const VbatchArgs<T> v{p->d_orders, p->d_members, d_a, d_inv, d_lda, d_ldinv, d_status};
    const DetOut det = DET ? DetOut{d_det_mant, d_det_exp} : DetOut{nullptr, nullptr};
    for (int k = 0; k < kVbatchClasses; ++k) {
        const int first = p->class_begin[k], count = p->class_begin[k + 1] - first;
        if (count == 0) continue;  // a class without members is not launched
        const KernelInstance &c = kVbatchClass[k];
        MI32_TRY(hip_status(
            c.lanes ? resident_vinvert(c.lanes, v, det, first, count, h->stream, h->prof, h->set.pivoting)
                    : workgroup_vinvert(c.rows_per_thread, v, det, first, count, h->stream, h->prof, h->set.pivoting),
            "kernel launch"));
    }
    return MI32_OK;
}

// A X = B for a variable-size batch: the launches of vsolve_walk.  The arguments are checked before the context is
// touched.
template <typename T>
static int solve_device_vbatched(mi32_context *h, const mi32_vbatch *p, const T *const *d_a, const int *d_lda,
                                 const T *const *d_b, const int *d_ldb, int nrhs, T *const *d_x, const int *d_ldx,
                                 int *d_status)
{
    if (!h || !p || !d_a || !d_b || !d_x || nrhs <= 0) return MI32_BAD_SHAPE;
    if (p->device != h->device || !vsolve_has_columns(p->order_begin)) return MI32_BAD_SHAPE;
    std::lock_guard<std::mutex> lk(h->mu);
    MI32_HIP(hipSetDevice(h->device));
    // zeroed once: a launch only ever raises a member's flag
    MI32_TRY(zeroed_status_buffer(h, d_status, p->batch, &d_status));
    hipError_t e = hipSuccess;
    vsolve_walk(p->order_begin, nrhs, [&](const SolveLaunch &l) {
        const VsolveArgs<T> v{p->d_orders, p->d_members, d_a, d_b, d_x, d_lda, d_ldb, d_ldx, d_status, nrhs, l.col0, l.cols};
        e = l.kernel.lanes
                ? resident_vsolve(l.kernel.lanes, v, l.first, l.count, h->stream, h->prof, h->set.pivoting)
                : workgroup_vsolve(l.kernel.rows_per_thread, v, l.first, l.count, h->stream, h->prof, h->set.pivoting);
        return e == hipSuccess;
    });
    return hip_status(e, "kernel launch");
}

// The calls that walk a plan's members with the apply call's launch list (apply_walk: one launch per lane class that has
// members): the product, the CSR gather, the statistics, store and apply of block inverses in a per-member storage
// format (mi32_stored.h), and the block residual and relaxation sweep on them (mi32_relax.h).  No workspace, no memset, no status: a product or a copy cannot fail.  Each caller checks its
// own arguments before the context is touched; a plan of another device is refused here, before the lock.
template <typename T, typename Launch>
static int member_walk(mi32_context *h, const mi32_vbatch *p, const Launch &launch)
{
    if (p->device != h->device) return MI32_BAD_SHAPE;
    std::lock_guard<std::mutex> lk(h->mu);
    MI32_HIP(hipSetDevice(h->device));
    hipError_t e = hipSuccess;
    apply_walk(p->class_begin, sizeof(T), [&](const ApplyLaunch &l) {
        e = launch(l);
        return e == hipSuccess;
    });
    return hip_status(e, "kernel launch");
}

template <typename T>
static int apply_device_vbatched(mi32_context *h, const mi32_vbatch *p, const T *const *d_x, const int *d_ldx,
                                 const T *const *d_r, const int *d_ldr, int nrhs, T *const *d_z, const int *d_ldz)
{
    if (!h || !p || !d_x || !d_r || !d_z || nrhs <= 0) return MI32_BAD_SHAPE;
    return member_walk<T>(h, p, [&](const ApplyLaunch &l) {
        const ApplyArgs<T> a{p->d_orders, p->d_members, d_x, d_r, d_z, d_ldx, d_ldr, d_ldz, nrhs};
        return apply_vlaunch(l.lanes, a, l.first, l.count, h->stream, h->prof);
    });
}

template <typename T>
static int csr_blocks_device(mi32_context *h, const mi32_vbatch *p, const void *d_row_ptr, const void *d_col,
                             int index_bytes, const T *d_val, const long long *d_first, T *const *d_out,
                             const int *d_ldout)
{
    if (!h || !p || !d_row_ptr || !d_col || !d_val || !d_first || !d_out) return MI32_BAD_SHAPE;
    if (index_bytes != 4 && index_bytes != 8) return MI32_BAD_SHAPE;
    return member_walk<T>(h, p, [&](const ApplyLaunch &l) {
        const CsrBlocksArgs<T> a{p->d_orders, p->d_members, d_row_ptr, d_col, d_val, d_first, d_out, d_ldout, index_bytes};
        return csr_blocks_vlaunch(l.lanes, a, l.first, l.count, h->stream, h->prof);
    });
}

// The blocks of a CSR pattern (mi32_csr_find.h): the caller's temporary memory, no plan.  stages: FIND_ALL but for the
// measuring hook.
static int csr_find_blocks_device(mi32_context *h, long long n, const void *d_row_ptr, const void *d_col, int index_bytes,
                                  int max_order, int agglomerate, unsigned char *d_start, void *d_work, size_t work_bytes,
                                  int stages)
{
    if (!h || !d_row_ptr || !d_col || !d_start || !d_work || n < 1) return MI32_BAD_SHAPE;
    if (index_bytes != 4 && index_bytes != 8) return MI32_BAD_SHAPE;
    if (max_order < 1 || max_order > kFindMaxOrder) return MI32_BAD_SHAPE;
    if (work_bytes < find_layout(n).bytes || (reinterpret_cast<uintptr_t>(d_work) & 15) != 0) return MI32_BAD_SHAPE;
    std::lock_guard<std::mutex> lk(h->mu);
    MI32_HIP(hipSetDevice(h->device));
    const FindArgs a{n, d_row_ptr, d_col, index_bytes, max_order, agglomerate != 0, d_start, d_work};
    return hip_status(csr_find_launch(a, stages, h->stream, h->prof), "kernel launch");
}

template <typename T>
static int block_stats_device(mi32_context *h, const mi32_vbatch *p, const T *const *d_a, const int *d_lda, double *d_stats)
{
    if (!h || !p || !d_a || !d_stats) return MI32_BAD_SHAPE;
    return member_walk<T>(h, p, [&](const ApplyLaunch &l) {
        const BlockStatsArgs<T> a{p->d_orders, p->d_members, d_a, d_lda, d_stats};
        return block_stats_vlaunch(l.lanes, a, l.first, l.count, h->stream, h->prof);
    });
}

template <typename T>
static int store_inverses_device(mi32_context *h, const mi32_vbatch *p, const T *const *d_x, const int *d_ldx,
                                 const int *d_format, const long long *d_offset, void *d_store)
{
    if (!h || !p || !d_x || !d_format || !d_offset || !d_store) return MI32_BAD_SHAPE;
    return member_walk<T>(h, p, [&](const ApplyLaunch &l) {
        const StoreArgs<T> a{p->d_orders, p->d_members, d_x, d_ldx, d_format, d_offset, static_cast<unsigned char *>(d_store)};
        return store_vlaunch(l.lanes, a, l.first, l.count, h->stream, h->prof);
    });
}

template <typename T>
static int apply_stored_device(mi32_context *h, const mi32_vbatch *p, const void *d_store, const long long *d_offset,
                               const int *d_format, const T *const *d_r, const int *d_ldr, int nrhs, T *const *d_z,
                               const int *d_ldz)
{
    if (!h || !p || !d_store || !d_offset || !d_format || !d_r || !d_z || nrhs <= 0) return MI32_BAD_SHAPE;
    return member_walk<T>(h, p, [&](const ApplyLaunch &l) {
        const StoredApplyArgs<T> a{p->d_orders, p->d_members, static_cast<const unsigned char *>(d_store), d_offset, d_format,
                                   d_r, d_z, d_ldr, d_ldz, nrhs};
        return apply_stored_vlaunch(l.lanes, a, l.first, l.count, h->stream, h->prof);
    });
}

// The residual of the block rows (d_r set) or the fused sweep (d_xnew set) of mi32_relax.h.
template <typename T>
static int relax_device(mi32_context *h, const mi32_vbatch *p, const void *d_row_ptr, const void *d_col, int index_bytes,
                        const T *d_val, const long long *d_first, const void *d_store, const long long *d_offset,
                        const int *d_format, const T *d_x, const T *d_b, T omega, T *d_xnew, T *const *d_r)
{
    if (!h || !p || !d_row_ptr || !d_col || !d_val || !d_first || !d_x || !d_b) return MI32_BAD_SHAPE;
    if (d_xnew ? (!d_store || !d_offset || !d_format || d_r) : !d_r) return MI32_BAD_SHAPE;
    if (index_bytes != 4 && index_bytes != 8) return MI32_BAD_SHAPE;
    return member_walk<T>(h, p, [&](const ApplyLaunch &l) {
        const RelaxArgs<T> a{p->d_orders, p->d_members, d_row_ptr, d_col, d_val, d_first,
                             static_cast<const unsigned char *>(d_store), d_offset, d_format, d_x, d_b, d_xnew, d_r, omega,
                             index_bytes};
        return relax_vlaunch(l.lanes, a, l.first, l.count, h->stream, h->prof);
    });
}

extern "C" {

int mi32_inv_device(mi32_handle_t h, const float *d_a, int n, int batch, float *d_inv, int *d_status)
{
    return inv_device_checked(h, d_a, n, batch, d_inv, d_status);
}

int mi32_inv_device_f64(mi32_handle_t h, const double *d_a, int n, int batch, double *d_inv, int *d_status)
{
    return inv_device_checked(h, d_a, n, batch, d_inv, d_status);
}

int mi32_inv_det_device(mi32_handle_t h, const float *d_a, int n, int batch, float *d_inv, int *d_status,
                        double *d_det_mant, int *d_det_exp)
{
    return inv_det_device(h, kWorkgroupMaxOrder, d_a, n, batch, d_inv, d_status, d_det_mant, d_det_exp);
}

int mi32_inv_det_device_f64(mi32_handle_t h, const double *d_a, int n, int batch, double *d_inv, int *d_status,
                            double *d_det_mant, int *d_det_exp)
{
    return inv_det_device(h, kWorkgroupMaxOrder, d_a, n, batch, d_inv, d_status, d_det_mant, d_det_exp);
}

int mi32_inv_det_any_device(mi32_handle_t h, const float *d_a, int n, int batch, float *d_inv, int *d_status,
                            double *d_det_mant, int *d_det_exp)
{
    return inv_det_device(h, INT_MAX, d_a, n, batch, d_inv, d_status, d_det_mant, d_det_exp);
}

int mi32_inv_det_any_device_f64(mi32_handle_t h, const double *d_a, int n, int batch, double *d_inv, int *d_status,
                                double *d_det_mant, int *d_det_exp)
{
    return inv_det_device(h, INT_MAX, d_a, n, batch, d_inv, d_status, d_det_mant, d_det_exp);
}

int mi32_solve_device(mi32_handle_t h, const float *d_a, int n, int batch, const float *d_b, int nrhs, float *d_x,
                      int *d_status)
{
    return solve_device(h, d_a, n, batch, d_b, nrhs, d_x, d_status);
}

int mi32_solve_device_f64(mi32_handle_t h, const double *d_a, int n, int batch, const double *d_b, int nrhs, double *d_x,
                          int *d_status)
{
    return solve_device(h, d_a, n, batch, d_b, nrhs, d_x, d_status);
}

int mi32_vbatch_create(mi32_handle_t h, const int *orders, int batch, mi32_vbatch_t *out)
{
    if (!out) return MI32_BAD_SHAPE;
    *out = nullptr;
    if (!h || !orders || batch <= 0) return MI32_BAD_SHAPE;
    std::vector<int> perm((size_t)batch);
    mi32_vbatch *p = new (std::nothrow) mi32_vbatch();
    if (!p) return MI32_RUNTIME_ERROR;
    const int rc = vbatch_sort(orders, batch, perm.data(), p->class_begin, p->order_begin);
    if (rc != MI32_OK) {
        delete p;
        return rc;
    }
    p->device = h->device;
    p->batch = batch;
    const size_t bytes = (size_t)batch * sizeof(int);
    hipError_t e = hipSetDevice(h->device);
    if (e == hipSuccess) e = hipMalloc((void **)&p->d_orders, bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&p->d_members, bytes);
    // synchronous copies from pageable memory: the host arrays may go away when this returns
    if (e == hipSuccess) e = hipMemcpy(p->d_orders, orders, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p->d_members, perm.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)mi32_vbatch_destroy(p);
        return hip_status(e, "mi32_vbatch_create");
    }
    *out = p;
    return MI32_OK;
}

int mi32_vbatch_destroy(mi32_vbatch_t p)
{
    if (!p) return MI32_OK;
    (void)hipSetDevice(p->device);
    // hipFree synchronises with the device: calls that still read the plan finish first
    if (p->d_orders) (void)hipFree(p->d_orders);
    if (p->d_members) (void)hipFree(p->d_members);
    delete p;
    return MI32_OK;
}

int mi32_vbatch_info(mi32_vbatch_t p, int *batch, int *class_begin)
{
    if (!p) return MI32_BAD_SHAPE;
    if (batch) *batch = p->batch;
    if (class_begin)
        for (int k = 0; k <= kVbatchClasses; ++k) class_begin[k] = p->class_begin[k];
    return MI32_OK;
}

int mi32_inv_device_vbatched(mi32_handle_t h, mi32_vbatch_t p, const float *const *d_a, const int *d_lda,
                             float *const *d_inv, const int *d_ldinv, int *d_status)
{
    return inv_device_vbatched<float, false>(h, p, d_a, d_lda, d_inv, d_ldinv, d_status);
}

int mi32_inv_device_vbatched_f64(mi32_handle_t h, mi32_vbatch_t p, const double *const *d_a, const int *d_lda,
                                 double *const *d_inv, const int *d_ldinv, int *d_status)
{
    return inv_device_vbatched<double, false>(h, p, d_a, d_lda, d_inv, d_ldinv, d_status);
}

int mi32_inv_det_device_vbatched(mi32_handle_t h, mi32_vbatch_t p, const float *const *d_a, const int *d_lda,
                                 float *const *d_inv, const int *d_ldinv, int *d_status, double *d_det_mant,
                                 int *d_det_exp)
{
    return inv_device_vbatched<float, true>(h, p, d_a, d_lda, d_inv, d_ldinv, d_status, d_det_mant, d_det_exp);
}

int mi32_inv_det_device_vbatched_f64(mi32_handle_t h, mi32_vbatch_t p, const double *const *d_a, const int *d_lda,
                                     double *const *d_inv, const int *d_ldinv, int *d_status, double *d_det_mant,
                                     int *d_det_exp)
{
    return inv_device_vbatched<double, true>(h, p, d_a, d_lda, d_inv, d_ldinv, d_status, d_det_mant, d_det_exp);
}

int mi32_solve_device_vbatched(mi32_handle_t h, mi32_vbatch_t p, const float *const *d_a, const int *d_lda,
                               const float *const *d_b, const int *d_ldb, int nrhs, float *const *d_x, const int *d_ldx,
                               int *d_status)
{
    return solve_device_vbatched(h, p, d_a, d_lda, d_b, d_ldb, nrhs, d_x, d_ldx, d_status);
}

int mi32_solve_device_vbatched_f64(mi32_handle_t h, mi32_vbatch_t p, const double *const *d_a, const int *d_lda,
                                   const double *const *d_b, const int *d_ldb, int nrhs, double *const *d_x,
                                   const int *d_ldx, int *d_status)
{
    return solve_device_vbatched(h, p, d_a, d_lda, d_b, d_ldb, nrhs, d_x, d_ldx, d_status);
}

int mi32_apply_device_vbatched(mi32_handle_t h, mi32_vbatch_t p, const float *const *d_x, const int *d_ldx,
                               const float *const *d_r, const int *d_ldr, int nrhs, float *const *d_z, const int *d_ldz)
{
    return apply_device_vbatched(h, p, d_x, d_ldx, d_r, d_ldr, nrhs, d_z, d_ldz);
}

int mi32_apply_device_vbatched_f64(mi32_handle_t h, mi32_vbatch_t p, const double *const *d_x, const int *d_ldx,
                                   const double *const *d_r, const int *d_ldr, int nrhs, double *const *d_z,
                                   const int *d_ldz)
{
    return apply_device_vbatched(h, p, d_x, d_ldx, d_r, d_ldr, nrhs, d_z, d_ldz);
}

int mi32_csr_blocks_device(mi32_handle_t h, mi32_vbatch_t p, const void *d_row_ptr, const void *d_col, int index_bytes,
                           const float *d_val, const long long *d_first, float *const *d_out, const int *d_ldout)
{
    return csr_blocks_device(h, p, d_row_ptr, d_col, index_bytes, d_val, d_first, d_out, d_ldout);
}

int mi32_csr_blocks_device_f64(mi32_handle_t h, mi32_vbatch_t p, const void *d_row_ptr, const void *d_col,
                               int index_bytes, const double *d_val, const long long *d_first, double *const *d_out,
                               const int *d_ldout)
{
    return csr_blocks_device(h, p, d_row_ptr, d_col, index_bytes, d_val, d_first, d_out, d_ldout);
}

int mi32_csr_find_blocks_work_bytes(long long n, size_t *bytes)
{
    if (n < 1 || !bytes) return MI32_BAD_SHAPE;
    *bytes = find_layout(n).bytes;
    return MI32_OK;
}

int mi32_csr_find_blocks_chunk_rows(void) { return kFindChunk; }

int mi32_csr_find_blocks_device(mi32_handle_t h, long long n, const void *d_row_ptr, const void *d_col, int index_bytes,
                                int max_order, int agglomerate, unsigned char *d_start, void *d_work, size_t work_bytes)
{
    return csr_find_blocks_device(h, n, d_row_ptr, d_col, index_bytes, max_order, agglomerate, d_start, d_work, work_bytes,
                                  FIND_ALL);
}

// Not part of include/mat_inv_32_csr_find.h: the stages of `stages` (1 nat, 2 runs, 4 sv, 8 chain, 16 mark) alone, on the
// temporary memory a whole call left, for tools/csr_find_blocks_bench.py to time them one by one.
int mi32_debug_csr_find_stages(mi32_handle_t h, long long n, const void *d_row_ptr, const void *d_col, int index_bytes,
                               int max_order, int agglomerate, unsigned char *d_start, void *d_work, size_t work_bytes,
                               int stages)
{
    return csr_find_blocks_device(h, n, d_row_ptr, d_col, index_bytes, max_order, agglomerate, d_start, d_work, work_bytes,
                                  stages & FIND_ALL);
}

int mi32_block_stats_device(mi32_handle_t h, mi32_vbatch_t p, const float *const *d_a, const int *d_lda, double *d_stats)
{
    return block_stats_device(h, p, d_a, d_lda, d_stats);
}

int mi32_block_stats_device_f64(mi32_handle_t h, mi32_vbatch_t p, const double *const *d_a, const int *d_lda,
                                double *d_stats)
{
    return block_stats_device(h, p, d_a, d_lda, d_stats);
}

int mi32_store_inverses_device(mi32_handle_t h, mi32_vbatch_t p, const float *const *d_x, const int *d_ldx,
                               const int *d_format, const long long *d_offset, void *d_store)
{
    return store_inverses_device(h, p, d_x, d_ldx, d_format, d_offset, d_store);
}

int mi32_store_inverses_device_f64(mi32_handle_t h, mi32_vbatch_t p, const double *const *d_x, const int *d_ldx,
                                   const int *d_format, const long long *d_offset, void *d_store)
{
    return store_inverses_device(h, p, d_x, d_ldx, d_format, d_offset, d_store);
}

int mi32_apply_stored_device(mi32_handle_t h, mi32_vbatch_t p, const void *d_store, const long long *d_offset,
                             const int *d_format, const float *const *d_r, const int *d_ldr, int nrhs,
                             float *const *d_z, const int *d_ldz)
{
    return apply_stored_device(h, p, d_store, d_offset, d_format, d_r, d_ldr, nrhs, d_z, d_ldz);
}

int mi32_apply_stored_device_f64(mi32_handle_t h, mi32_vbatch_t p, const void *d_store, const long long *d_offset,
                                 const int *d_format, const double *const *d_r, const int *d_ldr, int nrhs,
                                 double *const *d_z, const int *d_ldz)
{
    return apply_stored_device(h, p, d_store, d_offset, d_format, d_r, d_ldr, nrhs, d_z, d_ldz);
}

int mi32_csr_block_residual_device(mi32_handle_t h, mi32_vbatch_t p, const void *d_row_ptr, const void *d_col,
                                   int index_bytes, const float *d_val, const long long *d_first, const float *d_x,
                                   const float *d_b, float *const *d_r)
{
    return relax_device<float>(h, p, d_row_ptr, d_col, index_bytes, d_val, d_first, nullptr, nullptr, nullptr, d_x, d_b, 0.0f,
                               nullptr, d_r);
}

int mi32_csr_block_residual_device_f64(mi32_handle_t h, mi32_vbatch_t p, const void *d_row_ptr, const void *d_col,
                                       int index_bytes, const double *d_val, const long long *d_first, const double *d_x,
                                       const double *d_b, double *const *d_r)
{
    return relax_device<double>(h, p, d_row_ptr, d_col, index_bytes, d_val, d_first, nullptr, nullptr, nullptr, d_x, d_b, 0.0,
                                nullptr, d_r);
}

int mi32_csr_relax_stored_device(mi32_handle_t h, mi32_vbatch_t p, const void *d_row_ptr, const void *d_col,
                                 int index_bytes, const float *d_val, const long long *d_first, const void *d_store,
                                 const long long *d_offset, const int *d_format, const float *d_x, const float *d_b,
                                 float omega, float *d_xnew)
{
    if (!d_xnew) return MI32_BAD_SHAPE;
    return relax_device<float>(h, p, d_row_ptr, d_col, index_bytes, d_val, d_first, d_store, d_offset, d_format, d_x, d_b,
                               omega, d_xnew, nullptr);
}

int mi32_csr_relax_stored_device_f64(mi32_handle_t h, mi32_vbatch_t p, const void *d_row_ptr, const void *d_col,
                                     int index_bytes, const double *d_val, const long long *d_first, const void *d_store,
                                     const long long *d_offset, const int *d_format, const double *d_x, const double *d_b,
                                     double omega, double *d_xnew)
{
    if (!d_xnew) return MI32_BAD_SHAPE;
    return relax_device<double>(h, p, d_row_ptr, d_col, index_bytes, d_val, d_first, d_store, d_offset, d_format, d_x, d_b,
                                omega, d_xnew, nullptr);
}

int mi32_residual_device(mi32_handle_t h, const float *d_a, const float *d_x, int n, int batch, double *d_out)
{
    if (!h || !d_a || !d_x || !d_out || n <= 0 || batch <= 0) return MI32_BAD_SHAPE;
    std::lock_guard<std::mutex> lk(h->mu);
    MI32_HIP(hipSetDevice(h->device));
    MI32_TRY(h->ws.ensure(h, dense_route(h, h->set, n, batch, sizeof(float)).ws_bytes));
    if (g_ws_guard.load(std::memory_order_relaxed) != 0 || !h->zones.empty())  // the diagnostic guard mode
        MI32_TRY(guard_arm(h, {residual_carve_of(n, batch)}));
    return hip_status(residual_launch(d_a, d_x, n, batch, d_out, h->ws.ptr, h->stream), "residual launch");
}

}  // extern "C"
