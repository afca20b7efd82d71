// mi32_relax.hip -- one block-Jacobi relaxation sweep  x' = x + omega blockdiag(A)^-1 (b - A x)  from the CSR matrix and
// the stored block inverses, one launch per lane class that has members (apply_walk, at most five), and the residual of
// the block rows as a call of its own (mi32_relax.h).  No workspace, no memset, no atomics, no status.
//
// A group of L lanes (the workgroup of the 128 class) owns one member, as in mi32_stored.hip, and runs three stages:
//
// RESIDUAL.  The group splits into L / 8 SUB-GROUPS of 8 lanes, one block row each, ceil(n / (L / 8)) rounds.  Lane s of
// a sub-group takes the entries s, s + 8, ... of its row in stored order: its chain of fused multiply-adds IS the
// partial sum p_s of the definition (mat_inv_32_relax.h), whatever the row's length.  The butterfly over the 8 lanes
// (xor 4, 2, 1: additions of the same two operands in both lanes, so all eight hold the same bits) gives the row's sum,
// and lane 0 of the sub-group writes r = b - sum into the group's R region in LDS, where the product expects it -- or,
// in the residual-only instances, to the member's r in global memory.  Nothing of this depends on L.
//
// LOADS IN FLIGHT.  A row is a chain of dependent latencies: its range from row_ptr, then col and val, then the gather
// x[col].  So (1) the range and b of the NEXT round's row are loaded before this round's entries; (2) a lane loads the
// col / val of kInFlight of its entries, then gathers their x, before the first fma consumes one; (3) the first tile of
// the stored inverse and the old x of the lane's row are loaded before the residual stage and wait in registers.  Only
// the order of the fmas is fixed, not that of the loads.  Rows of different lengths share a wave: the entry loop is
// divergent, the round loop runs to the wave's largest order and the butterfly sits outside both.
//
// PRODUCT AND STORE.  The product is the loop of apply_chunk<T, L, 1, StoredLoader<T>> (mi32_member_walk.h), WRITTEN A
// SECOND TIME here with R staged by the residual stage (MINUS zero past the member's order) on the loader of
// mi32_stored_loader.h: cutting apply_chunk into pieces changed the code of the existing apply instances, which the
// sweep must not do.  Whoever changes one loop changes the other.  Its first group_sync<L>, behind the write of the first tile, stands between the residual stage and
// the first read of R (the 128 class uses both waves for rows: there it is a workgroup barrier).  Lane i stores
// fma(omega, acc, x_old) to x'[first + i].
#include <cstdint>

#include "mi32_relax.h"
#include "mi32_stored_loader.h"

namespace mi32 {

constexpr int kSubLanes = 8;  // of a sub-group: the partial sums of the definition
constexpr int kInFlight = 4;  // the entries a lane loads before the first fma

// The residuals of the group's member: sink(i, r) in lane 0 of the sub-group that took block row i.  f: the member's
// first row; nmax: the largest order among the wave's groups (the member's own in the 128 class).
template <typename T, typename I, int L, typename Sink>
__device__ __forceinline__ void block_residual(const RelaxArgs<T> &a, const int lane, const int n, const int nmax,
                                               const long long f, const Sink &sink)
{
    constexpr int S = L / kSubLanes;
    const I *rp = static_cast<const I *>(a.row_ptr);
    const I *col = static_cast<const I *>(a.col);
    const int sub = lane / kSubLanes, s = lane % kSubLanes;
    const int rounds = (nmax + S - 1) / S;  // (wave-uniform; workgroup-uniform for L = 128)
    int i = sub;
    long long k = 0, end = 0;
    T bi = T(0);
    if (i < n) {
        k = (long long)rp[f + i];
        end = (long long)rp[f + i + 1];
        bi = a.b[f + i];
    }
    for (int t = 0; t < rounds; ++t) {
        // the next round's row: its range and b, ahead of this round's entries
        const int inext = i + S;
        long long knext = 0, endnext = 0;
        T bnext = T(0);
        if (inext < n) {
            knext = (long long)rp[f + inext];
            endnext = (long long)rp[f + inext + 1];
            bnext = a.b[f + inext];
        }
        T p = T(0);
        for (k += s; k < end; k += kSubLanes * kInFlight) {  // (divergent: rows differ in length)
            size_t c[kInFlight];
            T v[kInFlight], xv[kInFlight];
#pragma unroll
            for (int u = 0; u < kInFlight; ++u) {
                const long long ku = k + u * kSubLanes;
                c[u] = 0;  // (x[0] exists: the gather of a lane past the row's end needs no branch)
                v[u] = T(0);
                if (ku < end) {
                    c[u] = (size_t)col[ku];
                    v[u] = a.val[ku];
                }
            }
#pragma unroll
            for (int u = 0; u < kInFlight; ++u) xv[u] = a.x[c[u]];
#pragma unroll
            for (int u = 0; u < kInFlight; ++u)
                if (k + u * kSubLanes < end) p = fma_t(v[u], xv[u], p);
        }
        const T q = p + __shfl_xor(p, 4, 64);
        const T w = q + __shfl_xor(q, 2, 64);
        const T sum = w + __shfl_xor(w, 1, 64);
        if (s == 0 && i < n) sink(i, bi - sum);
        i = inext;
        k = knext;
        end = endnext;
        bi = bnext;
    }
}

// I: the index type of row_ptr and col.  kSweep: the fused sweep; false: the residual alone, which needs no LDS.
template <typename T, typename I, int L, bool kSweep>
__global__ __launch_bounds__(walk_threads(L), 2) void relax_stored_vkernel(const RelaxArgs<T> a, const int first,
                                                                         const int count)
{
    const MemberSlot g = member_slot<L>(a.orders, a.members, first, count);
    const int nmax = wave_max<L>(g.n);
    const long long f = g.valid ? a.first[g.m] : 0;
    if constexpr (kSweep) {
        using G = ApplyGeom<T, L>;
        using Ld = StoredLoader<T>;
        __shared__ T xs[G::kThreads * G::kPitch];
        __shared__ T rs[G::kGroups * G::kRGroup];
        StoredMember<T> mb{nullptr, nullptr, nullptr, g.n, nmax, 1, 1, MI32_STORE_NATIVE};
        if (g.valid) {
            mb.x = a.store + a.offset[g.m];
            mb.fmt = a.format[g.m];
        }
        if constexpr (L >= 64) mb.fmt = __builtin_amdgcn_readfirstlane(mb.fmt);  // one member per wave: scalar branches
        T *xg = xs + g.grp * (L * G::kPitch), *rg = rs + g.grp * G::kRGroup;
        const int trow = g.lane / G::TJ, tcol = g.lane % G::TJ;
        typename Ld::Raw pf[G::TJ];
        Ld::template load_tile<L>(mb, 0, trow, tcol, pf);
        const T xold = g.lane < g.n ? a.x[f + g.lane] : T(0);
        // R: the member's residuals, MINUS zero past its order (beside X's +0 the padded product is exactly -0)
        if (g.lane >= g.n) rg[g.lane] = T(-0.0);
        block_residual<T, I, L>(a, g.lane, g.n, nmax, f, [&](const int i, const T r) { rg[i] = r; });
        // the loop of apply_chunk<T, L, 1, Ld> (see the top); its first group_sync orders R before its reads
        T acc = T(0);
        const T *xrow = xg + g.lane * G::kPitch;
        for (int j0 = 0; j0 < nmax; j0 += G::TJ) {  // (workgroup-uniform for L = 128: nmax is the member's order)
            Ld::template write_tile<L>(mb, xg, trow, tcol, pf);
            group_sync<L>();
            if (j0 + G::TJ < nmax) Ld::template load_tile<L>(mb, j0 + G::TJ, trow, tcol, pf);
            const int jn = nmax - j0 < G::TJ ? nmax - j0 : G::TJ;
            const T *rj = rg + j0;
#pragma unroll 8
            for (int jj = 0; jj < jn; ++jj) acc = fma_t(xrow[jj], rj[jj], acc);
            group_sync<L>();  // before the tile is overwritten
        }
        if (g.lane < g.n) a.xnew[f + g.lane] = fma_t(a.omega, acc, xold);
    } else {
        T *r = g.valid ? a.r[g.m] : nullptr;
        block_residual<T, I, L>(a, g.lane, g.n, nmax, f, [&](const int i, const T v) { r[i] = v; });
    }
}

template <typename T>
hipError_t relax_vlaunch(int lanes, const RelaxArgs<T> &a, int first, int count, hipStream_t stream, Profiler *prof)
{
    if (count <= 0 || first < 0 || !a.orders || !a.members || !a.row_ptr || !a.col || !a.val || !a.first || !a.x || !a.b)
        return hipErrorInvalidValue;
    if (a.index_bytes != 4 && a.index_bytes != 8) return hipErrorInvalidValue;
    const bool sweep = a.xnew != nullptr;
    if (sweep == (a.r != nullptr)) return hipErrorInvalidValue;
    if (sweep && (!a.store || !a.offset || !a.format)) return hipErrorInvalidValue;
    const bool narrow = a.index_bytes == 4;
    if (sweep) {
        const auto k32 = [](auto l) { return relax_stored_vkernel<T, int32_t, decltype(l)::value, true>; };
        const auto k64 = [](auto l) { return relax_stored_vkernel<T, int64_t, decltype(l)::value, true>; };
        return narrow ? member_walk_launch(lanes, k32, a, first, count, stream, prof)
                      : member_walk_launch(lanes, k64, a, first, count, stream, prof);
    }
    const auto k32 = [](auto l) { return relax_stored_vkernel<T, int32_t, decltype(l)::value, false>; };
    const auto k64 = [](auto l) { return relax_stored_vkernel<T, int64_t, decltype(l)::value, false>; };
    return narrow ? member_walk_launch(lanes, k32, a, first, count, stream, prof)
                  : member_walk_launch(lanes, k64, a, first, count, stream, prof);
}
template hipError_t relax_vlaunch(int, const RelaxArgs<float> &, int, int, hipStream_t, Profiler *);
template hipError_t relax_vlaunch(int, const RelaxArgs<double> &, int, int, hipStream_t, Profiler *);

}  // namespace mi32
