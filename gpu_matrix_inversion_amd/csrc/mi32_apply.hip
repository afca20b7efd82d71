// mi32_apply.hip -- Z_b = X_b R_b for the members of a variable-size batch: applying stored block inverses, the
// per-iteration half of a block-Jacobi preconditioner (mi32_apply_device_vbatched*).  Memory-bound: every element of X
// is read once per chunk of columns and takes part in one fused multiply-add per column.
//
// The arithmetic is fixed (mi32_apply.h): per component one chain of fused multiply-adds over j ascending, from +0.
// LANE = ROW: a group of L lanes owns one member and lane i keeps the accumulators of row i, so the chain runs inside
// one lane and nothing is reduced across lanes.
//
// X goes through LDS in tiles of TJ columns (128 bytes of a row, or the whole row of a narrower class).  The group
// loads a tile with consecutive lanes on consecutive elements of a row -- scalar loads, any alignment -- and writes
// it to LDS at the odd row pitch TJ + 1, so that the lane = row reads that follow fall into 64 different banks (fp64:
// 32 lanes on 32 bank pairs).  The chunk of R (n x KC) is staged once per chunk and read as a broadcast; the groups of
// a wave sit four elements further apart than their size, which keeps their broadcasts on different banks.  The next
// tile's global loads are issued before the current tile's multiply-adds and parked in registers.
//
// L <= 64: workgroups of 256 threads hold 256 / L members, every group inside one wave: no workgroup barrier, only
// program order within the wave.  Groups of different orders share a wave; every loop runs to the wave's largest order
// nmax, and what lies past a group's own order is staged as +0 in X and as -0 in R.  The padded product is then
// exactly -0, and fma(+0, -0, acc) = (-0) + acc returns acc for EVERY acc: +0, -0 (a chain can end in -0: a negative
// product below half the smallest subnormal rounds to it), every finite value, infinities and NaN.  (+0 in both
// factors would turn a final -0 into +0.)  So the padded terms change no bit, and a lane past the order stores
// nothing.  L = 128: one workgroup of 128 threads per member; the trip count of every loop with a barrier is the
// member's, uniform by construction.
//
// The body all of this describes -- geometry, chunk, column loop -- is in mi32_member_walk.h, written once around a loader
// and shared with apply_stored_vkernel (mi32_stored.hip).  Here: the plain loader, the kernel and its launch.
#include "mi32_member_walk.h"

namespace mi32 {

// what one group knows of its member
template <typename T>
struct ApplyMember {
    const T *x;
    const T *r;
    T *z;
    int n, nmax, ldx, ldr, ldz;
};

// the plain loader of the shared body (mi32_member_walk.h): X is T in memory, rows ldx elements apart, parked as it is
template <typename T>
struct ApplyLoader {
    using Member = ApplyMember<T>;
    using Raw = T;

    template <int L>
    static __device__ __forceinline__ void load_tile(const Member &mb, const int j0, const int trow, const int tcol,
                                                     T (&pf)[ApplyGeom<T, L>::TJ])
    {
        using G = ApplyGeom<T, L>;
        const int col = j0 + tcol;
#pragma unroll
        for (int t = 0; t < G::TJ; ++t) {
            const int row = t * G::kRows + trow;
            pf[t] = (row < mb.n && col < mb.n) ? mb.x[(size_t)row * mb.ldx + col] : T(0);
        }
    }
    template <int L>
    static __device__ __forceinline__ void write_tile(const Member &, T *xg, const int trow, const int tcol,
                                                      const T (&pf)[ApplyGeom<T, L>::TJ])
    {
        using G = ApplyGeom<T, L>;
#pragma unroll
        for (int t = 0; t < G::TJ; ++t) xg[(t * G::kRows + trow) * G::kPitch + tcol] = pf[t];
    }
};

// The member pointers carry no __restrict__: a member may be applied in place.
template <typename T, int L>
__global__ __launch_bounds__(walk_threads(L)) void apply_vkernel(const ApplyArgs<T> a, const int first, const int count)
{
    using G = ApplyGeom<T, L>;
    __shared__ T xs[G::kThreads * G::kPitch];
    __shared__ T rs[G::kGroups * G::kRGroup];
    const MemberSlot g = member_slot<L>(a.orders, a.members, first, count);
    ApplyMember<T> mb{nullptr, nullptr, nullptr, g.n, wave_max<L>(g.n), g.n, a.nrhs, a.nrhs};
    if (g.valid) {
        mb.x = a.x[g.m];
        mb.r = a.r[g.m];
        mb.z = a.z[g.m];
        if (a.ldx) mb.ldx = a.ldx[g.m];
        if (a.ldr) mb.ldr = a.ldr[g.m];
        if (a.ldz) mb.ldz = a.ldz[g.m];
    }
    apply_columns<T, L, ApplyLoader<T>>(mb, xs + g.grp * (L * G::kPitch), rs + g.grp * G::kRGroup, g.lane, a.nrhs);
}

template <typename T>
hipError_t apply_vlaunch(int lanes, const ApplyArgs<T> &a, int first, int count, hipStream_t stream, Profiler *prof)
{
    if (count <= 0 || first < 0 || a.nrhs < 1 || !a.orders || !a.members || !a.x || !a.r || !a.z) return hipErrorInvalidValue;
    return member_walk_launch(lanes, [](auto l) { return apply_vkernel<T, decltype(l)::value>; }, a, first, count, stream, prof);
}
template hipError_t apply_vlaunch(int, const ApplyArgs<float> &, int, int, hipStream_t, Profiler *);
template hipError_t apply_vlaunch(int, const ApplyArgs<double> &, int, int, hipStream_t, Profiler *);

}  // namespace mi32
