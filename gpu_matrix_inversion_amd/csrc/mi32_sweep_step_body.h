// mi32_sweep_step_body.h -- the body of gj_sweep_step_kernel and of its det twin gj_sweep_step_det_kernel
// (mi32_sweep.hip), included INTO both kernels: the plain kernel sees the very tokens it always had, so its instances
// compile to the same code; with MI32_STEP_DET defined the thread that updates orig and the status also stores the
// step's pivot and counts the exchange (mi32_det_large.h).  No include guard: it is included twice on purpose.
    __shared__ PivotRec<T> s_key[kSweepThreads / 64];
    const int b = blockIdx.z;
    const int tid = threadIdx.x;
    const T *src = src_all + (size_t)b * wstride;
    T *dst = dst_all + (size_t)b * wstride;

    // 1. finalMaxPivot: reduce the per-row-tile records of column r
    int p = r;
    if constexpr (PIVOT) {
        PivotRec<T> k = PivotRec<T>::none();
        for (int t = tid; t < npart; t += kSweepThreads) {
            const PivotRec<T> o = keys_in[(size_t)b * npart + t];
            k = decltype(k)::best_of(o, k);
        }
        k = wave_max_rec<T>(k);
        if ((tid & 63) == 0) s_key[tid >> 6] = k;
        __syncthreads();
        {
            const PivotRec<T> a = PivotRec<T>::best_of(s_key[0], s_key[1]);
            const PivotRec<T> c = PivotRec<T>::best_of(s_key[2], s_key[3]);
            k = decltype(k)::best_of(a, c);
        }
        p = k.row(r);
    }
    const T piv = src[(size_t)p * ld + r];  // read before the swap, as mat_inv_32.cpp:70,129-130

    const int j4 = (blockIdx.x * kSweepThreads + tid) * 4;
    const bool active = j4 < ld;
    const int rc = r - j4;                   // component of column r inside this thread's group, if 0..3
    const bool has_r = (rc >= 0 && rc < 4);
    const int nc = r + 1 - j4;               // component of column r+1
    const bool has_next = PIVOT && (nc >= 0 && nc < 4) && (r + 1 < n);
    const int row0 = blockIdx.y * TR;

    // 2. fixRow: the normalised pivot row slice (IEEE division), identity entry -> 1/piv
    const Vec4<T> zero4 = {T(0), T(0), T(0), T(0)};
    Vec4<T> prn = zero4;
    if (active) {
        const Vec4<T> pr = *reinterpret_cast<const Vec4<T> *>(src + (size_t)p * ld + j4);
        prn.x = pr.x / piv;
        prn.y = pr.y / piv;
        prn.z = pr.z / piv;
        prn.w = pr.w / piv;
        if (has_r) set_comp<T>(prn, rc, T(1) / piv);
    }

    // 3. pivotElements + fixColumn over this workgroup's rows
    PivotRec<T> best = PivotRec<T>::none();
#pragma unroll
    for (int u0 = 0; u0 < TR; u0 += 4) {
        T f[4];
        Vec4<T> v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = row0 + u0 + u;
            const int s = (i == p) ? r : i;  // slot p receives the old row r
            const bool ok = (i < n);
            f[u] = ok ? src[(size_t)s * ld + r] : T(0);
#ifdef MI32_STEP_DET  // a value, not the object zero4: the plain kernel's form below selects between two ADDRESSES, which
                      // keeps zero4 in 32 / 64 bytes of scratch -- its instances stay as they are, the twin needs none
            v[u] = (ok && active) ? *reinterpret_cast<const Vec4<T> *>(src + (size_t)s * ld + j4)
                                  : Vec4<T>{T(0), T(0), T(0), T(0)};
#else
            v[u] = (ok && active) ? *reinterpret_cast<const Vec4<T> *>(src + (size_t)s * ld + j4) : zero4;
#endif
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = row0 + u0 + u;
            if (i >= n || !active) continue;
            Vec4<T> o;
            if (i == r) {
                o = prn;
            } else {
                o = v[u];
                if (has_r) set_comp<T>(o, rc, T(0));  // the implicit identity column's entry in this row
                if (f[u] != T(0)) o = fma4_neg<T>(f[u], prn, o);
            }
            *reinterpret_cast<Vec4<T> *>(dst + (size_t)i * ld + j4) = o;
            if (has_next && i > r) {
                const PivotRec<T> kk = PivotRec<T>::make(comp<T>(o, nc), i);
                best = decltype(best)::best_of(kk, best);
            }
        }
    }
    // 4. maxPivot record of column r+1 for the next launch
    if (has_next && active) keys_out[(size_t)b * npart + blockIdx.y] = best;

    if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) {
        if (p != r) {
            int *og = orig + (size_t)b * n;
            const int t = og[r];
            og[r] = og[p];
            og[p] = t;
        }
        if (status && (piv == T(0) || piv - piv != T(0))) status[b] = MI32_SINGULAR;  // zero, NaN or infinite pivot
#ifdef MI32_STEP_DET  // the det twin: this thread owns the parity word and the launches are ordered
        det_piv[(size_t)b * det_pstride + r] = piv;
        if (p != r) det_parity[b] ^= 1;
#endif
    }
