// mi32_b64_step_body.h -- the body of b64_panel_step_kernel and of its det twin b64_panel_step_det_kernel
// (mi32_blocked64.hip), included INTO both kernels: the plain kernel sees the very tokens it always had, so its
// instances compile to the same code; with MI32_STEP_DET defined the thread that updates the maps and the status also
// stores the step's pivot and counts the exchange (mi32_det_large.h).  No include guard: it is included twice on purpose.
    constexpr int TY = kB64Threads / TX;  // rows per pass
    __shared__ PivotRec<double> s_key[kB64Threads / 64];
    const int b = blockIdx.z;
    const int tid = threadIdx.x;
    const double *src = src_all + (size_t)b * wstride;
    double *dst = dst_all + (size_t)b * wstride;

    const int tx = tid % TX, ty = tid / TX;
    const int j4 = col_lo + tx * 4;
    const int rc = r - j4;  // component of column r inside this thread's group, if 0..3
    const bool has_r = (rc >= 0 && rc < 4);
    const int nc = r + 1 - j4;
    const bool has_next = (nc >= 0 && nc < 4);  // column r + 1 belongs to this window and this thread
    const int row0 = blockIdx.y * TR;

    // The step is a chain of dependent global-memory round trips (records -> pivot row -> rows): this workgroup's
    // rows do not depend on the pivot search (but for the one row that receives the old row r), so they are
    // requested FIRST and arrive while the records are reduced and the pivot row is fetched.
    constexpr int NP = (TR + TY - 1) / TY;  // passes over the rows
    double fv[NP];
    Vec4<double> vv[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const int i = row0 + ty + q * TY;
        const bool ok = (ty + q * TY < TR) && (i < np);
        fv[q] = ok ? src[(size_t)i * ld + r] : 0.0;
        vv[q] = ok ? *reinterpret_cast<const Vec4<double> *>(src + (size_t)i * ld + j4) : Vec4<double>{0.0, 0.0, 0.0, 0.0};
    }

    // finalMaxPivot: reduce the per-row-tile records of column r
    PivotRec<double> k = PivotRec<double>::none();
    for (int t = tid; t < npart; t += kB64Threads) {
        const PivotRec<double> o = keys_in[(size_t)b * npart + t];
        k = decltype(k)::best_of(o, k);
    }
    k = wave_max_rec<double>(k);
    if ((tid & 63) == 0) s_key[tid >> 6] = k;
    __syncthreads();
    {
        const PivotRec<double> a = PivotRec<double>::best_of(s_key[0], s_key[1]);
        const PivotRec<double> c = PivotRec<double>::best_of(s_key[2], s_key[3]);
        k = decltype(k)::best_of(a, c);
    }
    const int p = k.row(r);
    const double piv = src[(size_t)p * ld + r];  // read before the swap, as mat_inv_32.cpp:70,129-130

    // fixRow: the normalised pivot row slice (IEEE division), identity entry -> 1/piv
    Vec4<double> prn;
    {
        const Vec4<double> pr = *reinterpret_cast<const Vec4<double> *>(src + (size_t)p * ld + j4);
        prn.x = pr.x / piv;
        prn.y = pr.y / piv;
        prn.z = pr.z / piv;
        prn.w = pr.w / piv;
        if (has_r) {
            const double one = 1.0 / piv;
            if (rc == 0) prn.x = one; else if (rc == 1) prn.y = one; else if (rc == 2) prn.z = one; else prn.w = one;
        }
    }
    // pivotElements + fixColumn over this workgroup's rows
    PivotRec<double> best = PivotRec<double>::none();
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const int i = row0 + ty + q * TY;
        if (!((ty + q * TY < TR) && (i < np))) continue;
        double f = fv[q];
        Vec4<double> o = vv[q];
        if (i == p && p != r) {  // slot p receives the old row r (the swap of pivotElements, done by redirecting the read)
            f = src[(size_t)r * ld + r];
            o = *reinterpret_cast<const Vec4<double> *>(src + (size_t)r * ld + j4);
        }
        if (i == r) {
            o = prn;
        } else {
            if (has_r) {  // the implicit identity column's entry in this row
                if (rc == 0) o.x = 0.0; else if (rc == 1) o.y = 0.0; else if (rc == 2) o.z = 0.0; else o.w = 0.0;
            }
            if (f != 0.0) {
                o.x = __builtin_fma(-f, prn.x, o.x);
                o.y = __builtin_fma(-f, prn.y, o.y);
                o.z = __builtin_fma(-f, prn.z, o.z);
                o.w = __builtin_fma(-f, prn.w, o.w);
            }
        }
        *reinterpret_cast<Vec4<double> *>(dst + (size_t)i * ld + j4) = o;
        if (has_next && i > r) {
            const double v = (nc == 0) ? o.x : (nc == 1) ? o.y : (nc == 2) ? o.z : o.w;
            const PivotRec<double> kk = PivotRec<double>::make(v, i);
            best = decltype(best)::best_of(kk, best);
        }
    }
    // maxPivot record of column r + 1 for the next launch: the TY threads (one tx) that own that column hold
    // partial results; thread (tx, 0) folds them.  Absent at the last step of a window (column r + 1 then belongs
    // to the next block: b64_block_prep_kernel writes its records after the rank-bw update).
    __shared__ PivotRec<double> s_part[TY];
    if (has_next) s_part[ty] = best;
    __syncthreads();
    if (has_next && ty == 0) {
        PivotRec<double> m = s_part[0];
#pragma unroll
        for (int q = 1; q < TY; ++q) m = PivotRec<double>::best_of(s_part[q], m);
        keys_out[(size_t)b * npart + blockIdx.y] = m;
    }
    if (blockIdx.y == 0 && tid == 0) {
        if (p != r) {
            int *og = orig + (size_t)b * np;
            const int t = og[r]; og[r] = og[p]; og[p] = t;
            int *rm = rowmap + (size_t)b * np;
            const int t2 = rm[r]; rm[r] = rm[p]; rm[p] = t2;
        }
        if (status && (piv == 0.0 || piv - piv != 0.0)) status[b] = MI32_SINGULAR;  // zero, NaN or infinite pivot
#ifdef MI32_STEP_DET  // the det twin: this thread owns the parity word and the launches are ordered
        det_piv[(size_t)b * det_pstride + r] = piv;
        if (p != r) det_parity[b] ^= 1;
#endif
    }
