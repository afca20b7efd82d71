/* relax_mirror.c -- TEST INFRASTRUCTURE ONLY: the residual of a CSR row and the last step of a relaxation sweep in
 * float and in double, the expected values of the relaxation tests (tests/relax_cases.py).  The arithmetic is the
 * contract of include/mat_inv_32_relax.h, spelled out:
 *
 *     p_0 ... p_7 = +0;  for the row's entries e = 0 ... c-1 in stored order:  p[e mod 8] = fma(val_e, x[col_e], p[e mod 8])
 *     q_s = p_s + p_{s xor 4};  t_s = q_s + q_{s xor 2};  r = b - (t_0 + t_1)
 *
 * and  xnew = fma(omega, z, x)  per element.  row_ptr and col are int64 here, whatever the call under test takes.
 *
 * Built at test time with the host C compiler: -O2 -ffp-contract=off, linked with -lm. */
#include <math.h>
#include <stddef.h>

#define RELAX_MIRROR(SUFFIX, T, FMA)                                                                                 \
    void residual_mirror_##SUFFIX(long long nrows, const long long *rows, const long long *row_ptr,                  \
                                  const long long *col, const T *val, const T *x, const T *b, T *r)                  \
    {                                                                                                                \
        for (long long k = 0; k < nrows; ++k) {                                                                      \
            const long long g = rows[k], begin = row_ptr[g], end = row_ptr[g + 1];                                   \
            T p[8] = {0, 0, 0, 0, 0, 0, 0, 0}, q[8], t[8];                                                           \
            for (long long e = begin; e < end; ++e) p[(e - begin) & 7] = FMA(val[e], x[col[e]], p[(e - begin) & 7]); \
            for (int s = 0; s < 8; ++s) q[s] = p[s] + p[s ^ 4];                                                      \
            for (int s = 0; s < 8; ++s) t[s] = q[s] + q[s ^ 2];                                                      \
            r[k] = b[g] - (t[0] + t[1]);                                                                             \
        }                                                                                                            \
    }                                                                                                                \
    void axpy_mirror_##SUFFIX(long long n, T omega, const T *z, const T *x, T *xnew)                                 \
    {                                                                                                                \
        for (long long i = 0; i < n; ++i) xnew[i] = FMA(omega, z[i], x[i]);                                          \
    }

RELAX_MIRROR(f32, float, fmaf)
RELAX_MIRROR(f64, double, fma)
