/* solve_mirror.c -- TEST INFRASTRUCTURE ONLY: step-by-step Gauss-Jordan on [A | B] in float and in double, the
 * expected values of the solve tests (tests/solve_cases.py).  A is n x n, B is n x k, both row-major; X is B's final
 * content in natural row and column order.
 *
 * On A it is the in-place N x N form of tests/det_mirror.c, unchanged: the pivot is the largest |a| of column r at or
 * below row r, the LOWEST row among equal maxima, a NaN never wins; one IEEE division per element of the pivot row, one
 * fused multiply-add per element and step, a zero multiplier skips its row.  Every column of B takes, with the same p,
 * piv and f: the row exchange, prn = b[p] / piv, b[i] = fma(-f, prn, b[i]) unless f == 0, b[r] = prn.  A zero, NaN or
 * infinite pivot or a non-finite entry of A or of B flags the member (status 2) and the elimination goes on regardless.
 * A's columns never need un-permuting: only B is returned.  tests/test_solve_mirror.py holds it to the oracle bit for
 * bit through B = I.
 *
 * Built at test time with the host C compiler: -O2 -ffp-contract=off, linked with -lm. */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#define SOLVE_MIRROR(NAME, T, FMA, FABS)                                                                            \
    int NAME(const T *a_in, int n, const T *b_in, int k, T *x, int pivoting)                                        \
    {                                                                                                               \
        const int w = n + k; /* the augmented row: n working columns of A, then B's */                             \
        T *a = (T *)malloc(sizeof(T) * (size_t)n * w);                                                              \
        T *prn = (T *)malloc(sizeof(T) * (size_t)w);                                                                \
        int bad = 0;                                                                                                \
        if (!a || !prn) {                                                                                           \
            free(a);                                                                                                \
            free(prn);                                                                                              \
            return 1;                                                                                               \
        }                                                                                                           \
        for (int i = 0; i < n; ++i) {                                                                               \
            memcpy(a + (size_t)i * w, a_in + (size_t)i * n, sizeof(T) * (size_t)n);                                 \
            memcpy(a + (size_t)i * w + n, b_in + (size_t)i * k, sizeof(T) * (size_t)k);                             \
        }                                                                                                           \
        for (int i = 0; i < n * w; ++i)                                                                             \
            if (a[i] - a[i] != 0) bad = 1; /* a non-finite entry of A or of B */                                    \
        for (int r = 0; r < n; ++r) {                                                                               \
            int p = r;                                                                                              \
            if (pivoting) {                                                                                         \
                T best = (T)-1;                                                                                     \
                for (int i = r; i < n; ++i) {                                                                       \
                    const T v = FABS(a[i * w + r]);                                                                 \
                    if (v > best) { /* false for a NaN; the first of equal maxima is kept */                        \
                        best = v;                                                                                   \
                        p = i;                                                                                      \
                    }                                                                                               \
                }                                                                                                   \
            }                                                                                                       \
            if (p != r) {                                                                                           \
                for (int j = 0; j < w; ++j) {                                                                       \
                    const T t = a[r * w + j];                                                                       \
                    a[r * w + j] = a[p * w + j];                                                                    \
                    a[p * w + j] = t;                                                                               \
                }                                                                                                   \
            }                                                                                                       \
            const T piv = a[r * w + r];                                                                             \
            if (piv == 0 || piv - piv != 0) bad = 1;                                                                \
            /* the normalised pivot row; the implicit identity column's 1 becomes 1 / piv */                        \
            for (int j = 0; j < w; ++j) prn[j] = (j == r ? (T)1 : a[r * w + j]) / piv;                              \
            for (int i = 0; i < n; ++i) {                                                                           \
                if (i == r) continue;                                                                               \
                const T f = a[i * w + r];                                                                           \
                a[i * w + r] = 0; /* the identity column's entry in this row */                                     \
                if (f != 0)                                                                                         \
                    for (int j = 0; j < w; ++j) a[i * w + j] = FMA(-f, prn[j], a[i * w + j]);                       \
            }                                                                                                       \
            memcpy(a + (size_t)r * w, prn, sizeof(T) * (size_t)w);                                                  \
        }                                                                                                           \
        for (int i = 0; i < n; ++i) memcpy(x + (size_t)i * k, a + (size_t)i * w + n, sizeof(T) * (size_t)k);        \
        free(a);                                                                                                    \
        free(prn);                                                                                                  \
        return bad ? 2 : 0;                                                                                         \
    }

SOLVE_MIRROR(solve_mirror_f32, float, fmaf, fabsf)
SOLVE_MIRROR(solve_mirror_f64, double, fma, fabs)
