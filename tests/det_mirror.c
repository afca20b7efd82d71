/* det_mirror.c -- TEST INFRASTRUCTURE ONLY: a step-by-step Gauss-Jordan inversion in float and in double that also
 * reports every step's pivot value and whether the step exchanged two rows.  The determinant tests build the expected
 * (mantissa, exponent) pair from these with the recurrence of include/mat_inv_32_c.h (tests/det_cases.py).
 *
 * The arithmetic is the CPU oracle's (oracle/gj_oracle.c, in-place N x N form), restated because the oracle reports no
 * pivot values: one IEEE division per element of the pivot row, one fused multiply-add per element and step, a zero
 * multiplier skips its row; the pivot is the largest |a| of column r at or below row r, the LOWEST row among equal
 * maxima, and a NaN never wins; a zero, NaN or infinite pivot or a non-finite input entry flags the member (status 2)
 * and the elimination goes on regardless.  tests/test_det_mirror.py holds it to the oracle bit for bit.
 *
 * Built at test time with the host C compiler: -O2 -ffp-contract=off, linked with -lm. */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#define DET_MIRROR(NAME, T, FMA, FABS)                                                                              \
    int NAME(const T *in, int n, T *out, T *pivot_value, int *swapped, int pivoting)                                \
    {                                                                                                               \
        T *a = (T *)malloc(sizeof(T) * (size_t)n * n);                                                              \
        T *prn = (T *)malloc(sizeof(T) * (size_t)n);                                                                \
        int *orig = (int *)malloc(sizeof(int) * (size_t)n);                                                         \
        int bad = 0;                                                                                                \
        if (!a || !prn || !orig) {                                                                                  \
            free(a);                                                                                                \
            free(prn);                                                                                              \
            free(orig);                                                                                             \
            return 1;                                                                                               \
        }                                                                                                           \
        memcpy(a, in, sizeof(T) * (size_t)n * n);                                                                   \
        for (int j = 0; j < n; ++j) orig[j] = j;                                                                    \
        for (int i = 0; i < n * n; ++i)                                                                             \
            if (a[i] - a[i] != 0) bad = 1; /* a non-finite input entry */                                           \
        for (int r = 0; r < n; ++r) {                                                                               \
            int p = r;                                                                                              \
            if (pivoting) {                                                                                         \
                T best = (T)-1;                                                                                     \
                for (int i = r; i < n; ++i) {                                                                       \
                    const T v = FABS(a[i * n + r]);                                                                 \
                    if (v > best) { /* false for a NaN; the first of equal maxima is kept */                        \
                        best = v;                                                                                   \
                        p = i;                                                                                      \
                    }                                                                                               \
                }                                                                                                   \
            }                                                                                                       \
            if (p != r) {                                                                                           \
                for (int j = 0; j < n; ++j) {                                                                       \
                    const T t = a[r * n + j];                                                                       \
                    a[r * n + j] = a[p * n + j];                                                                    \
                    a[p * n + j] = t;                                                                               \
                }                                                                                                   \
                const int t = orig[r];                                                                              \
                orig[r] = orig[p];                                                                                  \
                orig[p] = t;                                                                                        \
            }                                                                                                       \
            const T piv = a[r * n + r];                                                                             \
            pivot_value[r] = piv;                                                                                   \
            swapped[r] = p != r;                                                                                    \
            if (piv == 0 || piv - piv != 0) bad = 1;                                                                \
            /* the normalised pivot row; the implicit identity column's 1 becomes 1 / piv */                        \
            for (int j = 0; j < n; ++j) prn[j] = (j == r ? (T)1 : a[r * n + j]) / piv;                              \
            for (int i = 0; i < n; ++i) {                                                                           \
                if (i == r) continue;                                                                               \
                const T f = a[i * n + r];                                                                           \
                a[i * n + r] = 0; /* the identity column's entry in this row */                                     \
                if (f != 0)                                                                                         \
                    for (int j = 0; j < n; ++j) a[i * n + j] = FMA(-f, prn[j], a[i * n + j]);                       \
            }                                                                                                       \
            memcpy(a + r * n, prn, sizeof(T) * (size_t)n);                                                          \
        }                                                                                                           \
        /* working column c holds inverse column orig[c] */                                                         \
        for (int i = 0; i < n; ++i)                                                                                 \
            for (int c = 0; c < n; ++c) out[i * n + orig[c]] = a[i * n + c];                                        \
        free(a);                                                                                                    \
        free(prn);                                                                                                  \
        free(orig);                                                                                                 \
        return bad ? 2 : 0;                                                                                         \
    }

DET_MIRROR(det_mirror_f32, float, fmaf, fabsf)
DET_MIRROR(det_mirror_f64, double, fma, fabs)
