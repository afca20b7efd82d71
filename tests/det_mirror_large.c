/* det_mirror_large.c -- TEST INFRASTRUCTURE ONLY: the pivot-reporting mirrors of the determinant tests above order 128
 * (tests/det_large_cases.py).  The oracle (oracle/gj_oracle.c) reports no pivot values; tests/det_mirror.c restates
 * its step-by-step order serially, which is too slow at the orders the sweep and blocked paths serve.  Two mirrors:
 *
 *  (a) detl_steps_f32 / _f64: the step-by-step elimination of tests/det_mirror.c, in float and in double, with and
 *      without pivoting.  The row loop of a step runs in parallel where the compiler has OpenMP: every row is its own
 *      chain of fused multiply-adds, so no bit depends on the thread count.
 *  (b) detl_blocked_f64: the fp64 blocked order of the oracle's gjo_matrix_inv_64_blocked -- the steps of a block of
 *      bw columns on the block's columns only, then one delayed rank-bw update of every other column, a k-ascending
 *      fma chain per element starting from the old value.  The pivoted fp64 blocked path follows this order, so its
 *      pivots differ from (a)'s in the last bits.
 *
 * Both report every step's pivot value and whether the step exchanged two rows; the (mantissa, exponent) recurrence
 * stays tests/det_cases.py's frexp_det.  A zero, NaN or infinite pivot or a non-finite input entry gives status 2 and
 * the elimination goes on regardless.  tests/test_det_large_mirror.py holds both to the oracle bit for bit.
 *
 * Built at test time with the host C compiler: -O2 -ffp-contract=off (-fopenmp where it links), linked with -lm. */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

/* at most 16 threads, whatever the machine has */
static int detl_threads(long work)
{
#ifdef _OPENMP
    int t = omp_get_num_procs();
    if (t > 16) t = 16;
    if (work < 200000) t = 1;
    return t < 1 ? 1 : t;
#else
    (void)work;
    return 1;
#endif
}

#define DETL_STEPS(NAME, T, FMA, FABS)                                                                               \
    int NAME(const T *in, int n, T *out, T *pivot_value, int *swapped, int pivoting)                                  \
    {                                                                                                                 \
        T *a = (T *)malloc(sizeof(T) * (size_t)n * n);                                                                \
        T *prn = (T *)malloc(sizeof(T) * (size_t)n);                                                                  \
        int *orig = (int *)malloc(sizeof(int) * (size_t)n);                                                           \
        int bad = 0;                                                                                                  \
        if (!a || !prn || !orig) {                                                                                    \
            free(a);                                                                                                  \
            free(prn);                                                                                                \
            free(orig);                                                                                               \
            return 1;                                                                                                 \
        }                                                                                                             \
        memcpy(a, in, sizeof(T) * (size_t)n * n);                                                                     \
        for (int j = 0; j < n; ++j) orig[j] = j;                                                                      \
        for (size_t i = 0; i < (size_t)n * n; ++i)                                                                    \
            if (a[i] - a[i] != 0) bad = 1; /* a non-finite input entry */                                             \
        const int nthreads = detl_threads((long)n * n);                                                               \
        (void)nthreads;                                                                                               \
        for (int r = 0; r < n; ++r) {                                                                                 \
            int p = r;                                                                                                \
            if (pivoting) {                                                                                           \
                T best = (T)-1;                                                                                       \
                for (int i = r; i < n; ++i) {                                                                         \
                    const T v = FABS(a[(size_t)i * n + r]);                                                           \
                    if (v > best) { /* false for a NaN; the first of equal maxima is kept */                          \
                        best = v;                                                                                     \
                        p = i;                                                                                        \
                    }                                                                                                 \
                }                                                                                                     \
            }                                                                                                         \
            if (p != r) {                                                                                             \
                for (int j = 0; j < n; ++j) {                                                                         \
                    const T t = a[(size_t)r * n + j];                                                                 \
                    a[(size_t)r * n + j] = a[(size_t)p * n + j];                                                      \
                    a[(size_t)p * n + j] = t;                                                                         \
                }                                                                                                     \
                const int t = orig[r];                                                                                \
                orig[r] = orig[p];                                                                                    \
                orig[p] = t;                                                                                          \
            }                                                                                                         \
            const T piv = a[(size_t)r * n + r];                                                                       \
            pivot_value[r] = piv;                                                                                     \
            swapped[r] = p != r;                                                                                      \
            if (piv == 0 || piv - piv != 0) bad = 1;                                                                  \
            /* the normalised pivot row; the implicit identity column's 1 becomes 1 / piv */                          \
            for (int j = 0; j < n; ++j) prn[j] = (j == r ? (T)1 : a[(size_t)r * n + j]) / piv;                        \
            _Pragma("omp parallel for schedule(static) num_threads(nthreads)")                                        \
            for (int i = 0; i < n; ++i) {                                                                             \
                if (i == r) continue;                                                                                 \
                T *ai = a + (size_t)i * n;                                                                            \
                const T f = ai[r];                                                                                    \
                ai[r] = 0; /* the identity column's entry in this row */                                              \
                if (f != 0)                                                                                           \
                    for (int j = 0; j < n; ++j) ai[j] = FMA(-f, prn[j], ai[j]);                                       \
            }                                                                                                         \
            memcpy(a + (size_t)r * n, prn, sizeof(T) * (size_t)n);                                                    \
        }                                                                                                             \
        /* working column c holds inverse column orig[c] */                                                           \
        for (int i = 0; i < n; ++i)                                                                                   \
            for (int c = 0; c < n; ++c) out[(size_t)i * n + orig[c]] = a[(size_t)i * n + c];                          \
        free(a);                                                                                                      \
        free(prn);                                                                                                    \
        free(orig);                                                                                                   \
        return bad ? 2 : 0;                                                                                           \
    }

DETL_STEPS(detl_steps_f32, float, fmaf, fabsf)
DETL_STEPS(detl_steps_f64, double, fma, fabs)

int detl_blocked_f64(const double *in, int n, int bw, double *out, double *pivot_value, int *swapped)
{
    double *m = (double *)malloc(sizeof(double) * (size_t)n * n);
    double *rs = (double *)malloc(sizeof(double) * (size_t)bw * n);
    double *rowr = (double *)malloc(sizeof(double) * (size_t)bw);
    int *orig = (int *)malloc(sizeof(int) * (size_t)n);
    int bad = 0;
    if (!m || !rs || !rowr || !orig || bw <= 0) {
        free(m);
        free(rs);
        free(rowr);
        free(orig);
        return 1;
    }
    memcpy(m, in, sizeof(double) * (size_t)n * n);
    for (int i = 0; i < n; ++i) orig[i] = i;
    for (size_t i = 0; i < (size_t)n * n; ++i)
        if (m[i] - m[i] != 0) bad = 1;
    const int nthreads = detl_threads((long)n * n);
    (void)nthreads;
    for (int c0 = 0; c0 < n; c0 += bw) {
        const int kw = (c0 + bw <= n) ? bw : n - c0;
        for (int s = 0; s < kw; ++s) { /* the steps of (a) on the columns [c0, c0 + kw) */
            const int r = c0 + s;
            int p = r;
            double best = -1.0;
            for (int i = r; i < n; ++i) {
                const double v = fabs(m[(size_t)i * n + r]);
                if (v > best) {
                    best = v;
                    p = i;
                }
            }
            const double piv = m[(size_t)p * n + r];
            pivot_value[r] = piv;
            swapped[r] = p != r;
            if (piv == 0 || piv - piv != 0) bad = 1;
            if (p != r) { /* the exchange moves every column right away */
                for (int j = 0; j < n; ++j) {
                    const double t = m[(size_t)r * n + j];
                    m[(size_t)r * n + j] = m[(size_t)p * n + j];
                    m[(size_t)p * n + j] = t;
                }
                const int t = orig[r];
                orig[r] = orig[p];
                orig[p] = t;
            }
            double *mr = m + (size_t)r * n + c0;
            for (int c = 0; c < kw; ++c) mr[c] = mr[c] / piv;
            mr[s] = 1.0 / piv;
            memcpy(rowr, mr, sizeof(double) * (size_t)kw);
            for (int i = 0; i < n; ++i) {
                if (i == r) continue;
                double *mi = m + (size_t)i * n + c0;
                const double f = mi[s];
                mi[s] = 0.0;
                if (f != 0.0)
                    for (int c = 0; c < kw; ++c) mi[c] = fma(-f, rowr[c], mi[c]);
            }
        }
        if (kw == n) break;
        /* R = the block's pivot rows as they stand; every column outside the block: one chain from the old value */
        for (int k = 0; k < kw; ++k) memcpy(rs + (size_t)k * n, m + (size_t)(c0 + k) * n, sizeof(double) * (size_t)n);
#pragma omp parallel for schedule(static) num_threads(nthreads)
        for (int i = 0; i < n; ++i) {
            double *mi = m + (size_t)i * n;
            const double *g = mi + c0;
            const int in_block = (i >= c0 && i < c0 + kw);
            for (int j = 0; j < n; ++j) {
                if (j >= c0 && j < c0 + kw) continue;
                double acc = in_block ? 0.0 : mi[j];
                for (int k = 0; k < kw; ++k) acc = fma(g[k], rs[(size_t)k * n + j], acc);
                mi[j] = acc;
            }
        }
    }
    for (int i = 0; i < n; ++i)
        for (int c = 0; c < n; ++c) out[(size_t)i * n + orig[c]] = m[(size_t)i * n + c];
    free(m);
    free(rs);
    free(rowr);
    free(orig);
    return bad ? 2 : 0;
}
