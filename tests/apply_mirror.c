/* apply_mirror.c -- TEST INFRASTRUCTURE ONLY: Z = X R in float and in double, the expected values of the apply tests
 * (tests/apply_cases.py).  X is n x n with rows ldx elements apart, R and Z are n x k with rows ldr / ldz apart, all
 * row-major.  The arithmetic is the contract of mi32_apply_device_vbatched, spelled out:
 *
 *     z[i][c] = acc after:  acc = +0;  for j = 0 ... n-1 ascending:  acc = fma(x[i][j], r[j][c], acc)
 *
 * one fused multiply-add per term in the element type, no term skipped.  Padding (the columns from n / k on) is neither
 * read nor written.
 *
 * Built at test time with the host C compiler: -O2 -ffp-contract=off, linked with -lm. */
#include <math.h>
#include <stddef.h>

#define APPLY_MIRROR(NAME, T, FMA)                                                                                   \
    void NAME(const T *x, int n, int ldx, const T *r, int k, int ldr, T *z, int ldz)                                \
    {                                                                                                               \
        for (int i = 0; i < n; ++i)                                                                                 \
            for (int c = 0; c < k; ++c) {                                                                           \
                T acc = (T)0;                                                                                       \
                for (int j = 0; j < n; ++j) acc = FMA(x[(size_t)i * ldx + j], r[(size_t)j * ldr + c], acc);         \
                z[(size_t)i * ldz + c] = acc;                                                                       \
            }                                                                                                       \
    }

APPLY_MIRROR(apply_mirror_f32, float, fmaf)
APPLY_MIRROR(apply_mirror_f64, double, fma)
