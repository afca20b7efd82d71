/*
 * tri_panel_mirror.c -- plain-C restatement of the blocked fp32 inversion with TRIANGULAR panel steps (test code only;
 * built by tests/test_tri_panel_mirror.py with -ffp-contract=off, every fused multiply-add spelled out).
 *
 * The in-place N x N Gauss-Jordan elimination with partial pivoting, in sub-panels of W pivot columns.  Inside a
 * sub-panel, step R
 *   - searches column R (largest |a| from the diagonal down, first maximum wins), swaps,
 *   - updates the columns c > R of the sub-panel only; a column c <= R keeps what it held when its own step ran: the
 *     row's multiplier of that step (in the pivot row: the pivot).
 * After the last step
 *   - the entries of the W pivot rows LEFT of their pivots come from a recursion over the kept multipliers, with one
 *     IEEE division each;
 *   - the finished entries of every row in the sub-panel's own columns (G_s) are rebuilt from the row's W multipliers
 *     and the normalised pivot rows;
 *   - every other column takes the W steps from its old value.
 * Each of these is the fmaf chain the step-by-step elimination applies to the same element, in its order.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

static float cand_abs(float x)
{
    float v = fabsf(x);
    return (v == v) ? v : -1.0f; /* a NaN never wins the search */
}

static int bad_pivot(float p) { return p == 0.0f || p != p || p - p != 0.0f; }

/* in, out: n x n row-major.  Returns 0, or 2 when a pivot was zero or not finite or the input holds such an entry. */
int tri_panel_inverse(const float *in, int n, int W, float *out)
{
    const size_t ld = (size_t)n;
    float *m = (float *)malloc(sizeof(float) * ld * n);
    float *s = (float *)malloc(sizeof(float) * ld * W);   /* the slab: n rows x w columns */
    float *prn = (float *)malloc(sizeof(float) * W * W);  /* prn[R][c]: the normalised pivot row of step R */
    int *orig = (int *)malloc(sizeof(int) * n);
    int status = 0;
    memcpy(m, in, sizeof(float) * ld * n);
    for (int i = 0; i < n; ++i) orig[i] = i;
    for (size_t i = 0; i < ld * n; ++i)
        if (in[i] - in[i] != 0.0f) status = 2;

    for (int c0 = 0; c0 < n; c0 += W) {
        const int w = (n - c0 < W) ? n - c0 : W;
        for (int i = 0; i < n; ++i)
            for (int c = 0; c < w; ++c) s[(size_t)i * W + c] = m[i * ld + c0 + c];
        /* ---- the W steps on the slab, upper triangle only */
        for (int R = 0; R < w; ++R) {
            const int r = c0 + R;
            int p = r;
            float best = cand_abs(s[(size_t)r * W + R]);
            for (int i = r + 1; i < n; ++i) {
                const float v = cand_abs(s[(size_t)i * W + R]);
                if (v > best) { best = v; p = i; }
            }
            if (p != r) { /* whole rows move: the slab (kept multipliers included) and every other column */
                for (int c = 0; c < w; ++c) {
                    const float t = s[(size_t)r * W + c];
                    s[(size_t)r * W + c] = s[(size_t)p * W + c];
                    s[(size_t)p * W + c] = t;
                }
                for (int j = 0; j < n; ++j) {
                    const float t = m[r * ld + j];
                    m[r * ld + j] = m[p * ld + j];
                    m[p * ld + j] = t;
                }
                const int t = orig[r];
                orig[r] = orig[p];
                orig[p] = t;
            }
            const float piv = s[(size_t)r * W + R];
            if (bad_pivot(piv)) status = 2;
            prn[R * W + R] = 1.0f / piv;
            for (int c = R + 1; c < w; ++c) prn[R * W + c] = s[(size_t)r * W + c] / piv;
            for (int i = 0; i < n; ++i) {
                if (i == r) continue;
                const float f = s[(size_t)i * W + R]; /* stays in column R: the row's multiplier of this step */
                for (int c = R + 1; c < w; ++c) s[(size_t)i * W + c] = fmaf(-f, prn[R * W + c], s[(size_t)i * W + c]);
            }
            for (int c = R + 1; c < w; ++c) s[(size_t)r * W + c] = prn[R * W + c]; /* columns <= R: as found */
        }
        /* ---- the pivot rows left of their pivots: the recursion over the kept multipliers */
        for (int R = 1; R < w; ++R) {
            const float *rec = s + (size_t)(c0 + R) * W; /* [m < R]: multipliers, [R]: the pivot */
            for (int c = 0; c < R; ++c) {
                float v = 0.0f;
                for (int k = c; k < R; ++k) v = fmaf(-rec[k], prn[k * W + c], v);
                prn[R * W + c] = v / rec[R];
            }
        }
        /* ---- every other column: the W steps from the old value (the pivot row is normalised by its own step) */
        for (int R = 0; R < w; ++R) {
            const int r = c0 + R;
            const float piv = s[(size_t)r * W + R];
            for (int j = 0; j < n; ++j) {
                if (j >= c0 && j < c0 + w) continue;
                m[r * ld + j] = m[r * ld + j] / piv;
            }
            for (int i = 0; i < n; ++i) {
                if (i == r) continue;
                const float f = s[(size_t)i * W + R];
                for (int j = 0; j < n; ++j) {
                    if (j >= c0 && j < c0 + w) continue;
                    m[i * ld + j] = fmaf(-f, m[r * ld + j], m[i * ld + j]);
                }
            }
        }
        /* ---- G_s of every row from its multipliers and the normalised pivot rows */
        for (int i = 0; i < n; ++i) {
            const int ps = i - c0; /* the row's own pivot step, if it has one */
            for (int c = 0; c < w; ++c) {
                float v = 0.0f;
                for (int k = c; k < w; ++k)
                    v = (k == ps) ? prn[k * W + c] : fmaf(-s[(size_t)i * W + k], prn[k * W + c], v);
                m[i * ld + c0 + c] = v;
            }
        }
    }
    for (int i = 0; i < n; ++i)
        for (int c = 0; c < n; ++c) out[(size_t)i * n + orig[c]] = m[i * ld + c];
    free(m);
    free(s);
    free(prn);
    free(orig);
    return status;
}
