/* asg_oracle.c -- CPU oracle of affine-gap semi-global alignment (DPX_ALGO_ASG), written from the definition in include/dpx_align.h,
 * not from the kernels.  TEST INFRASTRUCTURE ONLY: the test module builds it with `cc -O2 -shared -fPIC` into a temporary directory.
 *
 *   H[0][j] = 0 (0 <= j <= n); H[i][0] = o + i*e (i >= 1); I and D have virtual -inf borders (row 1 / column 1 always open)
 *   D[i][j] = max(H[i-1][j] + o + e, D[i-1][j] + e)      dirD = GAP_OPEN (1) if the open term >= the extend term, else GAP_EXTEND (2)
 *   I[i][j] = max(H[i][j-1] + o + e, I[i][j-1] + e)      dirI likewise
 *   best = H[i-1][j-1] + s, move = MATCH (1) / MISMATCH (2); D >= best: QUERY_DELETION (4); then I >= best: QUERY_INSERTION (3)
 *   H[i][j] = best (no floor); dirH = the move; on the borders NONE_MAIN (0) along row 0, QUERY_DELETION (4) down column 0
 * Score = max over 0 <= j <= n of H[m][j], end cell = (m, smallest such j).  The walk starts there in SCORING and runs while
 * i != 0 && j != 0: follow the move; INSERTION emits ref / ' ' / '_' and leaves on GAP_OPEN, DELETION emits '_' / ' ' / qry.  Then the
 * remaining i query characters are deletions; the remaining reference characters are not emitted.
 * Matrices are int32 row-major (m+1) x (n+1) computed in 64 bits; the enum matrices uint8; I and D borders are 0.  Lines are
 * NUL-terminated. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define NEG_INF (-(1ll << 40))

int asg_fill(const unsigned char *ref, int n, const unsigned char *qry, int m, int match, int mismatch, int o, int e,
             int32_t *H, int32_t *I, int32_t *D, uint8_t *dirH, uint8_t *dirI, uint8_t *dirD, int32_t *score, int32_t *endRow,
             int32_t *endCol) {
    const size_t W = (size_t)n + 1, cells = ((size_t)m + 1) * W;
    long long *h = calloc(cells, sizeof *h), *ii = malloc(cells * sizeof *ii), *dd = malloc(cells * sizeof *dd);
    if (!h || !ii || !dd) { free(h); free(ii); free(dd); return -1; }
    for (size_t k = 0; k < cells; k++) { ii[k] = NEG_INF; dd[k] = NEG_INF; }
    if (dirH) memset(dirH, 0, cells);
    if (dirI) memset(dirI, 0, cells);
    if (dirD) memset(dirD, 0, cells);
    for (int i = 1; i <= m; i++) {
        h[(size_t)i * W] = (long long)o + (long long)i * e;
        if (dirH) dirH[(size_t)i * W] = 4;
    }
    for (int i = 1; i <= m; i++) {
        for (int j = 1; j <= n; j++) {
            const size_t c = (size_t)i * W + (size_t)j, up = c - W, left = c - 1, dg = up - 1;
            const long long dOpen = h[up] + o + e, dExt = dd[up] + e;
            const long long iOpen = h[left] + o + e, iExt = ii[left] + e;
            dd[c] = dOpen >= dExt ? dOpen : dExt;
            ii[c] = iOpen >= iExt ? iOpen : iExt;
            if (dirD) dirD[c] = dOpen >= dExt ? 1 : 2;
            if (dirI) dirI[c] = iOpen >= iExt ? 1 : 2;
            long long b = h[dg] + (qry[i - 1] == ref[j - 1] ? match : mismatch);
            int mv = qry[i - 1] == ref[j - 1] ? 1 : 2;
            if (dd[c] >= b) { b = dd[c]; mv = 4; }
            if (ii[c] >= b) { b = ii[c]; mv = 3; }
            h[c] = b;
            if (dirH) dirH[c] = (uint8_t)mv;
        }
    }
    long long best = h[(size_t)m * W];
    int bj = 0;
    for (int j = 1; j <= n; j++)
        if (h[(size_t)m * W + (size_t)j] > best) { best = h[(size_t)m * W + (size_t)j]; bj = j; }
    for (size_t k = 0; k < cells; k++) {
        const int border = (k < W) || (k % W == 0);
        if (H) H[k] = (int32_t)h[k];
        if (I) I[k] = border ? 0 : (int32_t)ii[k];
        if (D) D[k] = border ? 0 : (int32_t)dd[k];
    }
    *score = (int32_t)best;
    *endRow = m;
    *endCol = bj;
    free(h); free(ii); free(dd);
    return 0;
}

/* the walk over the enum matrices of asg_fill; lines of capacity m + n + 1 each; returns the length */
int asg_walk(const unsigned char *ref, int n, const unsigned char *qry, int m, const uint8_t *dirH, const uint8_t *dirI,
             const uint8_t *dirD, int i, int j, char *lr, char *lx, char *lq) {
    const size_t W = (size_t)n + 1;
    const int cap = m + n;
    int pos = cap, state = 0; /* 0 SCORING, 1 INSERTION, 2 DELETION */
    while (i != 0 && j != 0) {
        const size_t c = (size_t)i * W + (size_t)j;
        if (state == 0) {
            const int mv = dirH[c];
            if (mv == 1 || mv == 2) {
                --pos; lr[pos] = (char)ref[j - 1]; lx[pos] = mv == 1 ? '*' : '|'; lq[pos] = (char)qry[i - 1];
                i--; j--;
            } else if (mv == 3) state = 1;
            else state = 2;
        } else if (state == 1) {
            --pos; lr[pos] = (char)ref[j - 1]; lx[pos] = ' '; lq[pos] = '_';
            if (dirI[c] == 1) state = 0;
            j--;
        } else {
            --pos; lr[pos] = '_'; lx[pos] = ' '; lq[pos] = (char)qry[i - 1];
            if (dirD[c] == 1) state = 0;
            i--;
        }
    }
    while (i > 0) { --pos; lr[pos] = '_'; lx[pos] = ' '; lq[pos] = (char)qry[i - 1]; i--; } /* column 0 drains the query; row 0 ends the walk */
    const int len = cap - pos;
    memmove(lr, lr + pos, (size_t)len); lr[len] = 0;
    memmove(lx, lx + pos, (size_t)len); lx[len] = 0;
    memmove(lq, lq + pos, (size_t)len); lq[len] = 0;
    return len;
}
