/* basw_oracle.c -- CPU oracle of banded affine-gap Smith-Waterman (DPX_ALGO_BASW), written from the definition in
 * include/dpx_align.h, not from the kernels.  TEST INFRASTRUCTURE ONLY: the test module builds it with `cc -O2 -shared -fPIC` into a
 * temporary directory.
 *
 *   cell (i, j), 1 <= i <= m, 1 <= j <= n, is in the band when |i - j| <= B - 1
 *   every neighbour that is a border cell or lies outside the band reads H = 0, I = D = -inf (64-bit arithmetic, a true -inf)
 *   D[i][j] = max(H[i-1][j] + o + e, D[i-1][j] + e)      dirD = GAP_OPEN (1) if the open term >= the extend term, else GAP_EXTEND (2)
 *   I[i][j] = max(H[i][j-1] + o + e, I[i][j-1] + e)      dirI likewise
 *   best = H[i-1][j-1] + s, move = MATCH (1) / MISMATCH (2); D >= best: QUERY_DELETION (4); then I >= best: QUERY_INSERTION (3)
 *   H[i][j] = max(0, best); dirH = NONE_MAIN (0) where H == 0
 *   cells outside the band: H = 0 and every exported value (H, I, D, the three enums) is 0, as on the borders
 * Score = max H, end cell = its first cell in row-major order ((0, 0) and 0 when every H is 0).  The walk starts there in SCORING:
 * stop at H == 0, else follow the move; INSERTION emits ref / ' ' / '_' and leaves on GAP_OPEN, DELETION emits '_' / ' ' / qry.
 * Matrices are int32 row-major (m+1) x (n+1); the enum matrices uint8.  Lines are NUL-terminated. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define NEG_INF (-(1ll << 40))

static int in_band(int i, int j, int B) {
    const int d = i - j;
    return i >= 1 && j >= 1 && d <= B - 1 && -d <= B - 1;
}

int basw_fill(const unsigned char *ref, int n, const unsigned char *qry, int m, int match, int mismatch, int o, int e, int B,
              int32_t *H, int32_t *I, int32_t *D, uint8_t *dirH, uint8_t *dirI, uint8_t *dirD, int32_t *score, int32_t *endRow,
              int32_t *endCol) {
    const size_t W = (size_t)n + 1, cells = ((size_t)m + 1) * W;
    long long *h = calloc(cells, sizeof *h), *ii = malloc(cells * sizeof *ii), *dd = malloc(cells * sizeof *dd);
    if (!h || !ii || !dd || B < 1) { free(h); free(ii); free(dd); return -1; }
    /* cells that are never computed (borders, outside the band) keep H = 0, I = D = -inf: exactly what a neighbour reads there */
    for (size_t k = 0; k < cells; k++) { ii[k] = NEG_INF; dd[k] = NEG_INF; }
    if (dirH) memset(dirH, 0, cells);
    if (dirI) memset(dirI, 0, cells);
    if (dirD) memset(dirD, 0, cells);
    long long best = 0;
    int bi = 0, bj = 0;
    for (int i = 1; i <= m; i++) {
        for (int j = 1; j <= n; j++) {
            if (!in_band(i, j, B)) continue;
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
            h[c] = b > 0 ? b : 0;
            if (dirH) dirH[c] = h[c] == 0 ? 0 : (uint8_t)mv;
            if (h[c] > best) { best = h[c]; bi = i; bj = j; }
        }
    }
    for (size_t k = 0; k < cells; k++) {
        const int inside = in_band((int)(k / W), (int)(k % W), B);
        if (H) H[k] = (int32_t)h[k];
        if (I) I[k] = inside ? (int32_t)ii[k] : 0;
        if (D) D[k] = inside ? (int32_t)dd[k] : 0;
    }
    *score = (int32_t)best;
    *endRow = bi;
    *endCol = bj;
    free(h); free(ii); free(dd);
    return 0;
}

/* the walk over the enum matrices of basw_fill; lines of capacity m + n + 1 each; returns the length, or -1 if the walk ever stood on
 * a cell outside the band (the definition says it cannot) */
int basw_walk(const unsigned char *ref, int n, const unsigned char *qry, int m, int B, const int32_t *H, const uint8_t *dirH,
              const uint8_t *dirI, const uint8_t *dirD, int i, int j, char *lr, char *lx, char *lq) {
    const size_t W = (size_t)n + 1;
    const int cap = m + n;
    int pos = cap, state = 0; /* 0 SCORING, 1 INSERTION, 2 DELETION */
    while (i > 0 && j > 0) {
        const size_t c = (size_t)i * W + (size_t)j;
        if (state == 0) {
            if (H[c] == 0) break;
            if (!in_band(i, j, B)) return -1;
            const int mv = dirH[c];
            if (mv == 1 || mv == 2) {
                --pos; lr[pos] = (char)ref[j - 1]; lx[pos] = mv == 1 ? '*' : '|'; lq[pos] = (char)qry[i - 1];
                i--; j--;
            } else if (mv == 3) state = 1;
            else state = 2;
        } else if (state == 1) {
            if (!in_band(i, j, B)) return -1;
            --pos; lr[pos] = (char)ref[j - 1]; lx[pos] = ' '; lq[pos] = '_';
            if (dirI[c] == 1) state = 0;
            j--;
        } else {
            if (!in_band(i, j, B)) return -1;
            --pos; lr[pos] = '_'; lx[pos] = ' '; lq[pos] = (char)qry[i - 1];
            if (dirD[c] == 1) state = 0;
            i--;
        }
    }
    const int len = cap - pos;
    memmove(lr, lr + pos, (size_t)len); lr[len] = 0;
    memmove(lx, lx + pos, (size_t)len); lx[len] = 0;
    memmove(lq, lq + pos, (size_t)len); lq[len] = 0;
    return len;
}
