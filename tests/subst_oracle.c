/* subst_oracle.c -- CPU oracle of BANW / BAXT under a substitution table (dpx_batch_set_substitution), written from the definition in
 * include/dpx_align.h, not from the kernels.  TEST INFRASTRUCTURE ONLY: the test module builds it with `cc -O2 -shared -fPIC` into a
 * temporary directory.
 *
 *   s(r, q) = scores[codeOf[r] * alphabet + codeOf[q]]        (row = reference code, column = query code)
 *   cell (i, j), 0 <= i <= m, 0 <= j <= n, is in the band when |i - j| <= B - 1 (border cells too)
 *   H[0][0] = 0, H[i][0] = o + i*e, H[0][j] = o + j*e on the in-band borders; I = D = -inf on every border
 *   outside the band H = I = D = -inf (64-bit arithmetic and an explicit -inf: -inf plus anything stays -inf)
 *   D[i][j] = max(H[i-1][j] + o + e, D[i-1][j] + e)      dirD = GAP_OPEN (1) if the open term >= the extend term, else GAP_EXTEND (2)
 *   I[i][j] = max(H[i][j-1] + o + e, I[i][j-1] + e)      dirI likewise
 *   best = H[i-1][j-1] + s(ref[j-1], qry[i-1]), move = MATCH (1) if the BYTES are equal, else MISMATCH (2) -- the move only chooses the
 *   relation character; D >= best: QUERY_DELETION (4); then I >= best: QUERY_INSERTION (3)
 *   H[i][j] = best (no floor)
 * ext == 0 (BANW): score = H[m][n], end cell (m, n); returns -2 when |m - n| >= B.
 * ext != 0 (BAXT): score = the maximum of H over the in-band cells, borders and (0, 0) included; end cell = the first cell in row-major
 * order that holds it.
 * The walk starts at the end cell in SCORING and runs while i != 0 && j != 0: follow the move; INSERTION emits ref / ' ' / '_' and
 * leaves on GAP_OPEN, DELETION emits '_' / ' ' / qry; then the remaining i as deletions and the remaining j as insertions.
 * Matrices are int64 row-major (m+1) x (n+1) with SUBST_NEG_INF for -inf; the enum matrices uint8 (0 where nothing is computed).
 * Lines are NUL-terminated. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define SUBST_NEG_INF (-(1ll << 40))

static int in_band(int i, int j, int B) {
    const int d = i - j;
    return d <= B - 1 && -d <= B - 1;
}

static long long add(long long a, long long b) { return a == SUBST_NEG_INF ? SUBST_NEG_INF : a + b; }

long long subst_neg_inf(void) { return SUBST_NEG_INF; }

int subst_fill(const unsigned char *ref, int n, const unsigned char *qry, int m, const int8_t *scores, int alphabet,
               const uint8_t *codeOf, int o, int e, int B, int ext, int64_t *H, int64_t *I, int64_t *D, uint8_t *dirH, uint8_t *dirI,
               uint8_t *dirD, int64_t *score, int32_t *endRow, int32_t *endCol) {
    const size_t W = (size_t)n + 1, cells = ((size_t)m + 1) * W;
    if (B < 1 || m < 0 || n < 0 || alphabet < 1 || alphabet > 32) return -1;
    for (int x = 0; x < 256; x++) if (codeOf[x] >= alphabet) return -1;
    if (!ext && abs(m - n) >= B) return -2;
    long long *h = malloc(cells * sizeof *h), *ii = malloc(cells * sizeof *ii), *dd = malloc(cells * sizeof *dd);
    if (!h || !ii || !dd) { free(h); free(ii); free(dd); return -1; }
    for (size_t k = 0; k < cells; k++) { h[k] = SUBST_NEG_INF; ii[k] = SUBST_NEG_INF; dd[k] = SUBST_NEG_INF; }
    if (dirH) memset(dirH, 0, cells);
    if (dirI) memset(dirI, 0, cells);
    if (dirD) memset(dirD, 0, cells);
    h[0] = 0;
    for (int i = 1; i <= m; i++) if (in_band(i, 0, B)) h[(size_t)i * W] = (long long)o + (long long)i * e;
    for (int j = 1; j <= n; j++) if (in_band(0, j, B)) h[j] = (long long)o + (long long)j * e;
    for (int i = 1; i <= m; i++) {
        for (int j = 1; j <= n; j++) {
            if (!in_band(i, j, B)) continue;
            const size_t c = (size_t)i * W + (size_t)j, up = c - W, left = c - 1, dg = up - 1;
            const long long dOpen = add(h[up], (long long)o + e), dExt = add(dd[up], e);
            const long long iOpen = add(h[left], (long long)o + e), iExt = add(ii[left], e);
            dd[c] = dOpen >= dExt ? dOpen : dExt;
            ii[c] = iOpen >= iExt ? iOpen : iExt;
            if (dirD) dirD[c] = dOpen >= dExt ? 1 : 2;
            if (dirI) dirI[c] = iOpen >= iExt ? 1 : 2;
            const int s = scores[(int)codeOf[ref[j - 1]] * alphabet + (int)codeOf[qry[i - 1]]];
            long long b = add(h[dg], s);
            int mv = qry[i - 1] == ref[j - 1] ? 1 : 2;
            if (dd[c] >= b) { b = dd[c]; mv = 4; }
            if (ii[c] >= b) { b = ii[c]; mv = 3; }
            h[c] = b;
            if (dirH) dirH[c] = (uint8_t)mv;
        }
    }
    long long best = h[cells - 1];
    int bi = m, bj = n;
    if (ext) { /* the first maximum in row-major order over the in-band cells, starting from (0, 0) */
        best = h[0]; bi = 0; bj = 0;
        for (int i = 0; i <= m; i++)
            for (int j = 0; j <= n; j++)
                if (in_band(i, j, B) && h[(size_t)i * W + (size_t)j] > best) { best = h[(size_t)i * W + (size_t)j]; bi = i; bj = j; }
    }
    for (size_t k = 0; k < cells; k++) {
        if (H) H[k] = h[k];
        if (I) I[k] = ii[k];
        if (D) D[k] = dd[k];
    }
    *score = best;
    if (endRow) *endRow = bi;
    if (endCol) *endCol = bj;
    free(h); free(ii); free(dd);
    return 0;
}

/* the walk over the enum matrices of subst_fill from the end cell (i, j); lines of capacity m + n + 1 each.  Returns the length of the
 * lines, or -1 if the walk ever stood on a cell outside the band (the definition says it cannot) */
int subst_walk(const unsigned char *ref, int n, const unsigned char *qry, int m, int B, int i, int j, const uint8_t *dirH,
               const uint8_t *dirI, const uint8_t *dirD, char *lr, char *lx, char *lq) {
    const size_t W = (size_t)n + 1;
    const int cap = m + n;
    int pos = cap, state = 0; /* 0 SCORING, 1 INSERTION, 2 DELETION */
    while (i != 0 && j != 0) {
        const size_t c = (size_t)i * W + (size_t)j;
        if (!in_band(i, j, B)) return -1;
        if (state == 0) {
            const int mv = dirH[c];
            if (mv == 1 || mv == 2) {
                --pos; lr[pos] = (char)ref[j - 1]; lx[pos] = mv == 1 ? '*' : '|'; lq[pos] = (char)qry[i - 1];
                i--; j--;
            } else if (mv == 3) state = 1;
            else if (mv == 4) state = 2;
            else return -1;
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
    if (!in_band(i, j, B)) return -1;
    while (i > 0) { --pos; lr[pos] = '_'; lx[pos] = ' '; lq[pos] = (char)qry[i - 1]; i--; }
    while (j > 0) { --pos; lr[pos] = (char)ref[j - 1]; lx[pos] = ' '; lq[pos] = '_'; j--; }
    const int len = cap - pos;
    memmove(lr, lr + pos, (size_t)len); lr[len] = 0;
    memmove(lx, lx + pos, (size_t)len); lx[len] = 0;
    memmove(lq, lq + pos, (size_t)len); lq[len] = 0;
    return len;
}
