/* dirtab_oracle.c -- CPU oracle of ANW, ASW and ASG under a substitution table (dpx_batch_set_direction_table), written from the
 * definitions in include/dpx_align.h, not from the kernels.  TEST INFRASTRUCTURE ONLY: the test modules build it with
 * `cc -O2 -shared -fPIC` into a temporary directory.
 *
 * kind 0 ANW, 1 ASW, 2 ASG.  int64 throughout, row by row.  With r the reference byte of column j and q the query byte of row i:
 *   s = scores[codeOf[r] * alphabet + codeOf[q]]                       (the row of the table is the reference code)
 *   borders   ANW: H[0][0] = 0, H[i][0] = o + i*e, H[0][j] = o + j*e;  ASW: all 0;  ASG: H[0][j] = 0, H[i][0] = o + i*e
 *             I and D are minus infinity on every border (row 1 / column 1 always open)
 *   D[i][j] = max(H[i-1][j] + o + e, D[i-1][j] + e)      dirD = GAP_OPEN (1) if the open term >= the extend term, else GAP_EXTEND (2)
 *   I[i][j] = max(H[i][j-1] + o + e, I[i][j-1] + e)      dirI likewise
 *   best = H[i-1][j-1] + s, move = MATCH (1) / MISMATCH (2) by BYTE equality; D >= best: QUERY_DELETION (4); then I >= best:
 *   QUERY_INSERTION (3);  H = best (ASW: max(0, best), and dirH = NONE (0) where H == 0)
 *   dirH on the borders: ANW row 0 QUERY_INSERTION, column 0 QUERY_DELETION, (0, 0) NONE; ASW NONE; ASG row 0 NONE, column 0
 *   QUERY_DELETION.  dirI / dirD are 0 on the borders.
 *   end cell  ANW (m, n); ASW the first strict maximum of H in row-major order, (0, 0) with score 0 when there is none; ASG the first
 *             maximum of row m over 0 <= j <= n.
 * The walk starts at the end cell in SCORING and runs while i != 0 && j != 0 (ASW: and stops in SCORING on a cell with H == 0): follow
 * the move; INSERTION emits ref / ' ' / '_' and leaves on GAP_OPEN, DELETION emits '_' / ' ' / qry likewise; a diagonal step prints '*'
 * where the two bytes are equal, else '|'.  Then ANW and ASG drain the remaining query ('_' / ' ' / qry), and ANW the remaining
 * reference.  Lines are NUL-terminated. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define NEG_INF (-(1ll << 40))

int dirtab_fill(int kind, const unsigned char *ref, int n, const unsigned char *qry, int m, const int8_t *scores, int alphabet,
                const uint8_t *codeOf, int o, int e, uint8_t *dirH, uint8_t *dirI, uint8_t *dirD, int64_t *score, int32_t *endRow,
                int32_t *endCol) {
    const size_t W = (size_t)n + 1;
    long long *hp = malloc(W * sizeof *hp), *hc = malloc(W * sizeof *hc), *dp = malloc(W * sizeof *dp), *dc = malloc(W * sizeof *dc);
    if (!hp || !hc || !dp || !dc) { free(hp); free(hc); free(dp); free(dc); return -1; }
    const int local = kind == 1, semi = kind == 2;
    hp[0] = 0; dp[0] = NEG_INF;
    if (dirH) dirH[0] = 0;
    if (dirI) dirI[0] = 0;
    if (dirD) dirD[0] = 0;
    for (int j = 1; j <= n; j++) {
        hp[j] = (local || semi) ? 0 : (long long)o + (long long)j * e;
        dp[j] = NEG_INF;
        if (dirH) dirH[j] = (local || semi) ? 0 : 3;
        if (dirI) dirI[j] = 0;
        if (dirD) dirD[j] = 0;
    }
    long long best = 0;
    int bi = 0, bj = 0;
    for (int i = 1; i <= m; i++) {
        const size_t row = (size_t)i * W;
        hc[0] = local ? 0 : (long long)o + (long long)i * e;
        dc[0] = NEG_INF;
        if (dirH) dirH[row] = local ? 0 : 4;
        if (dirI) dirI[row] = 0;
        if (dirD) dirD[row] = 0;
        long long ins = NEG_INF;
        const int qcode = codeOf[qry[i - 1]];
        for (int j = 1; j <= n; j++) {
            const long long dOpen = hp[j] + o + e, dExt = dp[j] + e;
            const long long iOpen = hc[j - 1] + o + e, iExt = ins + e;
            dc[j] = dOpen >= dExt ? dOpen : dExt;
            ins = iOpen >= iExt ? iOpen : iExt;
            if (dirD) dirD[row + (size_t)j] = dOpen >= dExt ? 1 : 2;
            if (dirI) dirI[row + (size_t)j] = iOpen >= iExt ? 1 : 2;
            long long b = hp[j - 1] + scores[(int)codeOf[ref[j - 1]] * alphabet + qcode];
            int mv = qry[i - 1] == ref[j - 1] ? 1 : 2;
            if (dc[j] >= b) { b = dc[j]; mv = 4; }
            if (ins >= b) { b = ins; mv = 3; }
            if (local && b <= 0) { b = 0; mv = 0; }
            hc[j] = b;
            if (dirH) dirH[row + (size_t)j] = (uint8_t)mv;
            if (local && b > best) { best = b; bi = i; bj = j; }
        }
        long long *t = hp; hp = hc; hc = t;
        t = dp; dp = dc; dc = t;
    }
    /* hp is row m */
    if (local) {
        *score = best; *endRow = bi; *endCol = bj;
    } else if (semi) {
        long long top = hp[0];
        int tj = 0;
        for (int j = 1; j <= n; j++) if (hp[j] > top) { top = hp[j]; tj = j; }
        *score = top; *endRow = m; *endCol = tj;
    } else {
        *score = hp[n]; *endRow = m; *endCol = n;
    }
    free(hp); free(hc); free(dp); free(dc);
    return 0;
}

/* the walk over the enum planes of dirtab_fill from (i, j); lines of capacity m + n + 1 each; returns the length, -1 on a plane that
 * does not say where to go */
int dirtab_walk(int kind, const unsigned char *ref, int n, const unsigned char *qry, int m, const uint8_t *dirH, const uint8_t *dirI,
                const uint8_t *dirD, int i, int j, char *lr, char *lx, char *lq) {
    const size_t W = (size_t)n + 1;
    const int cap = m + n;
    int pos = cap, state = 0; /* 0 SCORING, 1 INSERTION, 2 DELETION */
    while (i != 0 && j != 0) {
        const size_t c = (size_t)i * W + (size_t)j;
        if (state == 0) {
            const int mv = dirH[c];
            if (mv == 0) {
                if (kind != 1) return -1;
                break; /* ASW: H == 0 */
            }
            if (mv == 1 || mv == 2) {
                --pos; lr[pos] = (char)ref[j - 1]; lx[pos] = qry[i - 1] == ref[j - 1] ? '*' : '|'; lq[pos] = (char)qry[i - 1];
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
    if (kind != 1) {
        while (i > 0) { --pos; lr[pos] = '_'; lx[pos] = ' '; lq[pos] = (char)qry[i - 1]; i--; }
        if (kind == 0) while (j > 0) { --pos; lr[pos] = (char)ref[j - 1]; lx[pos] = ' '; lq[pos] = '_'; j--; }
    }
    const int len = cap - pos;
    memmove(lr, lr + pos, (size_t)len); lr[len] = 0;
    memmove(lx, lx + pos, (size_t)len); lx[len] = 0;
    memmove(lq, lq + pos, (size_t)len); lq[len] = 0;
    return len;
}
