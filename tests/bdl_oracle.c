/* bdl_oracle.c -- band-only CPU oracle of banded Smith-Waterman with linear gaps (DPX_ALGO_BSW) and affine gaps (DPX_ALGO_BASW), written
 * from the definitions in include/dpx_align.h, not from the kernels.  TEST INFRASTRUCTURE ONLY: bdl_ref.py builds it with
 * `cc -O2 -shared -fPIC` into a temporary directory.
 *
 * Only the band is kept: two rows of 64-bit H (and I, D) of 2B + 1 cells, and one byte per in-band cell for the walk, so the memory is
 * O((m + n) * B) and a 33 000-base pair is cheap.  Arithmetic is int64 with a true minus infinity.
 *
 *   cell (i, j), 1 <= i <= m, 1 <= j <= n, is in the band when |i - j| <= B - 1; every neighbour that is a border cell or lies outside
 *   the band reads H = 0 (BASW: I = D = -inf)
 *   BSW:  up = H[i-1][j] + g, left = H[i][j-1] + g, corner = H[i-1][j-1] + s, t = max of the three, H = max(0, t);
 *         dir = NONE (0) iff t < 0, else QUERY_DELETION (4) if up == H, else QUERY_INSERTION (3) if left == H, else MATCH (1) / MISMATCH (2)
 *   BASW: D = max(H[i-1][j] + o + e, D[i-1][j] + e), I = max(H[i][j-1] + o + e, I[i][j-1] + e), GAP_OPEN (1) wins a tie, else GAP_EXTEND (2);
 *         best = H[i-1][j-1] + s (1 / 2); D >= best: 4; then I >= best: 3; H = max(0, best); dirH = NONE where H == 0
 *   score = max H, end cell = its first cell in row-major order ((0, 0) and 0 when every H is 0)
 *   walk: from the end cell in SCORING; stop where H == 0 (a border cell and a cell outside the band have H = 0); BSW follows the cell's
 *         move one step at a time; BASW follows ASW's three states (a gap state leaves on GAP_OPEN)
 * Byte per in-band cell: bits 0-2 dirH, bit 3 H == 0, bits 4-5 dirI, bits 6-7 dirD. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define NEG_INF (-(1ll << 60))

static int in_band(int i, int j, int B) {
    const int d = i - j;
    return i >= 1 && j >= 1 && d <= B - 1 && -d <= B - 1;
}

/* lines of capacity m + n + 1 each (NUL-terminated on return); planes: NULL or three row-major (m+1) x (n+1) uint8 matrices (dirH, dirI,
 * dirD; BSW writes dirH only).  Returns the length of the lines, -1 on a bad argument or failed allocation, -2 if the walk met a cell
 * whose move is NONE while H > 0 (the definition says it cannot). */
int bdl_align(const unsigned char *ref, int n, const unsigned char *qry, int m, int affine, int match, int mismatch, int o, int e, int B,
              int64_t *score, int32_t *endRow, int32_t *endCol, char *lr, char *lx, char *lq, uint8_t *dirH, uint8_t *dirI, uint8_t *dirD) {
    if (B < 1 || m < 0 || n < 0) return -1;
    const size_t W = 2 * (size_t)B - 1;      /* in-band cells of a row: offset k = j - i + B - 1 in 0 .. 2B-2 */
    const size_t RW = W + 2;                 /* a row with one cell of slack on either side, which reads H = 0, I = D = -inf */
    long long *h = malloc(2 * RW * sizeof *h), *gi = malloc(2 * RW * sizeof *gi), *gd = malloc(2 * RW * sizeof *gd);
    uint8_t *cell = calloc((size_t)(m > 0 ? m : 1) * W, 1);
    if (!h || !gi || !gd || !cell) { free(h); free(gi); free(gd); free(cell); return -1; }
    const size_t full = ((size_t)m + 1) * ((size_t)n + 1);
    if (dirH) memset(dirH, 0, full);
    if (dirI) memset(dirI, 0, full);
    if (dirD) memset(dirD, 0, full);
    for (size_t k = 0; k < 2 * RW; k++) { h[k] = 0; gi[k] = NEG_INF; gd[k] = NEG_INF; }
    const long long g = affine ? (long long)o + e : (long long)o;
    long long best = 0;
    int bi = 0, bj = 0;
    for (int i = 1; i <= m; i++) {
        long long *hc = h + (size_t)(i & 1) * RW + 1, *hp = h + (size_t)((i - 1) & 1) * RW + 1; /* index k = j - i + B - 1 of their own row */
        long long *ic = gi + (size_t)(i & 1) * RW + 1, *dc = gd + (size_t)(i & 1) * RW + 1, *dp = gd + (size_t)((i - 1) & 1) * RW + 1;
        for (long long k = -1; k <= (long long)W; k++) { hc[k] = 0; ic[k] = NEG_INF; dc[k] = NEG_INF; }
        const int jlo = i - (B - 1) > 1 ? i - (B - 1) : 1, jhi = (long long)i + B - 1 < n ? i + B - 1 : n; /* the row's in-band columns */
        for (int j = jlo; j <= jhi; j++) {
            const long long k = (long long)j - i + B - 1;
            /* (i-1, j) is offset k + 1 of the previous row, (i-1, j-1) offset k, (i, j-1) offset k - 1 of this row; the slack cells, the
             * cells of row 0 (the previous row is all zeros when i == 1) and column 0 read H = 0, -inf */
            const long long upH = hp[k + 1], upD = dp[k + 1], dgH = hp[k];
            const long long leftH = (j == 1) ? 0 : hc[k - 1], leftI = (j == 1) ? NEG_INF : ic[k - 1];
            const int eq = qry[i - 1] == ref[j - 1];
            const long long corner = dgH + (eq ? match : mismatch);
            long long hv;
            uint8_t mv, di = 0, dd = 0;
            if (affine) {
                const long long dOpen = upH + g, dExt = upD + e, iOpen = leftH + g, iExt = leftI + e;
                dc[k] = dOpen >= dExt ? dOpen : dExt;
                ic[k] = iOpen >= iExt ? iOpen : iExt;
                dd = dOpen >= dExt ? 1 : 2;
                di = iOpen >= iExt ? 1 : 2;
                long long b = corner;
                mv = eq ? 1 : 2;
                if (dc[k] >= b) { b = dc[k]; mv = 4; }
                if (ic[k] >= b) { b = ic[k]; mv = 3; }
                hv = b > 0 ? b : 0;
                if (hv == 0) mv = 0;
            } else {
                const long long up = upH + g, left = leftH + g;
                long long t = up > left ? up : left;
                if (corner > t) t = corner;
                hv = t > 0 ? t : 0;
                mv = 0;
                if (t >= 0) mv = up == hv ? 4 : left == hv ? 3 : (eq ? 1 : 2);
            }
            hc[k] = hv;
            cell[(size_t)(i - 1) * W + (size_t)k] = (uint8_t)(mv | (hv == 0 ? 8 : 0) | (di << 4) | (dd << 6));
            if (dirH) dirH[(size_t)i * ((size_t)n + 1) + (size_t)j] = mv;
            if (affine && dirI) dirI[(size_t)i * ((size_t)n + 1) + (size_t)j] = di;
            if (affine && dirD) dirD[(size_t)i * ((size_t)n + 1) + (size_t)j] = dd;
            if (hv > best) { best = hv; bi = i; bj = j; }
        }
    }
    *score = best;
    *endRow = bi;
    *endCol = bj;
    const int cap = m + n;
    int pos = cap, state = 0, i = bi, j = bj, rc = 0; /* 0 SCORING, 1 INSERTION, 2 DELETION */
    while (i > 0 && j > 0) {
        if (!in_band(i, j, B)) break; /* H = 0: the walk stops (it can stand here in SCORING only) */
        const uint8_t c = cell[(size_t)(i - 1) * W + (size_t)(j - i + B - 1)];
        if (state == 0) {
            if (c & 8) break;
            const int mv = c & 7;
            if (mv == 1 || mv == 2) { --pos; lr[pos] = (char)ref[j - 1]; lx[pos] = mv == 1 ? '*' : '|'; lq[pos] = (char)qry[i - 1]; i--; j--; }
            else if (mv == 3) { if (affine) state = 1; else { --pos; lr[pos] = (char)ref[j - 1]; lx[pos] = ' '; lq[pos] = '_'; j--; } }
            else if (mv == 4) { if (affine) state = 2; else { --pos; lr[pos] = '_'; lx[pos] = ' '; lq[pos] = (char)qry[i - 1]; i--; } }
            else { rc = -2; break; }
        } else if (state == 1) {
            --pos; lr[pos] = (char)ref[j - 1]; lx[pos] = ' '; lq[pos] = '_';
            if (((c >> 4) & 3) == 1) state = 0;
            j--;
        } else {
            --pos; lr[pos] = '_'; lx[pos] = ' '; lq[pos] = (char)qry[i - 1];
            if (((c >> 6) & 3) == 1) state = 0;
            i--;
        }
    }
    if (state != 0 && rc == 0 && i > 0 && j > 0) rc = -2; /* a gap state on a cell outside the band */
    const int len = cap - pos;
    memmove(lr, lr + pos, (size_t)len); lr[len] = 0;
    memmove(lx, lx + pos, (size_t)len); lx[len] = 0;
    memmove(lq, lq + pos, (size_t)len); lq[len] = 0;
    free(h); free(gi); free(gd); free(cell);
    return rc < 0 ? rc : len;
}
