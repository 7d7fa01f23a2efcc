/* lb2_oracle.c -- band-only CPU oracle of banded affine Smith-Waterman (DPX_ALGO_BASW) under two-piece affine gaps, with or without a
 * substitution table, written from the definition in include/dpx_align.h ("A second gap piece for BASW local band-direction
 * batches"), not from the kernels.  TEST INFRASTRUCTURE ONLY: tests/lb2_ref.py builds it with `cc -O2 -shared -fPIC` into a temporary
 * directory.
 *
 * Only the band is kept: two rows of int64 H and of the four gap planes, 2B + 1 cells each, and one byte per in-band cell for the walk and
 * the planes, so the memory is O(m * B) and a 20 000 x 20 300 pair at band 256 is cheap.  A true minus infinity.
 *
 *   cell (i, j), 1 <= i <= m, 1 <= j <= n, is in the band when |i - j| <= B - 1; every neighbour that is a border cell, lies outside the
 *   band or outside the matrix reads H = 0 and D1 = D2 = I1 = I2 = -inf
 *   Dk = max(H[i-1][j] + ok + ek, Dk[i-1][j] + ek), Ik = max(H[i][j-1] + ok + ek, Ik[i][j-1] + ek); GAP_OPEN wins a tie
 *   best = H[i-1][j-1] + s; then D1, D2, I1, I2 in this order: a candidate >= the winner so far takes the cell; H = max(0, winner); the
 *   move is NONE where H == 0
 *   score = max H, end cell = its first cell in row-major order ((0, 0) and 0 when every H is 0)
 *   walk: five states from the end cell in SCORING; SCORING stops on the first cell whose H is 0 (a border cell and a cell outside the
 *   band have H = 0); a gap state emits its column, stays while the cell's own extend bit of its plane is set and returns to SCORING
 *   where that plane opened
 * Byte per in-band cell: bits 0-2 the move (0 none, 1 diagonal, 2 D1, 3 I1, 4 D2, 5 I2), bit 3 I1 extends, bit 4 D1, bit 5 I2, bit 6 D2. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define LB2_NEG_INF (-(1ll << 60))

static long long lb2_add(long long a, long long b) { return a == LB2_NEG_INF ? LB2_NEG_INF : a + b; }

/* scores == NULL: the diagonal term is match / mismatch by byte equality; else scores[codeOf[r] * alphabet + codeOf[q]].
 * lr / lx / lq: m + n + 1 bytes each (NUL-terminated on return).  planes: NULL, or 6 row-major (m + 1) x (n + 1) uint8 planes in the order
 * of dpx_batch_directions' selectors (H, I, D, I2, D2, H_PIECE), 0 on the borders and outside the band.  hOut: NULL, or (m + 1) x (n + 1)
 * int64 that receive H (0 where the definition reads 0: borders and outside the band).  Returns the length of the lines, -1 on a bad
 * argument or a failed allocation, -2 when the walk met what the definition excludes (a gap state on a cell without a code). */
int lb2_align(const unsigned char *ref, int n, const unsigned char *qry, int m, const int8_t *scores, int alphabet, const uint8_t *codeOf,
              int match, int mismatch, int o1, int e1, int o2, int e2, int B, int64_t *score, int32_t *endRow, int32_t *endCol, char *lr,
              char *lx, char *lq, uint8_t *planes, long long *hOut) {
    if (B < 1 || m < 0 || n < 0) return -1;
    if (scores) {
        if (alphabet < 1 || alphabet > 32 || !codeOf) return -1;
        for (int x = 0; x < 256; x++) if (codeOf[x] >= alphabet) return -1;
    }
    const size_t W = 2 * (size_t)B - 1; /* in-band cells of a row: offset k = j - i + B - 1 in 0 .. 2B-2 */
    const size_t RW = W + 2;            /* a row with one cell of slack on either side, which reads H = 0 and -inf */
    long long *buf = malloc(10 * RW * sizeof *buf);
    uint8_t *cell = calloc((size_t)(m > 0 ? m : 1) * W, 1);
    if (!buf || !cell) { free(buf); free(cell); return -1; }
    long long *h = buf, *gp[4]; /* the gap planes in the definition's order D1, D2, I1, I2; two rows each */
    for (int t = 0; t < 4; t++) gp[t] = buf + (size_t)(2 + 2 * t) * RW;
    for (size_t k = 0; k < 2 * RW; k++) { h[k] = 0; for (int t = 0; t < 4; t++) gp[t][k] = LB2_NEG_INF; }
    const size_t full = ((size_t)m + 1) * ((size_t)n + 1), NW = (size_t)n + 1;
    if (planes) memset(planes, 0, 6 * full);
    if (hOut) memset(hOut, 0, full * sizeof *hOut);
    const long long po[4] = {o1, o2, o1, o2}, pe[4] = {e1, e2, e1, e2};
    static const uint8_t moveOf[4] = {2, 4, 3, 5}, bitOf[4] = {16, 64, 8, 32};
    long long best = 0;
    int bi = 0, bj = 0;
    for (int i = 1; i <= m; i++) {
        const size_t cur = (size_t)(i & 1) * RW + 1, prv = (size_t)((i - 1) & 1) * RW + 1;
        for (long long k = -1; k <= (long long)W; k++) { h[cur + k] = 0; for (int t = 0; t < 4; t++) gp[t][cur + k] = LB2_NEG_INF; }
        const int jlo = i - (B - 1) > 1 ? i - (B - 1) : 1, jhi = (long long)i + B - 1 < n ? i + B - 1 : n;
        for (int j = jlo; j <= jhi; j++) {
            const long long k = (long long)j - i + B - 1;
            /* (i-1, j) is offset k + 1 of the previous row, (i-1, j-1) its offset k, (i, j-1) offset k - 1 of this row; the slack cells,
             * row 0 (the previous row is all zeros / -inf when i == 1) and column 0 read H = 0, -inf */
            const int s = scores ? scores[(int)codeOf[ref[j - 1]] * alphabet + (int)codeOf[qry[i - 1]]] : (qry[i - 1] == ref[j - 1] ? match : mismatch);
            long long win = h[prv + k] + s;
            uint8_t c = 1;
            for (int t = 0; t < 4; t++) {
                const int up = t < 2;
                const long long nbH = up ? h[prv + k + 1] : (j == 1 ? 0 : h[cur + k - 1]);
                const long long nbG = up ? gp[t][prv + k + 1] : (j == 1 ? LB2_NEG_INF : gp[t][cur + k - 1]);
                const long long open = nbH + po[t] + pe[t], extd = lb2_add(nbG, pe[t]);
                const long long v = open >= extd ? open : extd; /* GAP_OPEN wins a tie */
                if (!(open >= extd)) c |= bitOf[t];
                gp[t][cur + k] = v;
                if (v >= win) { win = v; c = (uint8_t)((c & ~7) | moveOf[t]); }
            }
            const long long hv = win > 0 ? win : 0;
            if (hv == 0) c &= (uint8_t)~7;
            h[cur + k] = hv;
            cell[(size_t)(i - 1) * W + (size_t)k] = c;
            if (hOut) hOut[(size_t)i * NW + (size_t)j] = hv;
            if (planes) {
                uint8_t *at = planes + (size_t)i * NW + (size_t)j;
                const int mv = c & 7;
                at[0] = mv == 0 ? 0 : (mv == 2 || mv == 4) ? 4 : (mv == 3 || mv == 5) ? 3 : (qry[i - 1] == ref[j - 1] ? 1 : 2);
                at[full] = (c & 8) ? 2 : 1; at[2 * full] = (c & 16) ? 2 : 1; at[3 * full] = (c & 32) ? 2 : 1; at[4 * full] = (c & 64) ? 2 : 1;
                at[5 * full] = (mv == 2 || mv == 3) ? 1 : (mv == 4 || mv == 5) ? 2 : 0;
            }
            if (hv > best) { best = hv; bi = i; bj = j; }
        }
    }
    *score = best;
    *endRow = bi;
    *endCol = bj;
    const int cap = m + n;
    int pos = cap, state = 0, i = bi, j = bj, rc = 0; /* 0 SCORING, else the move number of the gap plane */
    while (i > 0 && j > 0) {
        const int d = i - j;
        if (d > B - 1 || -d > B - 1) { if (state) rc = -2; break; } /* no code: H = 0, the walk stops (it can stand here in SCORING only) */
        const uint8_t c = cell[(size_t)(i - 1) * W + (size_t)(j - i + B - 1)];
        if (state == 0) {
            const int mv = c & 7;
            if (mv == 0) break;
            if (mv == 1) {
                --pos; lr[pos] = (char)ref[j - 1]; lx[pos] = ref[j - 1] == qry[i - 1] ? '*' : '|'; lq[pos] = (char)qry[i - 1];
                i--; j--;
                continue;
            }
            if (mv > 5) { rc = -2; break; }
            state = mv;
        }
        const int left = state == 3 || state == 5;
        const uint8_t bit = state == 3 ? 8 : state == 2 ? 16 : state == 5 ? 32 : 64;
        --pos;
        if (left) { lr[pos] = (char)ref[j - 1]; lq[pos] = '_'; } else { lr[pos] = '_'; lq[pos] = (char)qry[i - 1]; }
        lx[pos] = ' ';
        if (!(c & bit)) state = 0; /* this plane opened here */
        if (left) j--; else i--;
    }
    if (state != 0) rc = -2; /* a gap state that ran onto a border: an edge cell always opens */
    const int len = cap - pos;
    memmove(lr, lr + pos, (size_t)len); lr[len] = 0;
    memmove(lx, lx + pos, (size_t)len); lx[len] = 0;
    memmove(lq, lq + pos, (size_t)len); lq[len] = 0;
    free(buf); free(cell);
    return rc < 0 ? rc : len;
}
