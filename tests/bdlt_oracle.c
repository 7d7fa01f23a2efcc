/* bdlt_oracle.c -- band-only CPU oracle of banded Smith-Waterman with linear gaps (DPX_ALGO_BSW) and affine gaps (DPX_ALGO_BASW) under a
 * substitution table, written from the definition of dpx_batch_set_local_direction_table in include/dpx_align.h, not from the kernels.
 * TEST INFRASTRUCTURE ONLY: bdlt_ref.py builds it with `cc -O2 -shared -fPIC` into a temporary directory.
 *
 * Memory is O((m + n) * B): per row the 2B - 1 in-band cells (offset k = j - i + B - 1), two rows of int64 H, I and D, and one byte per
 * in-band cell for the walk.  Arithmetic is int64 with a true minus infinity.
 *
 *   cell (i, j), 1 <= i <= m, 1 <= j <= n, is in the band when |i - j| <= B - 1; a neighbour that is a border cell or lies outside the
 *   band reads H = 0 (BASW: I = D = -inf)
 *   s(i, j) = scores[codeOf[ref[j-1]] * alphabet + codeOf[qry[i-1]]]: the row is the reference code
 *   BSW:  up = H[i-1][j] + g, left = H[i][j-1] + g, corner = H[i-1][j-1] + s, t = max of the three, H = max(0, t);
 *         dir = NONE (0) iff t < 0, else QUERY_DELETION (4) if up == H, else QUERY_INSERTION (3) if left == H, else MATCH (1) / MISMATCH (2)
 *         by byte equality
 *   BASW: D = max(H[i-1][j] + o + e, D[i-1][j] + e), I = max(H[i][j-1] + o + e, I[i][j-1] + e), GAP_OPEN (1) wins a tie, else GAP_EXTEND (2);
 *         best = H[i-1][j-1] + s (1 / 2 by byte equality); D >= best: 4; then I >= best: 3; H = max(0, best); dirH = NONE where H == 0
 *   score = max H, end cell = its first cell in row-major order ((0, 0) and 0 when every H is 0)
 *   walk: from the end cell in SCORING; stop where H == 0 (a border cell and a cell outside the band have H = 0); BSW follows the cell's
 *         move one step at a time; BASW follows ASW's three states (a gap state leaves on GAP_OPEN); the relation line is byte equality
 * Byte per in-band cell: bits 0-2 dirH, bit 3 H == 0, bits 4-5 dirI, bits 6-7 dirD. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define MINUS_INF (-(1ll << 60))

typedef struct {
    long long *h, *gi, *gd; /* one row: index k + 1 for offset k in -1 .. W (a slack cell on either side) */
} band_row;

static int row_alloc(band_row *r, size_t cells) {
    r->h = malloc(cells * sizeof *r->h);
    r->gi = malloc(cells * sizeof *r->gi);
    r->gd = malloc(cells * sizeof *r->gd);
    return r->h && r->gi && r->gd;
}
static void row_free(band_row *r) { free(r->h); free(r->gi); free(r->gd); }
static void row_reset(band_row *r, size_t cells) {
    for (size_t k = 0; k < cells; k++) { r->h[k] = 0; r->gi[k] = MINUS_INF; r->gd[k] = MINUS_INF; }
}
static long long max2(long long a, long long b) { return a > b ? a : b; }

/* lines of capacity m + n + 1 each (NUL-terminated on return); planes: NULL or three row-major (m+1) x (n+1) uint8 matrices (dirH, dirI,
 * dirD; BSW writes dirH only).  Returns the length of the lines, -1 on a bad argument or failed allocation, -2 if the walk met a cell
 * whose move is NONE while H > 0 or stood in a gap state on a cell without a code (the definition says neither can happen). */
int bdlt_align(const unsigned char *ref, int n, const unsigned char *qry, int m, int affine, const int8_t *scores, int alphabet,
               const uint8_t *codeOf, int o, int e, int B, int64_t *score, int32_t *endRow, int32_t *endCol, char *lr, char *lx, char *lq,
               uint8_t *dirH, uint8_t *dirI, uint8_t *dirD) {
    if (B < 1 || m < 0 || n < 0 || alphabet < 1 || alphabet > 32 || !scores || !codeOf) return -1;
    for (int x = 0; x < 256; x++) if (codeOf[x] >= alphabet) return -1;
    const size_t W = 2 * (size_t)B - 1, cells = W + 2;
    band_row rows[2] = {{0, 0, 0}, {0, 0, 0}};
    uint8_t *cell = calloc((size_t)(m > 0 ? m : 1) * W, 1);
    if (!row_alloc(&rows[0], cells) || !row_alloc(&rows[1], cells) || !cell) { row_free(&rows[0]); row_free(&rows[1]); free(cell); return -1; }
    const size_t stride = (size_t)n + 1, full = ((size_t)m + 1) * stride;
    if (dirH) memset(dirH, 0, full);
    if (dirI) memset(dirI, 0, full);
    if (dirD) memset(dirD, 0, full);
    row_reset(&rows[0], cells); /* row 0: every H is 0 */
    const long long open = affine ? (long long)o + e : (long long)o;
    long long best = 0;
    int bi = 0, bj = 0;
    for (int i = 1; i <= m; i++) {
        band_row *cur = &rows[i & 1], *prev = &rows[(i - 1) & 1];
        row_reset(cur, cells);
        const int qc = codeOf[qry[i - 1]];
        for (int j = (i - (B - 1) > 1 ? i - (B - 1) : 1); j <= n && j - i <= B - 1; j++) {
            const size_t k = (size_t)(j - i + B - 1) + 1; /* this row's index of (i, j); (i-1, j) is k + 1 of the row above, (i-1, j-1) is k */
            const long long s = scores[(int)codeOf[ref[j - 1]] * alphabet + qc];
            const int same = qry[i - 1] == ref[j - 1];
            const long long diag = prev->h[k] + s;
            /* column 0 is a border: H = 0, I = -inf (the slack cell k - 1 holds exactly that when j - 1 is outside the band) */
            const long long leftH = j == 1 ? 0 : cur->h[k - 1], leftI = j == 1 ? MINUS_INF : cur->gi[k - 1];
            const long long upH = prev->h[k + 1], upD = prev->gd[k + 1];
            long long H;
            int mv, di = 0, dd = 0;
            if (affine) {
                const long long dOpen = upH + open, dExt = upD + e, iOpen = leftH + open, iExt = leftI + e;
                const long long D = max2(dOpen, dExt), I = max2(iOpen, iExt);
                dd = dOpen >= dExt ? 1 : 2;
                di = iOpen >= iExt ? 1 : 2;
                cur->gd[k] = D;
                cur->gi[k] = I;
                long long b = diag;
                mv = same ? 1 : 2;
                if (D >= b) { b = D; mv = 4; }
                if (I >= b) { b = I; mv = 3; }
                H = max2(b, 0);
                if (H == 0) mv = 0;
            } else {
                const long long up = upH + open, left = leftH + open;
                const long long t = max2(max2(up, left), diag);
                H = max2(t, 0);
                mv = t < 0 ? 0 : up == H ? 4 : left == H ? 3 : same ? 1 : 2;
            }
            cur->h[k] = H;
            cell[(size_t)(i - 1) * W + (k - 1)] = (uint8_t)(mv | (H == 0 ? 8 : 0) | (di << 4) | (dd << 6));
            if (dirH) dirH[(size_t)i * stride + (size_t)j] = (uint8_t)mv;
            if (affine && dirI) dirI[(size_t)i * stride + (size_t)j] = (uint8_t)di;
            if (affine && dirD) dirD[(size_t)i * stride + (size_t)j] = (uint8_t)dd;
            if (H > best) { best = H; bi = i; bj = j; } /* rows ascending, columns ascending: the first maximum in row-major order */
        }
    }
    *score = best;
    *endRow = bi;
    *endCol = bj;
    const int cap = m + n;
    int pos = cap, state = 0 /* 0 SCORING, 1 INSERTION, 2 DELETION */, i = bi, j = bj, rc = 0;
    while (i > 0 && j > 0) {
        const int d = i - j;
        if (d > B - 1 || -d > B - 1) { if (state != 0) rc = -2; break; } /* outside the band: H = 0 */
        const uint8_t c = cell[(size_t)(i - 1) * W + (size_t)(j - i + B - 1)];
        if (state == 0) {
            if (c & 8) break;
            const int mv = c & 7;
            if (mv == 1 || mv == 2) {
                --pos; lr[pos] = (char)ref[j - 1]; lx[pos] = ref[j - 1] == qry[i - 1] ? '*' : '|'; lq[pos] = (char)qry[i - 1];
                i--; j--;
            } else if (mv == 3) {
                if (affine) state = 1;
                else { --pos; lr[pos] = (char)ref[j - 1]; lx[pos] = ' '; lq[pos] = '_'; j--; }
            } else if (mv == 4) {
                if (affine) state = 2;
                else { --pos; lr[pos] = '_'; lx[pos] = ' '; lq[pos] = (char)qry[i - 1]; i--; }
            } else { rc = -2; break; }
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
    if (state != 0 && rc == 0 && i > 0 && j > 0) rc = -2;
    const int len = cap - pos;
    memmove(lr, lr + pos, (size_t)len); lr[len] = 0;
    memmove(lx, lx + pos, (size_t)len); lx[len] = 0;
    memmove(lq, lq + pos, (size_t)len); lq[len] = 0;
    row_free(&rows[0]); row_free(&rows[1]); free(cell);
    return rc < 0 ? rc : len;
}
