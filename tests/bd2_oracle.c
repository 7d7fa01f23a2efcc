/* bd2_oracle.c -- band-only CPU oracle of BANW / BAXT under two-piece affine gaps, with a substitution table and BAXT's extension mode,
 * written from the definition in include/dpx_align.h ("Two-piece affine gaps"), not from the kernels.
 * TEST INFRASTRUCTURE ONLY: tests/bd2_ref.py builds it with `cc -O2 -shared -fPIC` into a temporary directory.
 *
 * Scores: three anti-diagonals of the band in int64, as tests/bdx_oracle.c keeps them: a cell (i, j) of anti-diagonal a = i + j sits at
 * k = i - j + B (1 <= k <= 2B - 1); its upper neighbour is k - 1 and its left neighbour k + 1 on a - 1, its diagonal neighbour k on a - 2.
 * Choices: one byte per in-band cell with i, j >= 1 in a (m + 1) x (2B + 1) array -- bits 0-2 the winner (1 diagonal, 2 D1, 3 I1, 4 D2,
 * 5 I2), bit 3 I1 extends, bit 4 D1, bit 5 I2, bit 6 D2 -- from which the walk and the six exported planes are read.  O((m + n) * B) time,
 * O(m * B) memory: a 20 000 x 20 300 pair at band 256 takes 10 MB. */
#include <limits.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define BD2_NEG_INF (LLONG_MIN / 4)

static long long bd2_add(long long a, long long b) { return a == BD2_NEG_INF ? BD2_NEG_INF : a + b; }
static long long bd2_gap(long long k, int o1, int e1, int o2, int e2) {
    const long long a = o1 + k * e1, b = o2 + k * e2;
    return a >= b ? a : b;
}

/* ext = 0: BANW (score = H[m][n], needs |m - n| < B; Z and E must be -1); ext = 1: BAXT, Z / E = -1 off.
 * rec[8] = dpx_extension's fields in order (ext = 0: zeros); chosen[3] = the reported score, end row, end column.
 * planes: NULL, or 6 row-major (m + 1) x (n + 1) uint8 planes in the order of dpx_batch_directions' selectors (H, I, D, I2, D2, H_PIECE),
 * every plane 0 where i + j > lastDiag.  lr / lx / lq: NULL, or m + n + 1 bytes each for the three lines; *len receives their length
 * (-1: the walk left the stored cells, which cannot happen).  hOut: NULL, or (m + 1) x (n + 1) int64 that receive H (LLONG_MIN / 4 where
 * no cell was computed). */
int bd2_fill(const unsigned char *ref, int n, const unsigned char *qry, int m, const int8_t *scores, int alphabet, const uint8_t *codeOf,
             int o1, int e1, int o2, int e2, int B, int ext, int Z, int E, int32_t *rec, int32_t *chosen, uint8_t *planes, char *lr, char *lx,
             char *lq, int32_t *len, long long *hOut) {
    if (B < 1 || m < 0 || n < 0 || alphabet < 1 || alphabet > 32 || Z < -1 || E < -1) return -1;
    for (int x = 0; x < 256; x++) if (codeOf[x] >= alphabet) return -1;
    if (!ext && (abs(m - n) >= B || Z >= 0 || E >= 0)) return -2;
    const size_t K = 2 * (size_t)B + 1;
    long long *buf = malloc(15 * K * sizeof *buf);
    uint8_t *code = calloc(((size_t)m + 1) * K, 1);
    if (!buf || !code) { free(buf); free(code); return -1; }
    long long *h0 = buf, *h1 = buf + K, *h2 = buf + 2 * K;
    long long *g0[4], *g1[4]; /* the gap planes in the definition's order D1, D2, I1, I2: this anti-diagonal and the one before */
    for (int t = 0; t < 4; t++) { g0[t] = buf + (3 + 2 * t) * K; g1[t] = buf + (4 + 2 * t) * K; }
    for (size_t k = 0; k < 15 * K; k++) buf[k] = BD2_NEG_INF;
    h1[B] = 0; /* anti-diagonal 0: (0, 0) */
    if (hOut) { for (size_t x = 0; x < ((size_t)m + 1) * ((size_t)n + 1); x++) hOut[x] = BD2_NEG_INF; hOut[0] = 0; }
    const int po[4] = {o1, o2, o1, o2}, pe[4] = {e1, e2, e1, e2};
    const int flat = e1 >= e2 ? e1 : e2;
    const long long pen = flat < 0 ? -(long long)flat : 0;
    static const uint8_t moveOf[4] = {2, 4, 3, 5}, bitOf[4] = {16, 64, 8, 32};
    long long best = 0, mx = 0, qe = 0, fin = (m == 0 && n == 0) ? 0 : BD2_NEG_INF;
    int bi = 0, bj = 0, mi = 0, mj = 0, qj = m == 0 ? 0 : -1, last = m + n, dropped = 0;
    for (int a = 1; a <= m + n; a++) {
        for (size_t k = 0; k < K; k++) { h0[k] = BD2_NEG_INF; for (int t = 0; t < 4; t++) g0[t][k] = BD2_NEG_INF; }
        long long dm = 0;
        int ia = -1, ja = -1;
        const int lo = a > n ? a - n : 0, hi = a < m ? a : m;
        for (int i = lo; i <= hi; i++) { /* ascending rows */
            const int j = a - i, dlt = i - j;
            if (dlt > B - 1 || -dlt > B - 1) continue;
            const int k = dlt + B;
            long long h;
            if (i == 0 || j == 0) {
                h = bd2_gap(a, o1, e1, o2, e2);
            } else {
                uint8_t c = 1;
                h = bd2_add(h2[k], scores[(int)codeOf[ref[j - 1]] * alphabet + (int)codeOf[qry[i - 1]]]);
                for (int t = 0; t < 4; t++) {
                    const int nb = t < 2 ? k - 1 : k + 1; /* D: the upper neighbour, I: the left one */
                    const long long open = bd2_add(h1[nb], (long long)po[t] + pe[t]), extd = bd2_add(g1[t][nb], pe[t]);
                    g0[t][k] = open >= extd ? open : extd; /* GAP_OPEN wins a tie */
                    if (!(open >= extd)) c |= bitOf[t];
                    if (g0[t][k] >= h) { h = g0[t][k]; c = (uint8_t)((c & ~7) | moveOf[t]); }
                }
                code[(size_t)i * K + (size_t)k] = c;
            }
            h0[k] = h;
            if (hOut) hOut[(size_t)i * ((size_t)n + 1) + (size_t)j] = h;
            if (ia < 0 || h > dm) { dm = h; ia = i; ja = j; }
            /* the first maximum in row-major order: a later anti-diagonal can hold an earlier cell of the same score */
            if (h > mx || (h == mx && mx > 0 && (i < mi || (i == mi && j < mj)))) { mx = h; mi = i; mj = j; }
            if (i == m && (qj < 0 || h > qe)) { qe = h; qj = j; } /* row m's cells arrive in column order */
            if (i == m && j == n) fin = h;
        }
        if (ia >= 0) {
            if (dm > best) { best = dm; bi = ia; bj = ja; }
            else if (Z >= 0 && ia >= bi && ja >= bj) {
                long long g = (long long)(ia - bi) - (long long)(ja - bj);
                if (g < 0) g = -g;
                if (best - dm > (long long)Z + pen * g) { last = a; dropped = 1; }
            }
        }
        long long *t = h2; h2 = h1; h1 = h0; h0 = t;
        for (int q = 0; q < 4; q++) { t = g1[q]; g1[q] = g0[q]; g0[q] = t; }
        if (dropped) break;
    }
    free(buf);
    for (int k = 0; k < 8; k++) rec[k] = 0;
    if (!ext) {
        chosen[0] = (int32_t)fin; chosen[1] = m; chosen[2] = n;
    } else {
        const int reached = E >= 0 && !dropped && qj >= 0 && qe + E > mx;
        rec[0] = (int32_t)mx; rec[1] = mi; rec[2] = mj;
        rec[3] = qj >= 0 ? (int32_t)qe : INT32_MIN; rec[4] = qj;
        rec[5] = last; rec[6] = (dropped ? 1 : 0) | (reached ? 2 : 0);
        chosen[0] = reached ? (int32_t)qe : (int32_t)mx;
        chosen[1] = reached ? m : mi;
        chosen[2] = reached ? qj : mj;
    }
    if (planes) {
        const size_t W = (size_t)n + 1, P = ((size_t)m + 1) * W;
        memset(planes, 0, 6 * P);
        for (int i = 0; i <= m; i++)
            for (int j = 0; j <= n; j++) {
                if (abs(i - j) > B - 1 || i + j > last) continue;
                uint8_t *at = planes + (size_t)i * W + (size_t)j;
                if (i == 0 || j == 0) { at[0] = (i | j) == 0 ? 0 : j == 0 ? 4 : 3; continue; } /* ANW's borders in H, 0 elsewhere */
                const uint8_t c = code[(size_t)i * K + (size_t)(i - j + B)], mv = c & 7;
                at[0] = (mv == 2 || mv == 4) ? 4 : (mv == 3 || mv == 5) ? 3 : (qry[i - 1] == ref[j - 1] ? 1 : 2);
                at[P] = (c & 8) ? 2 : 1; at[2 * P] = (c & 16) ? 2 : 1; at[3 * P] = (c & 32) ? 2 : 1; at[4 * P] = (c & 64) ? 2 : 1;
                at[5 * P] = (mv == 2 || mv == 3) ? 1 : (mv == 4 || mv == 5) ? 2 : 0;
            }
    }
    if (lr && lx && lq && len) { /* the walk: five states, then ANW's two tails; written backwards, then turned round */
        int i = chosen[1], j = chosen[2], state = 0, k = 0, ok = 1;
        while (i > 0 && j > 0) {
            if (abs(i - j) > B - 1 || i + j > last) { ok = 0; break; }
            const uint8_t c = code[(size_t)i * K + (size_t)(i - j + B)];
            if (state == 0) {
                const int mv = c & 7;
                if (mv == 1) {
                    lr[k] = (char)ref[j - 1]; lq[k] = (char)qry[i - 1]; lx[k] = ref[j - 1] == qry[i - 1] ? '*' : '|';
                    k++; i--; j--;
                    continue;
                }
                if (mv < 2 || mv > 5) { ok = 0; break; }
                state = mv;
            }
            const int left = state == 3 || state == 5;
            const uint8_t bit = state == 3 ? 8 : state == 2 ? 16 : state == 5 ? 32 : 64;
            if (left) { lr[k] = (char)ref[j - 1]; lq[k] = '_'; } else { lr[k] = '_'; lq[k] = (char)qry[i - 1]; }
            lx[k] = ' ';
            k++;
            if (!(c & bit)) state = 0; /* this plane opened here */
            if (left) j--; else i--;
        }
        for (; i > 0; i--, k++) { lr[k] = '_'; lx[k] = ' '; lq[k] = (char)qry[i - 1]; }
        for (; j > 0; j--, k++) { lr[k] = (char)ref[j - 1]; lx[k] = ' '; lq[k] = '_'; }
        for (int x = 0; x < k / 2; x++) {
            char t;
            t = lr[x]; lr[x] = lr[k - 1 - x]; lr[k - 1 - x] = t;
            t = lx[x]; lx[x] = lx[k - 1 - x]; lx[k - 1 - x] = t;
            t = lq[x]; lq[x] = lq[k - 1 - x]; lq[k - 1 - x] = t;
        }
        *len = ok ? k : -1;
    }
    free(code);
    return (!ext || mx == best) ? 0 : -3; /* (maxScore == best always) */
}
