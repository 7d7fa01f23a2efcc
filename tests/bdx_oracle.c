/* bdx_oracle.c -- band-only CPU oracle of BANW / BAXT under a substitution table, with BAXT's extension mode, written from the
 * definitions in include/dpx_align.h (substitution-matrix scoring, BAXT extension mode, their conjunction), not from the kernels.
 * TEST INFRASTRUCTURE ONLY: the test module builds it with `cc -O2 -shared -fPIC` into a temporary directory.
 *
 * tests/zsub_oracle.c keeps (m + 1)(n + 1) cells and cannot run a 33 000 x 33 000 pair.  This one keeps three anti-diagonals of the band:
 * a cell (i, j) of anti-diagonal a = i + j sits at k = i - j + B (1 <= k <= 2B - 1); its upper neighbour is k - 1 and its left
 * neighbour k + 1 on a - 1, its diagonal neighbour k on a - 2.  O((m + n) * B) time, O(B) memory, int64 cells.  It returns the record
 * and the chosen score and end cell, no matrices and no lines; tests/test_bdx_oracle.py checks it against zsub_oracle.c. */
#include <limits.h>
#include <stdint.h>
#include <stdlib.h>

#define BDX_NEG_INF (LLONG_MIN / 4)

static long long bdx_add(long long a, long long b) { return a == BDX_NEG_INF ? BDX_NEG_INF : a + b; }

/* ext = 0: BANW (score = H[m][n], needs |m - n| < B; Z and E must be -1); ext = 1: BAXT, Z / E = -1 off.
 * rec[8] = dpx_extension's fields in order (ext = 0: zeros); chosen[3] = the reported score, end row, end column. */
int bdx_fill(const unsigned char *ref, int n, const unsigned char *qry, int m, const int8_t *scores, int alphabet, const uint8_t *codeOf,
             int o, int e, int B, int ext, int Z, int E, int32_t *rec, int32_t *chosen) {
    if (B < 1 || m < 0 || n < 0 || alphabet < 1 || alphabet > 32 || Z < -1 || E < -1) return -1;
    for (int x = 0; x < 256; x++) if (codeOf[x] >= alphabet) return -1;
    if (!ext && (abs(m - n) >= B || Z >= 0 || E >= 0)) return -2;
    const size_t K = 2 * (size_t)B + 1;
    long long *buf = malloc(7 * K * sizeof *buf);
    if (!buf) return -1;
    long long *h0 = buf, *h1 = buf + K, *h2 = buf + 2 * K, *i0 = buf + 3 * K, *i1 = buf + 4 * K, *d0 = buf + 5 * K, *d1 = buf + 6 * K;
    for (size_t k = 0; k < 7 * K; k++) buf[k] = BDX_NEG_INF;
    h1[B] = 0; /* anti-diagonal 0: (0, 0) */
    const long long pen = e < 0 ? -(long long)e : 0, oe = (long long)o + e;
    long long best = 0, mx = 0, qe = 0, fin = (m == 0 && n == 0) ? 0 : BDX_NEG_INF;
    int bi = 0, bj = 0, mi = 0, mj = 0, qj = m == 0 ? 0 : -1, last = m + n, dropped = 0;
    for (int a = 1; a <= m + n; a++) {
        for (size_t k = 0; k < K; k++) { h0[k] = BDX_NEG_INF; i0[k] = BDX_NEG_INF; d0[k] = BDX_NEG_INF; }
        long long dm = 0;
        int ia = -1, ja = -1;
        const int lo = a > n ? a - n : 0, hi = a < m ? a : m;
        for (int i = lo; i <= hi; i++) { /* ascending rows */
            const int j = a - i, dlt = i - j;
            if (dlt > B - 1 || -dlt > B - 1) continue;
            const int k = dlt + B;
            long long h;
            if (i == 0 || j == 0) {
                h = (long long)o + (long long)a * e;
            } else {
                const long long dOpen = bdx_add(h1[k - 1], oe), dExt = bdx_add(d1[k - 1], e);
                const long long iOpen = bdx_add(h1[k + 1], oe), iExt = bdx_add(i1[k + 1], e);
                d0[k] = dOpen >= dExt ? dOpen : dExt;
                i0[k] = iOpen >= iExt ? iOpen : iExt;
                h = bdx_add(h2[k], scores[(int)codeOf[ref[j - 1]] * alphabet + (int)codeOf[qry[i - 1]]]);
                if (d0[k] >= h) h = d0[k];
                if (i0[k] >= h) h = i0[k];
            }
            h0[k] = h;
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
        t = i1; i1 = i0; i0 = t;
        t = d1; d1 = d0; d0 = t;
        if (dropped) break;
    }
    free(buf);
    for (int k = 0; k < 8; k++) rec[k] = 0;
    if (!ext) {
        chosen[0] = (int32_t)fin; chosen[1] = m; chosen[2] = n;
        return 0;
    }
    const int reached = E >= 0 && !dropped && qj >= 0 && qe + E > mx;
    rec[0] = (int32_t)mx; rec[1] = mi; rec[2] = mj;
    rec[3] = qj >= 0 ? (int32_t)qe : INT32_MIN; rec[4] = qj;
    rec[5] = last; rec[6] = (dropped ? 1 : 0) | (reached ? 2 : 0);
    chosen[0] = reached ? (int32_t)qe : (int32_t)mx;
    chosen[1] = reached ? m : mi;
    chosen[2] = reached ? qj : mj;
    return mx == best ? 0 : -3; /* (maxScore == best always) */
}
