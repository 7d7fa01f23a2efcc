/* zsub_oracle.c -- CPU oracle of DPX_ALGO_BAXT in extension mode under a substitution table (dpx_batch_set_extension_table), written
 * from the definition in include/dpx_align.h ("BAXT extension mode under a substitution table", and the two blocks it joins), not from
 * the kernels.  TEST INFRASTRUCTURE ONLY: the test module builds it with `cc -O2 -shared -fPIC` into a temporary directory.
 *
 * Cells and walk are BAXT's under the table, so this file takes them from subst_oracle.c (subst_fill with ext = 1, subst_walk) and adds
 * what extension mode adds, restated here from the header: the scan over anti-diagonals a = 1 .. m + n with its update-or-drop rule,
 * lastDiag, and the results over the computed cells (in band, i + j <= lastDiag).  Z = E = -1 is accepted (the ABI refuses it): the
 * results are then subst_fill's.  The matrices come back UNMASKED; zsub_ref.py zeroes the exported planes behind lastDiag. */
#include "subst_oracle.c"

#include <limits.h>

/* rec[8] = dpx_extension's fields in order; chosen[3] = the reported score, end row, end column; bestCell[2] = the scan's (bi, bj) */
int zsub_fill(const unsigned char *ref, int n, const unsigned char *qry, int m, const int8_t *scores, int alphabet, const uint8_t *codeOf,
              int o, int e, int B, int Z, int E, int64_t *H, int64_t *I, int64_t *D, uint8_t *dirH, uint8_t *dirI, uint8_t *dirD,
              int32_t *rec, int32_t *chosen, int32_t *bestCell) {
    const size_t W = (size_t)n + 1;
    int64_t sc;
    if (m < 0 || n < 0 || Z < -1 || E < -1) return -1;
    int64_t *own = H ? NULL : malloc(((size_t)m + 1) * W * sizeof *own);
    const int64_t *h = H ? H : own;
    if (!h) return -1;
    if (subst_fill(ref, n, qry, m, scores, alphabet, codeOf, o, e, B, 1, H ? H : own, I, D, dirH, dirI, dirD, &sc, NULL, NULL) != 0) {
        free(own);
        return -1;
    }
    const long long pen = e < 0 ? -(long long)e : 0;
    long long best = 0;
    int bi = 0, bj = 0, last = m + n, dropped = 0;
    for (int a = 1; a <= m + n; a++) {
        long long dm = 0;
        int ia = -1, ja = -1;
        for (int i = a > n ? a - n : 0; i <= m && i <= a; i++) { /* ascending rows: the first maximum is the one with the smallest row */
            const int j = a - i;
            if (!in_band(i, j, B)) continue;
            if (ia < 0 || h[(size_t)i * W + (size_t)j] > dm) { dm = h[(size_t)i * W + (size_t)j]; ia = i; ja = j; }
        }
        if (ia < 0) continue; /* an empty anti-diagonal is skipped */
        if (dm > best) { best = dm; bi = ia; bj = ja; }
        else if (Z >= 0 && ia >= bi && ja >= bj) {
            long long g = (long long)(ia - bi) - (long long)(ja - bj);
            if (g < 0) g = -g;
            if (best - dm > (long long)Z + pen * g) { last = a; dropped = 1; break; }
        }
    }
    /* the first maximum in row-major order over the computed cells, starting from the 0 of (0, 0) */
    long long mx = 0;
    int mi = 0, mj = 0;
    for (int i = 0; i <= m; i++)
        for (int j = 0; j <= n && i + j <= last; j++)
            if (in_band(i, j, B) && h[(size_t)i * W + (size_t)j] > mx) { mx = h[(size_t)i * W + (size_t)j]; mi = i; mj = j; }
    /* row m: the maximum at the smallest column, over its computed in-band cells */
    long long qe = 0;
    int qj = -1;
    for (int j = 0; j <= n && m + j <= last; j++)
        if (in_band(m, j, B) && (qj < 0 || h[(size_t)m * W + (size_t)j] > qe)) { qe = h[(size_t)m * W + (size_t)j]; qj = j; }
    const int reached = E >= 0 && !dropped && qj >= 0 && qe + E > mx;
    rec[0] = (int32_t)mx; rec[1] = mi; rec[2] = mj;
    rec[3] = qj >= 0 ? (int32_t)qe : INT32_MIN; rec[4] = qj;
    rec[5] = last; rec[6] = (dropped ? 1 : 0) | (reached ? 2 : 0); rec[7] = 0;
    chosen[0] = reached ? (int32_t)qe : (int32_t)mx;
    chosen[1] = reached ? m : mi;
    chosen[2] = reached ? qj : mj;
    if (bestCell) { bestCell[0] = bi; bestCell[1] = bj; }
    free(own);
    return mx == best ? 0 : -2; /* (maxScore == best always) */
}
