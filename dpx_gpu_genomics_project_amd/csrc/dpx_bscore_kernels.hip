/*
 * dpx_bscore_kernels.hip -- DPX_LONG_SCORES on a band-direction batch of BANW / BAXT (DPX_KEEP_BAND_DIRECTIONS | DPX_LONG_SCORES) for
 * gfx950: the fill, k_bscore_fill<C, PB, EXT, TABLE, SCAN>, and nothing else.  There is no pool, no walk and no export: the kernel writes
 * the results (and, with the scan on, the dpx_extension records) and nothing more.
 *
 * The cells are k_bdir_fill's / k_bdx_fill's, value for value: int32 registers, the 2^28 range check, no n or m + n limit, the strings
 * staged in LDS and, TABLE, the 1280-byte table image behind them.  Everything outside the step is the shared frame,
 * dpx_banddir_fill.inc, included below under DPX_BANDDIR_SCORE_ONLY: the window, the pair's place in the pool, the 16-byte store per
 * group of steps and the partial last group are not compiled there, and a dropped pair (SCAN == 2) simply ends.  The scan after a step
 * (DPX_BANDDIR_SCAN_AFTER), zdrop_test, write_results and scan_border_line are the shared ones.
 *
 * The step, bscore_step, is this unit's own (one step per unit: profiles/band_sharing_ab.md, profiles/banddir_sharing_ab.md).  It is
 * bdx_step's recurrence, line for line in the same order -- the neighbour pick-up, the diagonal terms, D, I, H, the validity and
 * border selects, fin and the tracker key -- written without what only the codes needed: the four sign-bit tests (iLoses, dLoses,
 * iExtends, dExtends), the step's word and the 128-bit window.  Every H, I and D it hands on is the value the storing twin computes.
 *
 * Modes: EXT = 0 (BANW) takes SCAN = 0 with TABLE 0 / 1; EXT = 1 (BAXT) every (TABLE, SCAN), (0, 0) included -- there is no plain twin
 * to defer to.  8 modes x 4 C x 2 parities = 64 kernels.
 */
#define DPX_BANDDIR_SCORE_ONLY 1
#include "dpx_banddir_dev.hpp"

namespace {

using namespace dpx_band;

template <int C>
struct BscoreState {
    int prevH[C], prev2H[C]; /* H on anti-diagonals a-1 and a-2 */
    int prevI[C], prevD[C];  /* I and D on anti-diagonal a-1 */
    int qch[C], rch[C];      /* query / reference character of each slot's cell (TABLE: query code / reference code << 5) */
    long long bestKey;       /* EXT: the lane's running maximum of (H << 32 | ~row), signed: the highest H, then the smallest row ... */
    int bestA;               /* ... and the step of its first occurrence (the smallest column of that row) */
    int lim;                 /* B-1 - lane*C: slot c is inside the band on a step of parity p when c + p <= lim */
    int fin;                 /* !EXT: H[m][n], picked up on the last anti-diagonal by the lane that owns its slot */
    __device__ __forceinline__ void clear_gaps(const int c) { prevI[c] = DPX_NEG; prevD[c] = DPX_NEG; }
};

/* one anti-diagonal: bdx_step without the codes.  INTERIOR: every in-band slot lies inside the matrix, so validity is one compare against
 * the per-lane constant `lim`; no border slot and not the last anti-diagonal */
template <int C, bool EXT, bool TABLE, bool P1, bool INTERIOR>
__device__ __forceinline__ void bscore_step(BscoreState<C> &st, const int A, int &i0, int &j0, const int lane, const int m, const int n,
                                            const int B, [[maybe_unused]] const int match, [[maybe_unused]] const int mismatch, const int o,
                                            const int oe, const int e, const int cEnd, const unsigned char *qL, const unsigned char *rL,
                                            [[maybe_unused]] const signed char *tabL, [[maybe_unused]] const unsigned char *codeL) {
    const int p = P1 ? 1 : 0;
    if constexpr (P1) i0++; else j0++;
    const int smin = INTERIOR ? 0 : max(max(1 - i0, j0 - n), 0);
    const int smax = INTERIOR ? 0 : min(min(m - i0, j0 - 1), B - 1 - p);
    /* the in-band border cells of this anti-diagonal: (0, a) in slot -i0 and (a, 0) in slot j0, both H = o + a * e, while a <= B-1 */
    const int a = A + 2;
    const int bord = (INTERIOR || a > B - 1) ? DPX_NEG : o + a * e;
    const int sTop = (INTERIOR || a > n) ? -1 : -i0, sLeft = (INTERIOR || a > m) ? -1 : j0;
    const int lo = smin - lane * C, cnt = max(smax - smin + 1, 0), cTop = sTop - lane * C, cLeft = sLeft - lane * C;
    const bool last = !INTERIOR && a == m + n;
    int upH[C], upD[C], leftH[C], leftI[C];
    if constexpr (P1) {
        int newq = INTERIOR ? qL[i0 + 64 * C - 2] : qL[min(max(i0 + 64 * C - 2, 0), m - 1)];
        if constexpr (TABLE) newq = codeL[newq];
        const int tq = wave_shl1(st.qch[0], newq);
#pragma unroll
        for (int c = 0; c < C - 1; c++) st.qch[c] = st.qch[c + 1];
        st.qch[C - 1] = tq;
        const int nbH = wave_shl1(st.prevH[0], DPX_NEG);
        const int nbI = wave_shl1(st.prevI[0], DPX_NEG);
#pragma unroll
        for (int c = 0; c < C; c++) {
            upH[c] = st.prevH[c];
            upD[c] = st.prevD[c];
            leftH[c] = (c < C - 1) ? st.prevH[c + 1] : nbH;
            leftI[c] = (c < C - 1) ? st.prevI[c + 1] : nbI;
        }
    } else {
        int newr = INTERIOR ? rL[j0 - 1] : rL[min(max(j0 - 1, 0), n - 1)];
        if constexpr (TABLE) newr = (int)codeL[newr] << 5;
        const int tr = wave_shr1(st.rch[C - 1], newr);
#pragma unroll
        for (int c = C - 1; c > 0; c--) st.rch[c] = st.rch[c - 1];
        st.rch[0] = tr;
        const int nbH = wave_shr1(st.prevH[C - 1], DPX_NEG);
        const int nbD = wave_shr1(st.prevD[C - 1], DPX_NEG);
#pragma unroll
        for (int c = 0; c < C; c++) {
            leftH[c] = st.prevH[c];
            leftI[c] = st.prevI[c];
            upH[c] = (c > 0) ? st.prevH[c - 1] : nbH;
            upD[c] = (c > 0) ? st.prevD[c - 1] : nbD;
        }
    }
    int sc[C]; /* TABLE: all C byte reads are in flight before the first is used (codes are < 32: the address stays inside the 1-KiB table) */
#pragma unroll
    for (int c = 0; c < C; c++) {
        if constexpr (TABLE) sc[c] = (int)tabL[st.rch[c] + st.qch[c]];
        else sc[c] = (st.qch[c] == st.rch[c]) ? match : mismatch;
    }
    const int nrow0 = ~(i0 + lane * C); /* ~row of slot c is nrow0 - c (a border slot decodes to row 0 or column 0) */
#pragma unroll
    for (int cc = 0; cc < C; cc++) {
        /* a p = 0 step reads its upper neighbour from slot c - 1: going down the slots there, every slot is read before it is replaced */
        const int c = P1 ? cc : C - 1 - cc;
        const int dOpen = upH[c] + oe, dExt = upD[c] + e;
        const int iOpen = leftH[c] + oe, iExt = leftI[c] + e;
        int d = max(dOpen, dExt);
        int ii = max(iOpen, iExt);
        const int dg = st.prev2H[c] + sc[c];
        const int top = max(d, dg);
        int h = max(ii, top); /* (no floor; the diagonal neighbour of an in-band cell is in band, so h is finite) */
        if constexpr (INTERIOR) {
            const bool valid = (c + p) <= st.lim;
            h = valid ? h : DPX_NEG;
            d = valid ? d : DPX_NEG;
            ii = valid ? ii : DPX_NEG;
        } else {
            /* slot lane * C + c against the step's window [smin, smax] and its two border slots (cnt = 0 when the window is empty) */
            const bool valid = (unsigned)(c - lo) < (unsigned)cnt;
            h = valid ? h : ((c == cTop || c == cLeft) ? bord : DPX_NEG);
            d = valid ? d : DPX_NEG;
            ii = valid ? ii : DPX_NEG;
            if constexpr (!EXT) st.fin = (last && c == cEnd) ? h : st.fin;
        }
        if constexpr (EXT) { /* (after the border select: border cells take part) */
            const long long key = (long long)(((unsigned long long)(unsigned)h << 32) | (unsigned long long)(unsigned)(nrow0 - c));
            const bool up = key > st.bestKey; /* (an equal key is the same row on a later step, a larger column: it stays) */
            st.bestKey = up ? key : st.bestKey;
            st.bestA = up ? A : st.bestA;
        }
        st.prev2H[c] = st.prevH[c];
        st.prevH[c] = h;
        st.prevI[c] = ii;
        st.prevD[c] = d;
    }
}

template <int C, bool PB, bool EXT, bool TABLE, int SCAN>
__global__ void __launch_bounds__(DPX_FILL_THREADS) k_bscore_fill(const dpx_bdx_args x) {
    static_assert(EXT || SCAN == 0, "BANW has no extension mode");
    const dpx_fill_args &a = x.f;
    using State = BscoreState<C>;
    /* the wave-uniform row-m pick-up in both scan modes (dpx_banddir_dev.hpp, "Scalar registers": two forms of one function of the same
     * values).  Without the window it costs no scratch at C = 8 in either mode, and the per-lane form left <8, 1, 1, 1, 1> one VGPR above
     * its storing twin (128 against 127); tests/test_bscore_kernels_isa.py holds all 64 to zero scratch and to their twins' counts */
    [[maybe_unused]] constexpr bool kPickUniform = SCAN > 0;
    /* (the border line is linear in k: its first maximum is at k = L when e > 0 and at k = 1 otherwise) */
#define DPX_BANDDIR_WEIGHTS                                                                                              \
    const int match = a.match, mismatch = a.mismatch, o = a.gapOpen, e = a.gapExtend, oe = a.gapOpen + a.gapExtend;      \
    [[maybe_unused]] const int Z = x.scan.zdrop, pen = e < 0 ? -e : 0;                                                   \
    const int bord1 = oe;                                                                                                \
    auto bord = [o, e](const int k) -> int { return o + k * e; };                                                        \
    auto line_first_max = [e](const int L) -> int { return e > 0 ? L : min(L, 1); };
#define DPX_BANDDIR_NO_CELL_H DPX_NEG
#define DPX_BANDDIR_STEP(P1_, INTERIOR_, A_) \
    bscore_step<C, EXT, TABLE, P1_, INTERIOR_>(st, A_, i0, j0, lane, m, n, B, match, mismatch, o, oe, e, cEnd, qL, rL, tabL, codeL)
#include "dpx_banddir_fill.inc"
#undef DPX_BANDDIR_STEP
#undef DPX_BANDDIR_NO_CELL_H
#undef DPX_BANDDIR_WEIGHTS
}

} // namespace

hipError_t dpx_launch_bscore_fill(const dpx_bdx_args &x, int C, bool ext, hipStream_t stream) {
    if (x.f.numPairs <= 0) return hipSuccess;
    const bool table = x.tab.table != nullptr;
    const int scan = !ext ? 0 : x.scan.zdrop >= 0 ? 2 : x.scan.endBonus >= 0 ? 1 : 0;
    if ((table && !x.tab.codeOf) || (scan && !x.scan.ext)) return hipErrorInvalidValue;
    return dispatch_fill(C, x.f.band, table, [&](auto c, auto pb, auto tb) {
        constexpr int kC = decltype(c)::value;
        constexpr bool kPB = decltype(pb)::value, kTable = decltype(tb)::value;
        if (!ext) return launch_banddir_fill(k_bscore_fill<kC, kPB, false, kTable, 0>, x, x.f, stream);
        if (scan == 2) return launch_banddir_fill(k_bscore_fill<kC, kPB, true, kTable, 2>, x, x.f, stream);
        if (scan == 1) return launch_banddir_fill(k_bscore_fill<kC, kPB, true, kTable, 1>, x, x.f, stream);
        return launch_banddir_fill(k_bscore_fill<kC, kPB, true, kTable, 0>, x, x.f, stream);
    });
}
