/*
 * dpx_lscore_kernels.hip -- DPX_LONG_SCORES on a local band-direction batch of BSW / BASW (DPX_KEEP_LOCAL_BAND_DIRECTIONS |
 * DPX_LONG_SCORES) for gfx950: the fill, k_lscore_fill<C, PB, AFFINE, TABLE>, and nothing else.  There is no pool, no walk and no
 * export: the kernel writes score, end row and end column and nothing more.
 *
 * The cells are k_bdl_fill's / k_bdlt_fill's, value for value: the band |i-j| <= B-1 of the cells with i, j >= 1 in int32 registers, a
 * zero floor, every neighbour without a cell reads H = 0 (BASW: I = D = DPX_NEG), BSW's linear form under AFFINE = false, the 2^28 range
 * check, no m + n limit, the strings staged in LDS and, TABLE, the 1280-byte table image behind them.  Everything outside the step is the
 * shared frame, dpx_banddir_fill.inc, in its EXT form with no scan, included below under DPX_BANDDIR_SCORE_ONLY: the window, the pair's
 * place in the pool, the 16-byte store per group of steps and the partial last group are not compiled there.
 *
 * The step, lscore_step, is this unit's own (one step per unit: profiles/band_sharing_ab.md, profiles/banddir_sharing_ab.md).  It is
 * bdl_step's recurrence (dpx_bdl_dev.hpp), line for line in the same order, written without what only the codes needed: the sign-bit
 * tests, the code, the step's word and the 128-bit window.  Every H, I and D it hands on and every tracker key is the value the storing
 * twin computes, so the end cell is the same first maximum in row-major order; only H > 0 displaces (0, 0).
 *
 * 4 C x 2 parities x linear / affine x byte compare / table = 32 kernels.
 */
#define DPX_BANDDIR_SCORE_ONLY 1
#include "dpx_banddir_dev.hpp"

namespace {

using namespace dpx_band;

template <int C, bool AFFINE>
struct LscoreState {
    int prevH[C], prev2H[C];                          /* H on anti-diagonals a-1 and a-2 */
    int prevI[AFFINE ? C : 1], prevD[AFFINE ? C : 1]; /* BASW: I and D on anti-diagonal a-1 (BSW has no gap planes) */
    int qch[C], rch[C];                               /* query / reference character of each slot's cell (TABLE: query code / reference code << 5) */
    long long bestKey;                                /* the lane's running maximum of (H << 32 | ~row), signed: the highest H, then the smallest row ... */
    int bestA;                                        /* ... and the step of its first occurrence (the smallest column of that row) */
    int lim;                                          /* B-1 - lane*C: slot c is inside the band on a step of parity p when c + p <= lim */
    int fin;                                          /* (the frame's; not used: the end cell is the tracker's) */
    __device__ __forceinline__ void clear_gaps(const int c) {
        if constexpr (AFFINE) { prevI[c] = DPX_NEG; prevD[c] = DPX_NEG; }
    }
};

/* one anti-diagonal: bdl_step without the codes.  INTERIOR: every in-band slot lies inside the matrix, so validity is one compare against
 * the per-lane constant `lim`.  g: BSW's gap weight, BASW's gapOpen + gapExtend; e: BASW's gapExtend */
template <int C, bool AFFINE, bool TABLE, bool P1, bool INTERIOR>
__device__ __forceinline__ void lscore_step(LscoreState<C, AFFINE> &st, const int A, int &i0, int &j0, const int lane, const int m, const int n,
                                            const int B, [[maybe_unused]] const int match, [[maybe_unused]] const int mismatch, const int g,
                                            [[maybe_unused]] const int e, const unsigned char *qL, const unsigned char *rL,
                                            [[maybe_unused]] const signed char *tabL, [[maybe_unused]] const unsigned char *codeL) {
    const int p = P1 ? 1 : 0;
    if constexpr (P1) i0++; else j0++;
    const int smin = INTERIOR ? 0 : max(max(1 - i0, j0 - n), 0);
    const int smax = INTERIOR ? 0 : min(min(m - i0, j0 - 1), B - 1 - p);
    const int lo = smin - lane * C, cnt = max(smax - smin + 1, 0);
    constexpr int CG = AFFINE ? C : 1;
    int upH[C], leftH[C];
    [[maybe_unused]] int upD[CG], leftI[CG];
    if constexpr (P1) {
        int newq = INTERIOR ? qL[i0 + 64 * C - 2] : qL[min(max(i0 + 64 * C - 2, 0), m - 1)];
        if constexpr (TABLE) newq = codeL[newq];
        const int tq = wave_shl1(st.qch[0], newq);
#pragma unroll
        for (int c = 0; c < C - 1; c++) st.qch[c] = st.qch[c + 1];
        st.qch[C - 1] = tq;
        const int nbH = wave_shl1(st.prevH[0], 0); /* (the last lane has no neighbour: a cell outside the band, H = 0) */
        [[maybe_unused]] int nbI = 0;
        if constexpr (AFFINE) nbI = wave_shl1(st.prevI[0], DPX_NEG);
#pragma unroll
        for (int c = 0; c < C; c++) {
            upH[c] = st.prevH[c];
            leftH[c] = (c < C - 1) ? st.prevH[c + 1] : nbH;
            if constexpr (AFFINE) {
                upD[c] = st.prevD[c];
                leftI[c] = (c < C - 1) ? st.prevI[c + 1] : nbI;
            }
        }
    } else {
        int newr = INTERIOR ? rL[j0 - 1] : rL[min(max(j0 - 1, 0), n - 1)];
        if constexpr (TABLE) newr = (int)codeL[newr] << 5;
        const int tr = wave_shr1(st.rch[C - 1], newr);
#pragma unroll
        for (int c = C - 1; c > 0; c--) st.rch[c] = st.rch[c - 1];
        st.rch[0] = tr;
        const int nbH = wave_shr1(st.prevH[C - 1], 0);
        [[maybe_unused]] int nbD = 0;
        if constexpr (AFFINE) nbD = wave_shr1(st.prevD[C - 1], DPX_NEG);
#pragma unroll
        for (int c = 0; c < C; c++) {
            leftH[c] = st.prevH[c];
            upH[c] = (c > 0) ? st.prevH[c - 1] : nbH;
            if constexpr (AFFINE) {
                leftI[c] = st.prevI[c];
                upD[c] = (c > 0) ? st.prevD[c - 1] : nbD;
            }
        }
    }
    /* TABLE: all C byte reads are in flight before the first is used (codes are < 32: the address stays inside the 1-KiB table) */
    [[maybe_unused]] int tsc[TABLE ? C : 1];
    if constexpr (TABLE) {
#pragma unroll
        for (int c = 0; c < C; c++) tsc[c] = (int)tabL[st.rch[c] + st.qch[c]];
    }
    const int nrow0 = ~(i0 + lane * C); /* ~row of slot c is nrow0 - c */
#pragma unroll
    for (int cc = 0; cc < C; cc++) {
        /* a p = 0 step reads its upper neighbour from slot c - 1: going down the slots there, every slot is read before it is replaced */
        const int c = P1 ? cc : C - 1 - cc;
        int sc;
        if constexpr (TABLE) sc = tsc[c];
        else sc = (st.qch[c] == st.rch[c]) ? match : mismatch;
        const int dg = st.prev2H[c] + sc;
        [[maybe_unused]] int d = 0, ii = 0;
        int h;
        if constexpr (AFFINE) {
            const int dOpen = upH[c] + g, dExt = upD[c] + e;
            const int iOpen = leftH[c] + g, iExt = leftI[c] + e;
            d = max(dOpen, dExt);
            ii = max(iOpen, iExt);
            const int top = max(d, dg);
            h = max(max(ii, top), 0);
        } else {
            const int up = upH[c] + g, left = leftH[c] + g;
            const int lc = max(left, dg);
            const int t = max(up, lc);
            h = max(t, 0);
        }
        /* a slot without a cell hands on what its neighbours must read there: H = 0, I = D = minus infinity */
        const bool valid = INTERIOR ? (c + p) <= st.lim : (unsigned)(c - lo) < (unsigned)cnt;
        h = valid ? h : 0;
        {
            const long long key = (long long)(((unsigned long long)(unsigned)h << 32) | (unsigned long long)(unsigned)(nrow0 - c));
            const bool up = key > st.bestKey; /* (an equal key is the same row on a later step, a larger column: it stays) */
            st.bestKey = up ? key : st.bestKey;
            st.bestA = up ? A : st.bestA;
        }
        st.prev2H[c] = st.prevH[c];
        st.prevH[c] = h;
        if constexpr (AFFINE) {
            st.prevI[c] = valid ? ii : DPX_NEG;
            st.prevD[c] = valid ? d : DPX_NEG;
        }
    }
}

template <int C, bool PB, bool AFFINE, bool TABLE>
__global__ void __launch_bounds__(DPX_FILL_THREADS) k_lscore_fill(const dpx_bdx_args x) { /* (the frame's argument block: x.f and, TABLE, x.tab are read; x.scan is off) */
    constexpr bool EXT = true;
    constexpr int SCAN = 0;
    const dpx_fill_args &a = x.f;
    using State = LscoreState<C, AFFINE>;
    [[maybe_unused]] constexpr bool kPickUniform = false;
    /* (every border cell is 0: the border line of an empty sequence never displaces the 0 of (0, 0)) */
#define DPX_BANDDIR_WEIGHTS                                                                                              \
    [[maybe_unused]] const int match = a.match, mismatch = a.mismatch;                                                   \
    const int e = a.gapExtend, g = AFFINE ? a.gapOpen + a.gapExtend : a.gapOpen;                                         \
    [[maybe_unused]] const int Z = -1, pen = 0;                                                                          \
    const int bord1 = 0;                                                                                                 \
    auto bord = [](const int) -> int { return 0; };                                                                      \
    auto line_first_max = [](const int L) -> int { return min(L, 1); };
#define DPX_BANDDIR_NO_CELL_H 0
#define DPX_BANDDIR_STEP(P1_, INTERIOR_, A_) \
    lscore_step<C, AFFINE, TABLE, P1_, INTERIOR_>(st, A_, i0, j0, lane, m, n, B, match, mismatch, g, e, qL, rL, tabL, codeL)
#include "dpx_banddir_fill.inc"
#undef DPX_BANDDIR_STEP
#undef DPX_BANDDIR_NO_CELL_H
#undef DPX_BANDDIR_WEIGHTS
}

} // namespace

hipError_t dpx_launch_lscore_fill(const dpx_bdx_args &x, int C, bool affine, hipStream_t stream) {
    if (x.f.numPairs <= 0) return hipSuccess;
    const bool table = x.tab.table != nullptr;
    if (table && !x.tab.codeOf) return hipErrorInvalidValue;
    return dispatch_fill(C, x.f.band, affine, [&](auto c, auto pb, auto af) {
        constexpr int kC = decltype(c)::value;
        constexpr bool kPB = decltype(pb)::value, kAffine = decltype(af)::value;
        if (table) return launch_banddir_fill(k_lscore_fill<kC, kPB, kAffine, true>, x, x.f, stream);
        return launch_banddir_fill(k_lscore_fill<kC, kPB, kAffine, false>, x, x.f, stream);
    });
}
