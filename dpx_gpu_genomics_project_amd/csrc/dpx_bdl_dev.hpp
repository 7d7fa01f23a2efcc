/*
 * dpx_bdl_dev.hpp -- the step of the local band-direction fills, shared by dpx_bdl_kernels.hip (k_bdl_fill: byte equality) and
 * dpx_bdlt_kernels.hip (k_bdlt_fill: the diagonal term from a substitution table).  One text, a TABLE template constant as bdx_step has;
 * with TABLE = false it is the step k_bdl_fill had in its own unit, and its 16 kernels compile to the instructions they had
 * (profiles/r17/plain_bdl_isa.txt).
 *
 * Codes (one nibble, dpx_dir.h):
 *   BSW   LSW's code.  t = max(up, left, corner) with the one gap weight gapOpen, H = max(0, t); bits 0-1 the move: 0 iff t < 0, else 2
 *         (up) when up == H, else 3 (left) when left == H, else 1; bit 2: H == 0.  A cell with t == 0 has H == 0 and still carries a move.
 *   BASW  ASW's code.  D and I with GAP_OPEN winning a tie; best = diag, D >= best takes it, then I >= best takes it; H = max(0, best);
 *         bits 0-1 the move, 0 where H == 0; bit 2: I extends; bit 3: D extends.
 * Every test is the sign bit of a difference, as in bdir_step (the operands lie within +-2^30: fits_dir admits |values| <= 2^28 and
 * DPX_NEG is -2^29, so no difference wraps); BASW's "move 0 where H == 0" is min(move, 4 * H) on the floored H, two operations where a
 * test of best <= 0 and a mask took four (10 000 x 4096^2 at band 128: 9.75 against 10.28 ms, profiles/r13/).
 *
 * TABLE: the diagonal term is table[(codeOf[ref byte] << 5) + codeOf[qry byte]].  Table and map lie in the wave's LDS slice behind the
 * staged strings (the frame stages them, dpx_banddir_fill.inc); a character is translated once as it enters its window -- the query's
 * to its code, the reference's to its code << 5 -- and the C signed-byte reads of a step are issued before the first is used
 * (bdx_step's scheme).  Nothing else of the step knows about the table: the floor, the tie orders, the codes and the tracker are the same.
 */
#ifndef DPX_BDL_DEV_HPP
#define DPX_BDL_DEV_HPP

#include "dpx_banddir_dev.hpp"

namespace dpx_band {

template <int C, bool AFFINE>
struct BdlState {
    int prevH[C], prev2H[C];                   /* H on anti-diagonals a-1 and a-2 */
    int prevI[AFFINE ? C : 1], prevD[AFFINE ? C : 1]; /* BASW: I and D on anti-diagonal a-1 (BSW has no gap planes) */
    int qch[C], rch[C];                        /* query / reference character of each slot's cell (TABLE: query code / reference code << 5) */
    long long bestKey;                         /* the lane's running maximum of (H << 32 | ~row), signed: the highest H, then the smallest row ... */
    int bestA;                                 /* ... and the step of its first occurrence (the smallest column of that row) */
    int lim;                                   /* B-1 - lane*C: slot c is inside the band on a step of parity p when c + p <= lim */
    int fin;                                   /* (the frame's; not used: the end cell is the tracker's) */
    uint32_t w[4];                             /* the code window: 32 nibbles, the oldest step lowest */
    __device__ __forceinline__ void clear_gaps(const int c) {
        if constexpr (AFFINE) { prevI[c] = DPX_NEG; prevD[c] = DPX_NEG; }
    }
};

/* one anti-diagonal.  INTERIOR: every in-band slot lies inside the matrix, so validity is one compare against the per-lane constant
 * `lim`.  g: BSW's gap weight, BASW's gapOpen + gapExtend; e: BASW's gapExtend */
template <int C, bool AFFINE, bool TABLE, bool P1, bool INTERIOR>
__device__ __forceinline__ void bdl_step(BdlState<C, AFFINE> &st, const int A, int &i0, int &j0, const int lane, const int m, const int n,
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
    uint32_t word = 0u;
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
        uint32_t code;
        if constexpr (AFFINE) {
            const int dOpen = upH[c] + g, dExt = upD[c] + e;
            const int iOpen = leftH[c] + g, iExt = leftI[c] + e;
            d = max(dOpen, dExt);
            ii = max(iOpen, iExt);
            const int top = max(d, dg);
            h = max(max(ii, top), 0);
            /* the definition's order: D >= diag takes the move, then I >= the winner takes it from either; move 0 where H == 0 */
            const uint32_t iLoses = ((uint32_t)ii - (uint32_t)top) >> 31;  /* I < max(D, diag) */
            const uint32_t dLoses = ((uint32_t)d - (uint32_t)dg) >> 31;    /* D < diag */
            const uint32_t iExtends = ((uint32_t)iOpen - (uint32_t)iExt) >> 31, dExtends = ((uint32_t)dOpen - (uint32_t)dExt) >> 31;
            /* move 3 left, 2 up, 1 diagonal, and 0 where H == 0: H >= 1 makes 4 * H exceed every move (H <= 2^28, so 4 * H fits) */
            code = min(3u - iLoses - (iLoses & dLoses), (uint32_t)h << 2) | (iExtends << 2) | (dExtends << 3);
        } else {
            const int up = upH[c] + g, left = leftH[c] + g;
            const int lc = max(left, dg);
            const int t = max(up, lc);
            h = max(t, 0);
            /* up when up == t, else left when left == t, else the diagonal; nothing when t < 0 */
            const uint32_t upLoses = ((uint32_t)up - (uint32_t)lc) >> 31;  /* up < max(left, diag) */
            const uint32_t leftLoses = ((uint32_t)left - (uint32_t)dg) >> 31; /* left < diag */
            const uint32_t tNeg = (uint32_t)t >> 31, zero = ((uint32_t)t - 1u) >> 31; /* t < 0; t <= 0, that is H == 0 */
            code = ((2u + upLoses - 2u * (upLoses & leftLoses)) & (tNeg - 1u)) | (zero << 2); /* move 2 up, 3 left, 1 diagonal */
        }
        word |= code << (4 * c);
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
    window_push<4 * C>(st.w, word);
}

} // namespace dpx_band
#endif
