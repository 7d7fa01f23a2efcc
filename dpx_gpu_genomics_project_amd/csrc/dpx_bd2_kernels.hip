/*
 * dpx_bd2_kernels.hip -- two-piece banded direction batches (DPX_KEEP_BAND_DIRECTIONS | DPX_TWO_PIECE_GAPS) of BANW and BAXT for gfx950:
 * fill, walk and export.  The definition is include/dpx_align.h's "Two-piece affine gaps"; the layout is dpx_banddir2.h's.
 *
 * k_bd2_fill<C, PB, EXT, TABLE, SCAN> is k_bdx_fill with
 *   - four gap planes in int32 registers, Dk = max(H_up + ok + ek, Dk_up + ek) and Ik likewise, GAP_OPEN winning a tie;
 *   - H = the winner of diag, D1, D2, I1, I2 in that order, a candidate that is >= the winner so far taking the cell;
 *   - one BYTE per cell (move in bits 0-2, the four extend bits in 3-6), C bytes per step into the window, one 16-byte store per
 *     Gd = 16 / C steps;
 *   - the in-band border cells carrying g(a) = max(o1 + a * e1, o2 + a * e2), and pen = max(0, -max(e1, e2)) in the drop test.
 * C = 1, 2, 4 only (bands up to 256): at C = 8 the five planes of two anti-diagonals do not fit the register file.  Every mode is
 * instantiated, "no table, no scan" included (there is no other two-piece kernel to fall back on): BANW TABLE 0 / 1, BAXT TABLE x SCAN
 * 0 / 1 / 2, times 3 C and 2 parities = 48.  Everything outside the step is the shared frame, dpx_banddir_fill.inc, included in the kernel
 * below (schedule, three phases, code window, first-maximum tracker, table image in LDS, scan, drops and the partial last group, with
 * Gd = 16 / C); window_push, the launch helper and the scan after a step are dpx_banddir_dev.hpp's.  The step, bd2_step, is this unit's
 * own on purpose: sharing a step between fills moved their compiled code (profiles/band_sharing_ab.md,
 * profiles/banddir_sharing_ab.md).
 *
 * k_bd2_traceback is banddir_walk (dpx_banddir_dev.hpp) over the byte codec, five states: SCORING, and one per gap plane.  k_bd2_export is
 * banddir_export over it and serves the six selectors of dpx_batch_directions.
 */
#include "dpx_banddir_dev.hpp"

namespace {

using namespace dpx_band;

template <int C>
struct Bd2State {
    int prevH[C], prev2H[C];   /* H on anti-diagonals a-1 and a-2 */
    int prevI1[C], prevD1[C];  /* the gap planes on anti-diagonal a-1 */
    int prevI2[C], prevD2[C];
    int qch[C], rch[C];        /* query / reference character of each slot's cell (TABLE: query code / reference code << 5) */
    long long bestKey;         /* EXT: the lane's running maximum of (H << 32 | ~row), signed: the highest H, then the smallest row ... */
    int bestA;                 /* ... and the step of its first occurrence (the smallest column of that row) */
    int lim;                   /* B-1 - lane*C: slot c is inside the band on a step of parity p when c + p <= lim */
    int fin;                   /* !EXT: H[m][n], picked up on the last anti-diagonal by the lane that owns its slot */
    uint32_t w[4];             /* the code window: 16 bytes, the oldest step lowest */
    __device__ __forceinline__ void clear_gaps(const int c) { prevI1[c] = DPX_NEG; prevD1[c] = DPX_NEG; prevI2[c] = DPX_NEG; prevD2[c] = DPX_NEG; }
};

/* the two pieces: o + e and e of each */
struct Bd2Gaps { int oe1, e1, oe2, e2, o1, o2; };
__device__ __forceinline__ int gap_of(const Bd2Gaps &g, const int k) { return max(g.o1 + k * g.e1, g.o2 + k * g.e2); }

/* one anti-diagonal: bdx_step with two more planes and the byte code.  INTERIOR: every in-band slot lies inside the matrix, so validity is
 * one compare against the per-lane constant `lim`; no border slot and not the last anti-diagonal */
template <int C, bool EXT, bool TABLE, bool P1, bool INTERIOR>
__device__ __forceinline__ void bd2_step(Bd2State<C> &st, const int A, int &i0, int &j0, const int lane, const int m, const int n,
                                         const int B, const int match, const int mismatch, const Bd2Gaps &g, const int cEnd,
                                         const unsigned char *qL, const unsigned char *rL, const signed char *tabL, const unsigned char *codeL) {
    const int p = P1 ? 1 : 0;
    if constexpr (P1) i0++; else j0++;
    const int smin = INTERIOR ? 0 : max(max(1 - i0, j0 - n), 0);
    const int smax = INTERIOR ? 0 : min(min(m - i0, j0 - 1), B - 1 - p);
    /* the in-band border cells of this anti-diagonal: (0, a) in slot -i0 and (a, 0) in slot j0, both H = g(a), while a <= B-1 */
    const int a = A + 2;
    const int bord = (INTERIOR || a > B - 1) ? DPX_NEG : gap_of(g, a);
    const int sTop = (INTERIOR || a > n) ? -1 : -i0, sLeft = (INTERIOR || a > m) ? -1 : j0;
    const int lo = smin - lane * C, cnt = max(smax - smin + 1, 0), cTop = sTop - lane * C, cLeft = sLeft - lane * C;
    const bool last = !INTERIOR && a == m + n;
    int upH[C], upD1[C], upD2[C], leftH[C], leftI1[C], leftI2[C];
    if constexpr (P1) {
        int newq = INTERIOR ? qL[i0 + 64 * C - 2] : qL[min(max(i0 + 64 * C - 2, 0), m - 1)];
        if constexpr (TABLE) newq = codeL[newq];
        const int tq = wave_shl1(st.qch[0], newq);
#pragma unroll
        for (int c = 0; c < C - 1; c++) st.qch[c] = st.qch[c + 1];
        st.qch[C - 1] = tq;
        const int nbH = wave_shl1(st.prevH[0], DPX_NEG);
        const int nbI1 = wave_shl1(st.prevI1[0], DPX_NEG);
        const int nbI2 = wave_shl1(st.prevI2[0], DPX_NEG);
#pragma unroll
        for (int c = 0; c < C; c++) {
            upH[c] = st.prevH[c];
            upD1[c] = st.prevD1[c];
            upD2[c] = st.prevD2[c];
            leftH[c] = (c < C - 1) ? st.prevH[c + 1] : nbH;
            leftI1[c] = (c < C - 1) ? st.prevI1[c + 1] : nbI1;
            leftI2[c] = (c < C - 1) ? st.prevI2[c + 1] : nbI2;
        }
    } else {
        int newr = INTERIOR ? rL[j0 - 1] : rL[min(max(j0 - 1, 0), n - 1)];
        if constexpr (TABLE) newr = (int)codeL[newr] << 5;
        const int tr = wave_shr1(st.rch[C - 1], newr);
#pragma unroll
        for (int c = C - 1; c > 0; c--) st.rch[c] = st.rch[c - 1];
        st.rch[0] = tr;
        const int nbH = wave_shr1(st.prevH[C - 1], DPX_NEG);
        const int nbD1 = wave_shr1(st.prevD1[C - 1], DPX_NEG);
        const int nbD2 = wave_shr1(st.prevD2[C - 1], DPX_NEG);
#pragma unroll
        for (int c = 0; c < C; c++) {
            leftH[c] = st.prevH[c];
            leftI1[c] = st.prevI1[c];
            leftI2[c] = st.prevI2[c];
            upH[c] = (c > 0) ? st.prevH[c - 1] : nbH;
            upD1[c] = (c > 0) ? st.prevD1[c - 1] : nbD1;
            upD2[c] = (c > 0) ? st.prevD2[c - 1] : nbD2;
        }
    }
    int sc[C]; /* TABLE: all C byte reads are in flight before the first is used (codes are < 32: the address stays inside the 1-KiB table) */
#pragma unroll
    for (int c = 0; c < C; c++) {
        if constexpr (TABLE) sc[c] = (int)tabL[st.rch[c] + st.qch[c]];
        else sc[c] = (st.qch[c] == st.rch[c]) ? match : mismatch;
    }
    const int nrow0 = ~(i0 + lane * C); /* ~row of slot c is nrow0 - c (a border slot decodes to row 0 or column 0) */
    uint32_t word = 0u;
#pragma unroll
    for (int cc = 0; cc < C; cc++) {
        /* a p = 0 step reads its upper neighbour from slot c - 1: going down the slots there, every slot is read before it is replaced */
        const int c = P1 ? cc : C - 1 - cc;
        const int d1Open = upH[c] + g.oe1, d1Ext = upD1[c] + g.e1, d2Open = upH[c] + g.oe2, d2Ext = upD2[c] + g.e2;
        const int i1Open = leftH[c] + g.oe1, i1Ext = leftI1[c] + g.e1, i2Open = leftH[c] + g.oe2, i2Ext = leftI2[c] + g.e2;
        int d1 = max(d1Open, d1Ext), d2 = max(d2Open, d2Ext);
        int i1 = max(i1Open, i1Ext), i2 = max(i2Open, i2Ext);
        const int dg = st.prev2H[c] + sc[c];
        /* the definition's order: diag, then D1, D2, I1, I2, each taking the cell when it is >= the winner so far (no floor; the diagonal
         * neighbour of an in-band cell is in band, so h is finite) */
        const int t1 = max(dg, d1), t2 = max(t1, d2), t3 = max(t2, i1);
        int h = max(t3, i2);
        uint32_t mv = d1 >= dg ? 2u : 1u;
        mv = d2 >= t1 ? 4u : mv;
        mv = i1 >= t2 ? 3u : mv;
        mv = i2 >= t3 ? 5u : mv;
        /* extends: the sign bit of open - ext (every operand lies within +-2^30, so no difference wraps); GAP_OPEN wins a tie */
        const uint32_t x1 = ((uint32_t)i1Open - (uint32_t)i1Ext) >> 31, y1 = ((uint32_t)d1Open - (uint32_t)d1Ext) >> 31;
        const uint32_t x2 = ((uint32_t)i2Open - (uint32_t)i2Ext) >> 31, y2 = ((uint32_t)d2Open - (uint32_t)d2Ext) >> 31;
        const uint32_t code = mv | (x1 << 3) | (y1 << 4) | (x2 << 5) | (y2 << 6);
        word |= code << (8 * c);
        bool valid;
        if constexpr (INTERIOR) {
            valid = (c + p) <= st.lim;
            h = valid ? h : DPX_NEG;
        } else {
            /* slot lane * C + c against the step's window [smin, smax] and its two border slots (cnt = 0 when the window is empty) */
            valid = (unsigned)(c - lo) < (unsigned)cnt;
            h = valid ? h : ((c == cTop || c == cLeft) ? bord : DPX_NEG);
            if constexpr (!EXT) st.fin = (last && c == cEnd) ? h : st.fin;
        }
        d1 = valid ? d1 : DPX_NEG;
        d2 = valid ? d2 : DPX_NEG;
        i1 = valid ? i1 : DPX_NEG;
        i2 = valid ? i2 : DPX_NEG;
        if constexpr (EXT) { /* (after the border select: border cells take part) */
            const long long key = (long long)(((unsigned long long)(unsigned)h << 32) | (unsigned long long)(unsigned)(nrow0 - c));
            const bool up = key > st.bestKey; /* (an equal key is the same row on a later step, a larger column: it stays) */
            st.bestKey = up ? key : st.bestKey;
            st.bestA = up ? A : st.bestA;
        }
        st.prev2H[c] = st.prevH[c];
        st.prevH[c] = h;
        st.prevI1[c] = i1;
        st.prevD1[c] = d1;
        st.prevI2[c] = i2;
        st.prevD2[c] = d2;
    }
    window_push<8 * C>(st.w, word);
}

template <int C, bool PB, bool EXT, bool TABLE, int SCAN>
__global__ void __launch_bounds__(DPX_FILL_THREADS) k_bd2_fill(const dpx_bd2_args x) {
    static_assert(EXT || SCAN == 0, "BANW has no extension mode");
    static_assert(C == 1 || C == 2 || C == 4, "bands up to 256");
    const dpx_fill_args &a = x.f;
    using State = Bd2State<C>;
    constexpr int Gd = 16 / C, kStepBits = 8 * C; /* steps per 16-byte store (a multiple of 4); a byte per cell */
    constexpr bool kPickUniform = false;
    /* (the border line g(k) is convex in k: its first maximum is at k = 1 or at k = L) */
#define DPX_BANDDIR_WEIGHTS                                                                                                          \
    const int match = a.match, mismatch = a.mismatch;                                                                                \
    const Bd2Gaps g = {a.gapOpen + a.gapExtend, a.gapExtend, x.gapOpen2 + x.gapExtend2, x.gapExtend2, a.gapOpen, x.gapOpen2};        \
    const int Z = x.scan.zdrop, pen = max(0, -max(g.e1, g.e2));                                                                           \
    const int bord1 = gap_of(g, 1);                                                                                                  \
    auto bord = [g](const int k) -> int { return gap_of(g, k); };                                                                    \
    auto line_first_max = [g, bord1](const int L) -> int { return (L >= 1 && bord1 >= gap_of(g, L)) ? 1 : L; };
#define DPX_BANDDIR_NO_CELL_H DPX_NEG
#define DPX_BANDDIR_STEP(P1_, INTERIOR_, A_) \
    bd2_step<C, EXT, TABLE, P1_, INTERIOR_>(st, A_, i0, j0, lane, m, n, B, match, mismatch, g, cEnd, qL, rL, tabL, codeL)
#include "dpx_banddir_fill.inc"
#undef DPX_BANDDIR_STEP
#undef DPX_BANDDIR_NO_CELL_H
#undef DPX_BANDDIR_WEIGHTS
}

__global__ void __launch_bounds__(64) k_bd2_traceback(const dpx_fill_args a, int numPairs, const uint64_t *tbOff, char *tb, int32_t *tbLen) {
    __shared__ __attribute__((aligned(16))) unsigned char ring[kRingBytes];
    banddir_walk<ByteCodec>(ring, a, numPairs, tbOff, tb, tbLen);
}

/* `which` 0 directionMain, 1 / 2 piece 1's I / D, 3 / 4 piece 2's (directionIndel), 5 the piece of H's gap move */
__global__ void __launch_bounds__(256) k_bd2_export(const unsigned char *codes, const dpx_pair_dev pr, const char *seq, int band, int which,
                                                    uint8_t *out) {
    banddir_export<ByteCodec>(codes, pr, seq, band, which, out);
}

} // namespace

hipError_t dpx_launch_bd2_fill(const dpx_bd2_args &x, int C, bool ext, hipStream_t stream) {
    if (x.f.numPairs <= 0) return hipSuccess;
    const bool table = x.tab.table != nullptr;
    const int scan = !ext ? 0 : x.scan.zdrop >= 0 ? 2 : x.scan.endBonus >= 0 ? 1 : 0;
    if ((table && !x.tab.codeOf) || (scan && !x.scan.ext) || x.f.band > DPX_BANDDIR2_MAX_BAND || C != dpx_band_cpl(x.f.band)) return hipErrorInvalidValue;
    const bool pb = ((x.f.band + 1) & 1) != 0; /* parity of step A = 0 */
    return dpx_dev::dispatch_int<1, 2, 4>(C, [&](auto c) {
        return dpx_dev::dispatch_bool(pb, [&](auto pbc) {
            return dpx_dev::dispatch_bool(table, [&](auto tb) {
                constexpr int kC = decltype(c)::value;
                constexpr bool kPB = decltype(pbc)::value, kTable = decltype(tb)::value;
                if (!ext) return launch_banddir_fill(k_bd2_fill<kC, kPB, false, kTable, 0>, x, x.f, stream);
                if (scan == 2) return launch_banddir_fill(k_bd2_fill<kC, kPB, true, kTable, 2>, x, x.f, stream);
                if (scan == 1) return launch_banddir_fill(k_bd2_fill<kC, kPB, true, kTable, 1>, x, x.f, stream);
                return launch_banddir_fill(k_bd2_fill<kC, kPB, true, kTable, 0>, x, x.f, stream);
            });
        });
    });
}

hipError_t dpx_launch_bd2_traceback(const dpx_fill_args &a, int numPairs, const uint64_t *tbOff, char *tb, int32_t *tbLen, hipStream_t stream) {
    if (numPairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_bd2_traceback, dim3((unsigned)numPairs), dim3(64), 0, stream, a, numPairs, tbOff, tb, tbLen);
    return hipGetLastError();
}

hipError_t dpx_launch_bd2_export(const uint8_t *codes, const dpx_pair_dev &pr, const char *seq, int band, int which, uint8_t *out,
                                 hipStream_t stream) {
    const uint64_t total = (uint64_t)(pr.m + 1) * (uint64_t)(pr.n + 1);
    if (!total) return hipSuccess;
    if (which < 0 || which > 5) return hipErrorInvalidValue;
    uint64_t blocks = (total + 255) / 256;
    if (blocks > 65536u) blocks = 65536u;
    hipLaunchKernelGGL(k_bd2_export, dim3((unsigned)blocks), dim3(256), 0, stream, codes, pr, seq, band, which, out);
    return hipGetLastError();
}
