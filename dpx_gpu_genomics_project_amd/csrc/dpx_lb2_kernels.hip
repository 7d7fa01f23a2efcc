/*
 * dpx_lb2_kernels.hip -- two-piece local band-direction batches (DPX_KEEP_LOCAL_BAND_DIRECTIONS | DPX_LOCAL_TWO_PIECE_GAPS) of BASW for
 * gfx950: fill, walk and export.  The definition is include/dpx_align.h's "A second gap piece for BASW local band-direction batches"; the
 * layout is dpx_banddir2.h's unchanged (one byte per in-band cell).
 *
 * k_lb2_fill<C, PB, TABLE> is k_bdl_fill's frame set-up -- dpx_banddir_fill.inc in its EXT form with no scan, H = 0 in every slot without a
 * cell (DPX_BANDDIR_NO_CELL_H) and zero border callables -- around a step of its own, lb2_step:
 *   - bd2_step's four gap planes in int32 registers, Dk = max(H_up + ok + ek, Dk_up + ek) and Ik likewise, GAP_OPEN winning a tie; the
 *     winner of diag, D1, D2, I1, I2 in that order, a candidate that is >= the winner so far taking the cell; the byte code (move in bits
 *     0-2, the four extend bits in 3-6) and the sign-bit extend tests;
 *   - bdl_step's local rules: a neighbour without a cell (border, outside the band, outside the matrix) reads H = 0 and every gap plane
 *     DPX_NEG -- the DPP fill values and what an invalid slot hands on; there is no border value --, H = max(0, winner), move 0 where
 *     H == 0 (min(move, 8 * H) on the floored H: H >= 1 makes 8 * H exceed every move, and H <= 2^28 keeps 8 * H inside 32 bits), and the
 *     tracker of the first maximum in row-major order on every step;
 *   - bdx_step's table scheme (TABLE): characters translated as they enter their window, all C signed-byte reads issued before the first
 *     is used.
 * C = 1, 2, 4 only (bands up to 256), as for k_bd2_fill; 3 C x 2 parities x TABLE 0 / 1 = 12 instantiations.  The step is this unit's own
 * on purpose: sharing a step between fills moved their compiled code (profiles/banddir_sharing_ab.md).
 *
 * k_lb2_traceback is banddir_walk's LOCAL form over the byte codec, five states: from the end cell in SCORING until H == 0 (move 0, or a
 * cell without a code), no tails.  An edge cell's gap planes always open (the neighbour outside the band read DPX_NEG), so no gap state
 * extends out of the band.  k_lb2_export is banddir_export's LOCAL form and serves the six selectors of dpx_batch_directions: 0 on the
 * borders and outside the band in every plane.
 */
#include "dpx_banddir_dev.hpp"

namespace {

using namespace dpx_band;

template <int C>
struct Lb2State {
    int prevH[C], prev2H[C];   /* H on anti-diagonals a-1 and a-2 */
    int prevI1[C], prevD1[C];  /* the gap planes on anti-diagonal a-1 */
    int prevI2[C], prevD2[C];
    int qch[C], rch[C];        /* query / reference character of each slot's cell (TABLE: query code / reference code << 5) */
    long long bestKey;         /* the lane's running maximum of (H << 32 | ~row), signed: the highest H, then the smallest row ... */
    int bestA;                 /* ... and the step of its first occurrence (the smallest column of that row) */
    int lim;                   /* B-1 - lane*C: slot c is inside the band on a step of parity p when c + p <= lim */
    int fin;                   /* (the frame's; not used: the end cell is the tracker's) */
    uint32_t w[4];             /* the code window: 16 bytes, the oldest step lowest */
    __device__ __forceinline__ void clear_gaps(const int c) { prevI1[c] = DPX_NEG; prevD1[c] = DPX_NEG; prevI2[c] = DPX_NEG; prevD2[c] = DPX_NEG; }
};

/* the two pieces: o + e and e of each */
struct Lb2Gaps { int oe1, e1, oe2, e2; };

/* one anti-diagonal.  INTERIOR: every in-band slot lies inside the matrix, so validity is one compare against the per-lane constant
 * `lim` */
template <int C, bool TABLE, bool P1, bool INTERIOR>
__device__ __forceinline__ void lb2_step(Lb2State<C> &st, const int A, int &i0, int &j0, const int lane, const int m, const int n,
                                         const int B, [[maybe_unused]] const int match, [[maybe_unused]] const int mismatch, const Lb2Gaps &g,
                                         const unsigned char *qL, const unsigned char *rL, [[maybe_unused]] const signed char *tabL,
                                         [[maybe_unused]] const unsigned char *codeL) {
    const int p = P1 ? 1 : 0;
    if constexpr (P1) i0++; else j0++;
    const int smin = INTERIOR ? 0 : max(max(1 - i0, j0 - n), 0);
    const int smax = INTERIOR ? 0 : min(min(m - i0, j0 - 1), B - 1 - p);
    const int lo = smin - lane * C, cnt = max(smax - smin + 1, 0);
    int upH[C], upD1[C], upD2[C], leftH[C], leftI1[C], leftI2[C];
    if constexpr (P1) {
        int newq = INTERIOR ? qL[i0 + 64 * C - 2] : qL[min(max(i0 + 64 * C - 2, 0), m - 1)];
        if constexpr (TABLE) newq = codeL[newq];
        const int tq = wave_shl1(st.qch[0], newq);
#pragma unroll
        for (int c = 0; c < C - 1; c++) st.qch[c] = st.qch[c + 1];
        st.qch[C - 1] = tq;
        const int nbH = wave_shl1(st.prevH[0], 0); /* (the last lane has no neighbour: a cell outside the band, H = 0) */
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
        const int nbH = wave_shr1(st.prevH[C - 1], 0);
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
    const int nrow0 = ~(i0 + lane * C); /* ~row of slot c is nrow0 - c */
    uint32_t word = 0u;
#pragma unroll
    for (int cc = 0; cc < C; cc++) {
        /* a p = 0 step reads its upper neighbour from slot c - 1: going down the slots there, every slot is read before it is replaced */
        const int c = P1 ? cc : C - 1 - cc;
        const int d1Open = upH[c] + g.oe1, d1Ext = upD1[c] + g.e1, d2Open = upH[c] + g.oe2, d2Ext = upD2[c] + g.e2;
        const int i1Open = leftH[c] + g.oe1, i1Ext = leftI1[c] + g.e1, i2Open = leftH[c] + g.oe2, i2Ext = leftI2[c] + g.e2;
        const int d1 = max(d1Open, d1Ext), d2 = max(d2Open, d2Ext);
        const int i1 = max(i1Open, i1Ext), i2 = max(i2Open, i2Ext);
        const int dg = st.prev2H[c] + sc[c];
        /* the definition's order: diag, then D1, D2, I1, I2, each taking the cell when it is >= the winner so far; then the floor */
        const int t1 = max(dg, d1), t2 = max(t1, d2), t3 = max(t2, i1);
        int h = max(max(t3, i2), 0);
        uint32_t mv = d1 >= dg ? 2u : 1u;
        mv = d2 >= t1 ? 4u : mv;
        mv = i1 >= t2 ? 3u : mv;
        mv = i2 >= t3 ? 5u : mv;
        /* extends: the sign bit of open - ext (every operand lies within +-2^30, so no difference wraps); GAP_OPEN wins a tie */
        const uint32_t x1 = ((uint32_t)i1Open - (uint32_t)i1Ext) >> 31, y1 = ((uint32_t)d1Open - (uint32_t)d1Ext) >> 31;
        const uint32_t x2 = ((uint32_t)i2Open - (uint32_t)i2Ext) >> 31, y2 = ((uint32_t)d2Open - (uint32_t)d2Ext) >> 31;
        /* move 0 where H == 0: H >= 1 makes 8 * H exceed every move (H <= 2^28, so 8 * H fits) */
        const uint32_t code = min(mv, (uint32_t)h << 3) | (x1 << 3) | (y1 << 4) | (x2 << 5) | (y2 << 6);
        word |= code << (8 * c);
        /* a slot without a cell hands on what its neighbours must read there: H = 0, every gap plane minus infinity */
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
        st.prevI1[c] = valid ? i1 : DPX_NEG;
        st.prevD1[c] = valid ? d1 : DPX_NEG;
        st.prevI2[c] = valid ? i2 : DPX_NEG;
        st.prevD2[c] = valid ? d2 : DPX_NEG;
    }
    window_push<8 * C>(st.w, word);
}

template <int C, bool PB, bool TABLE>
__global__ void __launch_bounds__(DPX_FILL_THREADS) k_lb2_fill(const dpx_lb2_args y) {
    static_assert(C == 1 || C == 2 || C == 4, "bands up to 256");
    constexpr bool EXT = true;
    constexpr int SCAN = 0;
    const dpx_bd2_args x = {y.f, y.tab, {-1, -1, nullptr}, y.gapOpen2, y.gapExtend2}; /* (the frame's names; its scan is off) */
    const dpx_fill_args &a = x.f;
    using State = Lb2State<C>;
    constexpr int Gd = 16 / C, kStepBits = 8 * C; /* steps per 16-byte store (a multiple of 4); a byte per cell */
    [[maybe_unused]] constexpr bool kPickUniform = false;
    /* (every border cell is 0: the border line of an empty sequence never displaces the 0 of (0, 0)) */
#define DPX_BANDDIR_WEIGHTS                                                                                                   \
    [[maybe_unused]] const int match = a.match, mismatch = a.mismatch;                                                        \
    const Lb2Gaps g = {a.gapOpen + a.gapExtend, a.gapExtend, x.gapOpen2 + x.gapExtend2, x.gapExtend2};                        \
    [[maybe_unused]] const int Z = -1, pen = 0;                                                                               \
    const int bord1 = 0;                                                                                                      \
    auto bord = [](const int) -> int { return 0; };                                                                           \
    auto line_first_max = [](const int L) -> int { return min(L, 1); };
#define DPX_BANDDIR_NO_CELL_H 0
#define DPX_BANDDIR_STEP(P1_, INTERIOR_, A_) \
    lb2_step<C, TABLE, P1_, INTERIOR_>(st, A_, i0, j0, lane, m, n, B, match, mismatch, g, qL, rL, tabL, codeL)
#include "dpx_banddir_fill.inc"
#undef DPX_BANDDIR_STEP
#undef DPX_BANDDIR_NO_CELL_H
#undef DPX_BANDDIR_WEIGHTS
}

/* ByteCodec with the move 0 of a local cell: NONE in the H plane (and piece 0), not a diagonal */
struct LocalByteCodec : ByteCodec {
    static __device__ __forceinline__ int decode(const int c, const int which) {
        if (which == 0 && (c & 7) == 0) return 0;
        return ByteCodec::decode(c, which);
    }
};

__global__ void __launch_bounds__(64) k_lb2_traceback(const dpx_fill_args a, int numPairs, const uint64_t *tbOff, char *tb, int32_t *tbLen) {
    __shared__ __attribute__((aligned(16))) unsigned char ring[kRingBytes];
    banddir_walk<LocalByteCodec, true>(ring, a, numPairs, tbOff, tb, tbLen, false);
}

/* `which` 0 directionMain, 1 / 2 piece 1's I / D, 3 / 4 piece 2's (directionIndel), 5 the piece of H's gap move */
__global__ void __launch_bounds__(256) k_lb2_export(const unsigned char *codes, const dpx_pair_dev pr, const char *seq, int band, int which,
                                                    uint8_t *out) {
    banddir_export<LocalByteCodec, true>(codes, pr, seq, band, which, out);
}

} // namespace

hipError_t dpx_launch_lb2_fill(const dpx_lb2_args &x, int C, hipStream_t stream) {
    if (x.f.numPairs <= 0) return hipSuccess;
    const bool table = x.tab.table != nullptr;
    if ((table && !x.tab.codeOf) || x.f.band < 1 || x.f.band > DPX_BANDDIR2_MAX_BAND || C != dpx_band_cpl(x.f.band)) return hipErrorInvalidValue;
    const bool pb = ((x.f.band + 1) & 1) != 0; /* parity of step A = 0 */
    return dpx_dev::dispatch_int<1, 2, 4>(C, [&](auto c) {
        return dpx_dev::dispatch_bool(pb, [&](auto pbc) {
            return dpx_dev::dispatch_bool(table, [&](auto tb) {
                return launch_banddir_fill(k_lb2_fill<decltype(c)::value, decltype(pbc)::value, decltype(tb)::value>, x, x.f, stream);
            });
        });
    });
}

hipError_t dpx_launch_lb2_traceback(const dpx_fill_args &a, int numPairs, const uint64_t *tbOff, char *tb, int32_t *tbLen, hipStream_t stream) {
    if (numPairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_lb2_traceback, dim3((unsigned)numPairs), dim3(64), 0, stream, a, numPairs, tbOff, tb, tbLen);
    return hipGetLastError();
}

hipError_t dpx_launch_lb2_export(const uint8_t *codes, const dpx_pair_dev &pr, const char *seq, int band, int which, uint8_t *out,
                                 hipStream_t stream) {
    const uint64_t total = (uint64_t)(pr.m + 1) * (uint64_t)(pr.n + 1);
    if (!total) return hipSuccess;
    if (which < 0 || which > 5) return hipErrorInvalidValue;
    uint64_t blocks = (total + 255) / 256;
    if (blocks > 65536u) blocks = 65536u;
    hipLaunchKernelGGL(k_lb2_export, dim3((unsigned)blocks), dim3(256), 0, stream, codes, pr, seq, band, which, out);
    return hipGetLastError();
}
