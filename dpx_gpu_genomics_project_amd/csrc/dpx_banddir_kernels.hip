/*
 * dpx_banddir_kernels.hip -- banded direction batches (DPX_KEEP_BAND_DIRECTIONS) of BANW and BAXT for gfx950: fill, walk and export.
 *
 * The cells are k_banw_fill's / k_baxt_fill's, value for value, in int32 registers: ANW's Gotoh recurrence restricted to the band
 * |i-j| <= B-1, border cells included, -infinity (DPX_NEG) outside it, no zero floor.  The schedule is theirs too (dpx_banw_kernels.hip:
 * anti-diagonals a = i+j, slot s = (i-j+B-1)>>1, lane l owns the C = dpx_band_cpl(B) slots [l*C, l*C+C), two values per step by DPP,
 * border slots hand on o + a*e in the head phase, head / interior / tail phases, strings staged in LDS).  What is stored differs: no
 * score leaves the registers.  Per cell the fill forms dpx_dir.h's ANW code from compares the recurrence has anyway
 *       move 3 (left) when I >= max(D, diag), else 2 (up) when D >= diag, else 1;  bit 2: I extends (ext > open);  bit 3: D extends
 * and shifts it into a 128-bit register window from the top: after Gd = 32 / C steps the window holds the lane's 16 bytes of a chunk
 * in the layout of dpx_banddir.h, low nibble first, and one 16-byte store writes them.  The phase loops advance by two steps (one of
 * either parity); a store follows the odd step whenever a group is complete.  The last group of a pair is usually partial: its
 * nibbles are shifted down by the steps that are missing and stored into the pair's last chunk, so they land where dpx_banddir_byte
 * says and no store goes past ceil((m+n-1) / Gd) chunks.  The code of a slot that holds no cell is written but never read.
 *
 * Edge cells: I on the band's lower edge and D on its upper edge are -infinity; the bit the fill stores for them is never read (the
 * walk cannot stand there in that state, the export knows them from the geometry).
 *
 * End cell.  BANW: H[m][n] picked up on the last anti-diagonal.  BAXT: every lane keeps one tracker (best H, its row, its step) in three
 * registers, replaced when H is higher or equal on a smaller row (no 16-bit step key: no m + n limit; one tracker per slot would cost
 * 2 * C registers and take the C = 8 fill past 128).  A lane meets the cells of one row on increasing steps, that is in column order,
 * so the tracker holds the lane's first maximum in row-major order; a wave reduction takes the maximum score, then the smallest row,
 * then the smallest column.  Only H > 0 displaces (0, 0).
 *
 * Everything outside bdir_step is the frame shared with k_bdx_fill and k_bd2_fill, dpx_banddir_fill.inc, included in the kernel below with
 * no table and no scan; window_push, the launch helper, the walk (banddir_walk) and the export loop (banddir_export) are
 * dpx_banddir_dev.hpp's, over the nibble codec here.  The step is this unit's own on purpose: sharing a step between fills moved their
 * compiled code (profiles/band_sharing_ab.md, profiles/banddir_sharing_ab.md).
 */
#include "dpx_banddir_dev.hpp"

namespace {

using namespace dpx_band;

template <int C, bool EXT>
struct BdirState {
    int prevH[C], prev2H[C]; /* H on anti-diagonals a-1 and a-2 */
    int prevI[C], prevD[C];  /* I and D on anti-diagonal a-1 */
    int qch[C], rch[C];      /* query / reference character of each slot's cell */
    long long bestKey;       /* EXT: the lane's running maximum of (H << 32 | ~row), signed: the highest H, then the smallest row ... */
    int bestA;               /* ... and the step of its first occurrence (the smallest column of that row) */
    int lim;                 /* B-1 - lane*C: slot c is inside the band on a step of parity p when c + p <= lim */
    int fin;                 /* !EXT: H[m][n], picked up on the last anti-diagonal by the lane that owns its slot */
    uint32_t w[4];           /* the code window: 32 nibbles, the oldest step lowest */
    __device__ __forceinline__ void clear_gaps(const int c) { prevI[c] = DPX_NEG; prevD[c] = DPX_NEG; }
};

/* one anti-diagonal.  INTERIOR: every in-band slot lies inside the matrix, so validity is one compare against the per-lane constant
 * `lim`; no border slot and not the last anti-diagonal (the caller sees to both) */
template <int C, bool EXT, bool P1, bool INTERIOR>
__device__ __forceinline__ void bdir_step(BdirState<C, EXT> &st, const int A, int &i0, int &j0, const int lane, const int m, const int n,
                                          const int B, const int match, const int mismatch, const int o, const int oe, const int e,
                                          const int cEnd, const unsigned char *qL, const unsigned char *rL) {
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
        const int newq = INTERIOR ? qL[i0 + 64 * C - 2] : qL[min(max(i0 + 64 * C - 2, 0), m - 1)];
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
        const int newr = INTERIOR ? rL[j0 - 1] : rL[min(max(j0 - 1, 0), n - 1)];
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
    const int nrow0 = ~(i0 + lane * C); /* ~row of slot c is nrow0 - c (a border slot decodes to row 0 or column 0) */
    uint32_t word = 0u;
#pragma unroll
    for (int cc = 0; cc < C; cc++) {
        /* a p = 0 step reads its upper neighbour from slot c - 1: going down the slots there, every slot is read before it is replaced */
        const int c = P1 ? cc : C - 1 - cc;
        const int sc = (st.qch[c] == st.rch[c]) ? match : mismatch;
        const int dOpen = upH[c] + oe, dExt = upD[c] + e;
        const int iOpen = leftH[c] + oe, iExt = leftI[c] + e;
        int d = max(dOpen, dExt);
        int ii = max(iOpen, iExt);
        const int dg = st.prev2H[c] + sc;
        const int top = max(d, dg);
        int h = max(ii, top); /* (no floor; the diagonal neighbour of an in-band cell is in band, so h is finite) */
        /* the definition's order: D >= diag takes the move, then I >= the winner takes it from either.  The four tests are sign bits of
         * differences (every operand lies within +-2^30, so no difference wraps): eight cells' worth of compare masks would not fit
         * the scalar registers */
        const uint32_t iLoses = ((uint32_t)ii - (uint32_t)top) >> 31;   /* I < max(D, diag) */
        const uint32_t dLoses = ((uint32_t)d - (uint32_t)dg) >> 31;     /* D < diag */
        const uint32_t iExtends = ((uint32_t)iOpen - (uint32_t)iExt) >> 31, dExtends = ((uint32_t)dOpen - (uint32_t)dExt) >> 31;
        const uint32_t code = (3u - iLoses - (iLoses & dLoses)) | (iExtends << 2) | (dExtends << 3); /* move 3 left, 2 up, 1 diagonal */
        word |= code << (4 * c);
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
    window_push<4 * C>(st.w, word);
}

template <int C, bool PB, bool EXT>
__global__ void __launch_bounds__(DPX_FILL_THREADS) k_bdir_fill(const dpx_fill_args f) {
    constexpr bool TABLE = false;
    constexpr int SCAN = 0;
    const dpx_bdx_args x = {f, {nullptr, nullptr}, {-1, -1, nullptr}}; /* (the frame's names; nothing of it but x.f is read) */
    const dpx_fill_args &a = x.f;
    using State = BdirState<C, EXT>;
    constexpr int Gd = 32 / C, kStepBits = 4 * C; /* steps per 16-byte store (a multiple of 4); a nibble per cell */
    [[maybe_unused]] constexpr bool kPickUniform = false;
    /* (the border line is linear in k: its first maximum is at k = L when e > 0 and at k = 1 otherwise) */
#define DPX_BANDDIR_WEIGHTS                                                                                              \
    const int match = a.match, mismatch = a.mismatch, o = a.gapOpen, e = a.gapExtend, oe = a.gapOpen + a.gapExtend;      \
    [[maybe_unused]] const int Z = -1, pen = 0;                                                                          \
    const int bord1 = oe;                                                                                                \
    auto bord = [o, e](const int k) -> int { return o + k * e; };                                                        \
    auto line_first_max = [e](const int L) -> int { return e > 0 ? L : min(L, 1); };
#define DPX_BANDDIR_NO_CELL_H DPX_NEG
#define DPX_BANDDIR_STEP(P1_, INTERIOR_, A_) \
    bdir_step<C, EXT, P1_, INTERIOR_>(st, A_, i0, j0, lane, m, n, B, match, mismatch, o, oe, e, cEnd, qL, rL)
#include "dpx_banddir_fill.inc"
#undef DPX_BANDDIR_STEP
#undef DPX_BANDDIR_NO_CELL_H
#undef DPX_BANDDIR_WEIGHTS
}

__global__ void __launch_bounds__(64) k_bdir_traceback(const dpx_fill_args a, int numPairs, const uint64_t *tbOff, char *tb, int32_t *tbLen) {
    __shared__ __attribute__((aligned(16))) unsigned char ring[kRingBytes];
    banddir_walk<NibbleCodec>(ring, a, numPairs, tbOff, tb, tbLen);
}

/* `which` 0 directionMain, 1 / 2 directionIndel of I / D */
__global__ void __launch_bounds__(256) k_bdir_export(const unsigned char *codes, const dpx_pair_dev pr, const char *seq, int band, int which,
                                                     uint8_t *out) {
    banddir_export<NibbleCodec>(codes, pr, seq, band, which, out);
}

} // namespace

hipError_t dpx_launch_bdir_fill(const dpx_fill_args &a, int C, bool ext, hipStream_t stream) {
    if (a.numPairs <= 0) return hipSuccess;
    return dispatch_fill(C, a.band, ext, [&](auto c, auto pb, auto e) {
        return launch_banddir_fill(k_bdir_fill<decltype(c)::value, decltype(pb)::value, decltype(e)::value>, a, a, stream);
    });
}

hipError_t dpx_launch_bdir_traceback(const dpx_fill_args &a, int numPairs, const uint64_t *tbOff, char *tb, int32_t *tbLen, hipStream_t stream) {
    if (numPairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_bdir_traceback, dim3((unsigned)numPairs), dim3(64), 0, stream, a, numPairs, tbOff, tb, tbLen);
    return hipGetLastError();
}

hipError_t dpx_launch_bdir_export(const uint8_t *codes, const dpx_pair_dev &pr, const char *seq, int band, int which, uint8_t *out,
                                  hipStream_t stream) {
    const uint64_t total = (uint64_t)(pr.m + 1) * (uint64_t)(pr.n + 1);
    if (!total) return hipSuccess;
    uint64_t blocks = (total + 255) / 256;
    if (blocks > 65536u) blocks = 65536u;
    hipLaunchKernelGGL(k_bdir_export, dim3((unsigned)blocks), dim3(256), 0, stream, codes, pr, seq, band, which, out);
    return hipGetLastError();
}
