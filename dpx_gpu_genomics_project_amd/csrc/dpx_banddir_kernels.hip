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
 */
#include "dpx_band_affine.hpp"
#include "dpx_banddir.h"

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
};

/* `bits` new code bits enter the 128-bit window at the top, everything else moves down */
template <int BITS>
__device__ __forceinline__ void window_push(uint32_t (&w)[4], const uint32_t word) {
    if constexpr (BITS == 32) {
        w[0] = w[1]; w[1] = w[2]; w[2] = w[3]; w[3] = word;
    } else {
        w[0] = __builtin_amdgcn_alignbit(w[1], w[0], BITS);
        w[1] = __builtin_amdgcn_alignbit(w[2], w[1], BITS);
        w[2] = __builtin_amdgcn_alignbit(w[3], w[2], BITS);
        w[3] = (w[3] >> BITS) | (word << (32 - BITS));
    }
}

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
__global__ void __launch_bounds__(DPX_FILL_THREADS) k_bdir_fill(const dpx_fill_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int Gd = 32 / C; /* steps per 16-byte store (a multiple of 4) */
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int p = blockIdx.x * (int)a.wavesPerBlock + wv;
    if (p >= a.numPairs) return;
    if (a.order) p = a.order[p];
    const dpx_pair_dev pr = a.pairs[p];
    const int n = pr.n, m = pr.m, B = a.band;
    const int match = a.match, mismatch = a.mismatch, o = a.gapOpen, e = a.gapExtend, oe = a.gapOpen + a.gapExtend;
    if (m <= 0 || n <= 0) { /* an empty sequence: no cell has a code; the results are k_banw_fill's / k_baxt_fill's */
        if (lane == 0) {
            if constexpr (EXT) {
                /* the in-band cells are one border line, H = o + k*e for 1 <= k <= L and 0 at k = 0: linear in k, so the first maximum is
                 * at k = L when e > 0 and at k = 1 otherwise; it counts when it is above the 0 of (0, 0) */
                const int L = min(max(max(m, n), 0), B - 1);
                const int k = e > 0 ? L : min(L, 1);
                const int v = k > 0 ? o + k * e : 0;
                const bool take = v > 0;
                a.score[p] = take ? v : 0;
                a.endRow[p] = (take && m > 0) ? k : 0;
                a.endCol[p] = (take && m <= 0) ? k : 0;
            } else {
                a.score[p] = (m > 0 || n > 0) ? o + max(m, n) * e : 0;
                a.endRow[p] = max(m, 0);
                a.endCol[p] = max(n, 0);
            }
        }
        return;
    }
    const unsigned char *ref = reinterpret_cast<const unsigned char *>(a.seq + pr.refIdx);
    const unsigned char *qry = reinterpret_cast<const unsigned char *>(a.seq + pr.qryIdx);
    unsigned char *my = smem + (size_t)wv * a.ldsPerWave;
    const unsigned char *qL = stage_bytes(my, qry, m, lane, 64);
    const unsigned char *rL = stage_bytes(my + a.ldsRefOff, ref, n, lane, 64);

    BdirState<C, EXT> st;
    st.lim = B - 1 - lane * C;
    st.fin = DPX_NEG;
    st.w[0] = st.w[1] = st.w[2] = st.w[3] = 0u;
    { /* anti-diagonals a = 1 (prev: the border cells (0, 1) and (1, 0), in band when B >= 2) and a = 0 (prev2: H[0][0] = 0, which
       * shares its slot with cell (1, 1)); the character windows are those of a = 1, the first real step then slides one of them */
        const int p1 = B & 1;
        const int vi0 = (1 + p1 - (B - 1)) >> 1;
        const int vj0 = 1 - vi0;
#pragma unroll
        for (int c = 0; c < C; c++) {
            const int s = lane * C + c;
            st.qch[c] = qL[min(max(vi0 + s - 1, 0), m - 1)];
            st.rch[c] = rL[min(max(vj0 - s - 1, 0), n - 1)];
            const int bi = vi0 + s; /* the slot's cell on a = 1 is (bi, 1 - bi) */
            st.prevH[c] = (B >= 2 && (bi == 0 || bi == 1)) ? oe : DPX_NEG;
            st.prev2H[c] = (s == ((B - 1) >> 1)) ? 0 : DPX_NEG;
            st.prevI[c] = DPX_NEG;
            st.prevD[c] = DPX_NEG;
        }
        st.bestKey = 0xFFFFFFFFll; /* score 0 at row 0: only H > 0 displaces it */
        st.bestA = 0;
    }
    /* the lane and register that own the end cell (m, n) on the last anti-diagonal (BANW) */
    const int sEnd = (m - n + B - 1) >> 1;
    const int cEnd = (!EXT && lane == sEnd / C) ? (sEnd % C) : -1;
    /* is every in-band slot of anti-diagonal A inside the matrix?  (true for one contiguous range of A) */
    auto interior = [&](const int A) -> bool {
        const int aa = A + 2, pp = (aa + B - 1) & 1;
        const int ii0 = (aa + pp - (B - 1)) >> 1, jj0 = aa - ii0, top = B - 1 - pp;
        return ii0 >= 1 && ii0 + top <= m && jj0 - top >= 1 && jj0 <= n;
    };
    const int NS = m + n - 1;                 /* anti-diagonals a = 2 .. m+n */
    const int numGroups = (NS + Gd - 1) / Gd; /* == dpx_banddir_chunks(m, n, B): no store goes past the pair's last chunk */
    unsigned char *base = reinterpret_cast<unsigned char *>(a.mat) + (size_t)pr.matOff * 2u;
    const uint64_t cs = (uint64_t)pr.chunkStride * 2u;
    int i0 = (1 + (B & 1) - (B - 1)) >> 1;
    int j0 = 1 - i0;
    auto store_group = [&](const int grp) {
        if (grp < numGroups)
            *reinterpret_cast<u32x4 *>(base + dpx_banddir_piece((uint64_t)grp, lane, cs)) = u32x4{st.w[0], st.w[1], st.w[2], st.w[3]};
    };
#define DPX_BDIR_BODY(INTERIOR_)                                                                                          \
    {                                                                                                                     \
        bdir_step<C, EXT, PB, INTERIOR_>(st, A0, i0, j0, lane, m, n, B, match, mismatch, o, oe, e, cEnd, qL, rL);         \
        bdir_step<C, EXT, !PB, INTERIOR_>(st, A0 + 1, i0, j0, lane, m, n, B, match, mismatch, o, oe, e, cEnd, qL, rL);    \
        if (((A0 + 2) & (Gd - 1)) == 0) store_group((A0 + 1) / Gd);                                                       \
    }
    /* parity of step A is (A + B + 1) & 1; A0 is even, so even steps have parity PB and odd steps !PB.
     * Three phases: head (some slots outside the matrix, border slots), interior, tail.  The interior loop stops short of the last
     * anti-diagonal (A = NS-1), so BANW's end cell is always picked up by the general step.  When NS is odd the last pair of steps runs
     * one step past NS - 1, which holds no cell. */
    int A0 = 0;
    for (; A0 < NS && !(interior(A0) && interior(A0 + 1)); A0 += 2) DPX_BDIR_BODY(false)
    for (; A0 + 2 < NS && interior(A0 + 1); A0 += 2) DPX_BDIR_BODY(true)
    for (; A0 < NS; A0 += 2) DPX_BDIR_BODY(false)
#undef DPX_BDIR_BODY
    /* the partial last group: A0 steps have been pushed, A0 % Gd of them since the last store; the missing ones are shifted in as
     * zeros so that step t of the group sits at nibble t * C, and the group goes to the pair's last chunk */
    if (A0 & (Gd - 1)) {
        for (int t = A0 & (Gd - 1); t < Gd; t++) window_push<4 * C>(st.w, 0u);
        store_group(A0 / Gd);
    }
    if constexpr (!EXT) {
        if (cEnd >= 0) { a.score[p] = st.fin; a.endRow[p] = m; a.endCol[p] = n; }
    } else {
        /* the lane's candidate; across lanes max score, then min row, then min column.  A border slot decodes to i = 0 or j = 0.
         * (The border cells of anti-diagonal 1, which no step visits, need no candidate: see k_baxt_fill.) */
        int hv = (int)(st.bestKey >> 32);
        unsigned long long at = ~0ull;
        if (hv > 0) {
            const int i = (int)~(unsigned)(st.bestKey & 0xFFFFFFFFll);
            at = ((unsigned long long)(unsigned)i << 32) | (unsigned long long)(unsigned)(st.bestA + 2 - i);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int oh = __shfl_xor(hv, off, 64);
            const unsigned long long oa = __shfl_xor(at, off, 64);
            if (oh > hv || (oh == hv && oa < at)) { hv = oh; at = oa; }
        }
        if (lane == 0) {
            a.score[p] = hv;
            a.endRow[p] = hv > 0 ? (int)(at >> 32) : 0;
            a.endCol[p] = hv > 0 ? (int)(at & 0xFFFFFFFFull) : 0;
        }
    }
}

/* -----------------------------------------------------------------------------------------------------
 * Traceback: one WAVE per pair, k_traceback_dir's run scheme (dpx_dir_kernels.hip) over an LDS ring of code chunks.  The walk moves to
 * strictly smaller anti-diagonals and one chunk holds Gd whole anti-diagonals of the band, so the chunks a path needs are known in
 * advance: the ring holds kRing consecutive chunks as two halves, the walker stands in the upper half, and when it has left it the wave
 * drops that half and streams the next lower one in (every lane its own 16 bytes of each chunk: whole-KiB loads, all in flight at once).
 * A step of the walk: every lane reads the code of one cell of the line the path would follow next from LDS (the walker's diagonal in
 * SCORING, its row in INSERTION, its column in DELETION) and a ballot gives the number of cells the path really follows; a cell below
 * the ring ends the run early, and the next trip slides the ring.  Then ANW's two tails.
 * ----------------------------------------------------------------------------------------------------- */
constexpr int kRing = 16;                                   /* chunks in LDS */
constexpr int kRingBytes = kRing * (int)DPX_BANDDIR_CHUNK_BYTES;

__global__ void __launch_bounds__(64) k_bdir_traceback(const dpx_fill_args a, int numPairs, const uint64_t *tbOff, char *tb, int32_t *tbLen) {
    __shared__ __attribute__((aligned(16))) unsigned char ring[kRingBytes];
    const int p = blockIdx.x, lane = threadIdx.x;
    if (p >= numPairs) return;
    const dpx_pair_dev pr = a.pairs[p];
    const int n = pr.n, m = pr.m, B = a.band;
    const int cap = (m + n + 1 + 3) & ~3;
    char *lr = tb + tbOff[p], *lx = lr + cap, *lq = lx + cap;
    const unsigned char *qry = reinterpret_cast<const unsigned char *>(a.seq + pr.qryIdx);
    const unsigned char *ref = reinterpret_cast<const unsigned char *>(a.seq + pr.refIdx);
    const unsigned char *base = reinterpret_cast<const unsigned char *>(a.mat) + (size_t)pr.matOff * 2u;
    const uint64_t cs = (uint64_t)pr.chunkStride * 2u;
    const int sg = 5 - dpx_log2(dpx_band_cpl(B)); /* Gd = 2^sg */
    const int numChunks = (int)dpx_banddir_chunks(m, n, B);
    constexpr int kHalf = kRing / 2;
    int pos = cap; /* lines grow from the back; the character of run step l goes to pos - 1 - l */
    int i = __builtin_amdgcn_readfirstlane(a.endRow[p]), j = __builtin_amdgcn_readfirstlane(a.endCol[p]);
    int hTop = 0; /* the ring holds the halves hTop and hTop - 1 (half h = chunks [h * kHalf, h * kHalf + kHalf)) */
    bool have = false;
    auto load_half = [&](const int h) { /* (a half below chunk 0 or past the pair's last chunk: nothing to load, nothing reads it) */
        if (h < 0) return;
        u32x4 v[kHalf];
#pragma unroll
        for (int k = 0; k < kHalf; k++) {
            const int c = h * kHalf + k;
            v[k] = c < numChunks ? *reinterpret_cast<const u32x4 *>(base + dpx_banddir_piece((uint64_t)c, lane, cs)) : u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int k = 0; k < kHalf; k++) {
            const int c = h * kHalf + k;
            *reinterpret_cast<u32x4 *>(ring + (c & (kRing - 1)) * (int)DPX_BANDDIR_CHUNK_BYTES + lane * 16) = v[k];
        }
    };
    /* the code of cell (ci, cj): -1 when it has none (border, outside the band or the matrix), -2 when its chunk is below the ring */
    auto code = [&](const int ci, const int cj) -> int {
        if (ci < 1 || cj < 1 || !in_band(ci, cj, B)) return -1;
        if (((ci + cj - 2) >> sg) < (hTop - 1) * kHalf) return -2;
        int sh;
        const uint64_t off = dpx_banddir_byte(ci, cj, B, DPX_BANDDIR_CHUNK_BYTES, &sh);
        return ((int)ring[off & (uint64_t)(kRingBytes - 1)] >> sh) & 0xF;
    };
    auto run_of = [&](const bool cont) -> int { /* leading lanes (from lane 0) whose condition holds */
        const unsigned long long mask = __ballot(cont);
        return ~mask == 0ull ? 64 : __builtin_ctzll(~mask);
    };
    auto put = [&](const int at, const int rc, const int xc, const int qc) { lr[at] = (char)rc; lx[at] = (char)xc; lq[at] = (char)qc; };
    int cur = 0; /* 0 SCORING, 1 INSERTION, 2 DELETION */
    while (i != 0 && j != 0) {
        const int hw = ((i + j - 2) >> sg) / kHalf; /* the walker's half */
        if (!have || hw < hTop) {
            __syncthreads(); /* the reads of the last trip are done before the ring changes */
            if (!have) { hTop = hw; load_half(hw); load_half(hw - 1); have = true; }
            else while (hTop > hw) { hTop--; load_half(hTop - 1); }
            __syncthreads();
        }
        const int c0 = code(i, j); /* the walker's own cell: the same byte for every lane */
        if (c0 < 0) break;         /* (cannot happen: the walker stands on a stored cell of the ring's upper half) */
        const int mv = c0 & 3;
        int kind = mv == 3 ? 3 : mv == 2 ? 2 : 1;
        if (cur != 0) kind = cur == 1 ? 3 : 2;
        if (kind != 1) { /* a gap: step l is taken while the cells before it extend (bit 2 for I, bit 3 for D); the cell that opens ends it */
            const int c = kind == 3 ? code(i, j - lane) : code(i - lane, j), bit = kind == 3 ? 4 : 8;
            const int k = run_of(c >= 0 && (c & bit));
            int steps = 64;
            cur = kind == 3 ? 1 : 2;
            if (k < 64) {
                const int ck = __shfl(c, k, 64);
                if (ck >= 0) { steps = k + 1; cur = 0; } /* cell k opened the gap */
                else steps = k;                          /* cell k lies below the ring: go on from it in the same state */
            }
            if (steps == 0) break; /* (cannot happen: lane 0's cell is c0) */
            if (lane < steps) {
                if (kind == 3) put(pos - 1 - lane, ref[j - 1 - lane], ' ', '_');
                else put(pos - 1 - lane, '_', ' ', qry[i - 1 - lane]);
            }
            pos -= steps;
            if (kind == 3) j -= steps; else i -= steps;
            continue;
        }
        /* the diagonal: step l leaves cell l of the walker's diagonal, which must itself say "diagonal" (lane 0 has said so) */
        const int c = lane == 0 ? c0 : code(i - lane, j - lane);
        const int steps = run_of(c >= 0 && (lane == 0 || (c & 3) == 1));
        if (steps == 0) break; /* (cannot happen) */
        if (lane < steps) {
            const int qd = (int)qry[i - lane - 1], rd = (int)ref[j - lane - 1];
            put(pos - 1 - lane, rd, qd == rd ? '*' : '|', qd);
        }
        pos -= steps;
        i -= steps;
        j -= steps;
    }
    /* ANW's tails: the rest of column 0 as deletions, then the rest of row 0 as insertions (at most one of the two is left) */
    for (int x = lane; x < i; x += 64) put(pos - 1 - x, '_', ' ', qry[i - 1 - x]);
    pos -= max(i, 0);
    for (int x = lane; x < j; x += 64) put(pos - 1 - x, ref[j - 1 - x], ' ', '_');
    pos -= max(j, 0);
    if (lane == 0) tbLen[p] = cap - pos;
}

/* One pair's direction matrix as the oracles write it (c++/backtrack.h enums: directionMain NONE 0, MATCH 1, MISMATCH 2,
 * QUERY_INSERTION 3, QUERY_DELETION 4; directionIndel NONE 0, GAP_OPEN 1, GAP_EXTEND 2): 0 outside the band; the in-band border cells of
 * H as ANW exports them; I on the band's lower edge and D on its upper edge are GAP_OPEN by the geometry (-inf >= -inf). */
__global__ void __launch_bounds__(256) k_bdir_export(const unsigned char *codes, const dpx_pair_dev pr, const char *seq, int band, int which,
                                                     uint8_t *out) {
    const int n = pr.n, m = pr.m;
    const uint64_t total = (uint64_t)(m + 1) * (uint64_t)(n + 1);
    for (uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * blockDim.x) {
        const int i = (int)(idx / (uint64_t)(n + 1)), j = (int)(idx % (uint64_t)(n + 1));
        uint8_t v = 0;
        if (in_band(i, j, band)) {
            if (i == 0 || j == 0) {
                v = (which != 0 || (i | j) == 0) ? 0 : (j == 0 ? 4 : 3); /* column 0: QUERY_DELETION, row 0: QUERY_INSERTION */
            } else if ((which == 1 && i - j == band - 1) || (which == 2 && j - i == band - 1)) {
                v = 1;
            } else {
                int sh;
                const uint64_t off = dpx_banddir_byte(i, j, band, (uint64_t)pr.chunkStride * 2u, &sh);
                const int c = (codes[(size_t)pr.matOff * 2u + off] >> sh) & 0xF;
                if (which == 1) v = (c & 4) ? 2 : 1;
                else if (which == 2) v = (c & 8) ? 2 : 1;
                else {
                    const int mv = c & 3;
                    v = mv == 2 ? 4 : mv == 3 ? 3 : (seq[pr.qryIdx + i - 1] == seq[pr.refIdx + j - 1] ? 1 : 2);
                }
            }
        }
        out[idx] = v;
    }
}

/* (a direction batch sizes its LDS per wave, not as a four-wave request) */
template <class K>
hipError_t launch_bdir_kernel(K kernel, const dpx_fill_args &a, hipStream_t s) {
    const unsigned wpb = a.wavesPerBlock ? a.wavesPerBlock : 1u;
    const size_t lds = (size_t)a.ldsPerWave * wpb;
    if (lds > 64u * 1024u) { /* opt in to more than the default 64 KiB of dynamic LDS */
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const unsigned grid = ((unsigned)a.numPairs + wpb - 1) / wpb;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64u * wpb), lds, s, a);
    return hipGetLastError();
}

} // namespace

hipError_t dpx_launch_bdir_fill(const dpx_fill_args &a, int C, bool ext, hipStream_t stream) {
    if (a.numPairs <= 0) return hipSuccess;
    return dispatch_fill(C, a.band, ext, [&](auto c, auto pb, auto e) {
        return launch_bdir_kernel(k_bdir_fill<decltype(c)::value, decltype(pb)::value, decltype(e)::value>, a, stream);
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
