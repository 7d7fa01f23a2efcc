/*
 * dpx_bd2_kernels.hip -- two-piece banded direction batches (DPX_KEEP_BAND_DIRECTIONS | DPX_TWO_PIECE_GAPS) of BANW and BAXT for gfx950:
 * fill, walk and export.  The definition is include/dpx_align.h's "Two-piece affine gaps"; the layout is dpx_banddir2.h's.
 *
 * k_bd2_fill<C, PB, EXT, TABLE, SCAN> is k_bdx_fill's step, schedule, three phases, 128-bit code window, first-maximum tracker, table
 * image in LDS and scan (dpx_bdx_kernels.hip explains each), with
 *   - four gap planes in int32 registers, Dk = max(H_up + ok + ek, Dk_up + ek) and Ik likewise, GAP_OPEN winning a tie;
 *   - H = the winner of diag, D1, D2, I1, I2 in that order, a candidate that is >= the winner so far taking the cell;
 *   - one BYTE per cell (move in bits 0-2, the four extend bits in 3-6), C bytes per step into the window, one 16-byte store per
 *     Gd = 16 / C steps;
 *   - the in-band border cells carrying g(a) = max(o1 + a * e1, o2 + a * e2), and pen = max(0, -max(e1, e2)) in the drop test.
 * C = 1, 2, 4 only (bands up to 256): at C = 8 the five planes of two anti-diagonals do not fit the register file.  Every mode is
 * instantiated, "no table, no scan" included (there is no other two-piece kernel to fall back on): BANW TABLE 0 / 1, BAXT TABLE x SCAN
 * 0 / 1 / 2, times 3 C and 2 parities = 48.  That unit and k_bdir_fill's stay as they are (regrouping shared code moves the compiled
 * fills, dpx_band_affine.hpp), so the step's frame and window_push are copied here; zdrop_test and write_results are the shared ones.
 *
 * A drop, the partial last group and what is never stored: as in k_bdx_fill, with Gd = 16 / C.
 *
 * k_bd2_traceback is k_bdir_traceback's scheme (one wave per pair, an LDS ring of 16 whole chunks in two halves, runs by ballot, a cell
 * below the ring ends the run) with five states: SCORING, and one per gap plane.  In SCORING the cell's move names the plane; in a gap
 * state the walk follows that plane's own extend bit.  k_bd2_export serves the six selectors of dpx_batch_directions.
 */
#include "dpx_band_affine.hpp"
#include "dpx_banddir2.h"

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
};

/* the two pieces: o + e and e of each */
struct Bd2Gaps { int oe1, e1, oe2, e2, o1, o2; };
__device__ __forceinline__ int gap_of(const Bd2Gaps &g, const int k) { return max(g.o1 + k * g.e1, g.o2 + k * g.e2); }

/* `bits` new code bits enter the 128-bit window at the top, everything else moves down (dpx_banddir_kernels.hip's, copied) */
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

/* an empty sequence in extension mode (m <= 0 or n <= 0), on one lane: scan_border_line with the border line carrying g(k).  At most
 * B - 1 cells. */
template <bool ZDROP>
__device__ __forceinline__ void scan_border_line2(const dpx_fill_args &f, const int E, int32_t *ext, const int p, const int m, const int n, const int B,
                                                  const Bd2Gaps &g, const int Z, const int pen) {
    const int len = max(max(m, n), 0), L = min(len, B - 1);
    int best = 0, kb = 0, last = len, maxScore = 0, kmax = 0;
    bool dropped = false;
    for (int k = 1; k <= L; k++) {
        const int v = gap_of(g, k);
        if (v > best) {
            best = v;
            kb = k;
        } else if (ZDROP && best - v > Z + pen * (k - kb)) {
            last = k;
            dropped = true;
            break;
        }
    }
    const int seen = min(L, last); /* the computed cells are k = 0 .. seen */
    for (int k = 1; k <= seen; k++)
        if (gap_of(g, k) > maxScore) { maxScore = gap_of(g, k); kmax = k; }
    int qeScore = INT_MIN, qeCol = -1;
    if (m <= 0) { /* row m is row 0: the line itself (or the single cell (0, 0)) */
        qeScore = 0;
        qeCol = 0;
        for (int k = 1; k <= (n > 0 ? seen : 0); k++)
            if (gap_of(g, k) > qeScore) { qeScore = gap_of(g, k); qeCol = k; }
    } else if (m <= seen) { /* n == 0: row m holds the one cell (m, 0) */
        qeScore = gap_of(g, m);
        qeCol = 0;
    }
    write_results(f, E, ext, p, max(m, 0), maxScore, m > 0 ? kmax : 0, m > 0 ? 0 : kmax, qeScore, qeCol, last, dropped);
}

/* DPX_BDX_SCAN_AFTER of dpx_bdx_kernels.hip, over this kernel's names: after step A_, whose H values stand in st.prevH and whose first
 * slot is row i0, the row-m pick-up into the owning lane's (qeScore, qeCol), then (SCAN == 2) the anti-diagonal's maximum, its holder
 * with the smallest row and the drop test, which sets lastDiag and stop. */
#define DPX_BD2_SCAN_AFTER(A_)                                                                                            \
    if constexpr (SCAN > 0) {                                                                                             \
        const int a_ = (A_) + 2;                                                                                          \
        {                                                                                                                 \
            int pick_ = DPX_NEG;                                                                                          \
            const int cm_ = m - i0 - lane * C;                                                                            \
            _Pragma("unroll") for (int c = 0; c < C; c++) pick_ = (cm_ == c) ? st.prevH[c] : pick_;                       \
            const bool take_ = pick_ > qeScore;                                                                           \
            qeScore = take_ ? pick_ : qeScore;                                                                            \
            qeCol = take_ ? a_ - m : qeCol;                                                                               \
        }                                                                                                                 \
        if constexpr (SCAN == 2) {                                                                                        \
            int k_ = st.prevH[0];                                                                                         \
            _Pragma("unroll") for (int c = 1; c < C; c++) k_ = max(k_, st.prevH[c]);                                      \
            const int dm_ = wave_max_i32(k_);                                                                             \
            if (dm_ > DPX_NEG / 2) { /* (else: no cell on this anti-diagonal) */                                          \
                int ci_ = C;                                                                                              \
                _Pragma("unroll") for (int c = C - 1; c >= 0; c--) ci_ = (st.prevH[c] == dm_) ? c : ci_;                  \
                const int ln_ = __builtin_ctzll(__builtin_amdgcn_ballot_w64(ci_ < C));                                    \
                const int ia_ = i0 + ln_ * C + __builtin_amdgcn_readlane(ci_, ln_);                                       \
                if (zdrop_test(dm_, ia_, a_ - ia_, Z, pen, best, bi, bj)) {                                               \
                    lastDiag = a_;                                                                                        \
                    stop = true;                                                                                          \
                }                                                                                                         \
            }                                                                                                             \
        }                                                                                                                 \
    }

template <int C, bool PB, bool EXT, bool TABLE, int SCAN>
__global__ void __launch_bounds__(DPX_FILL_THREADS) k_bd2_fill(const dpx_bd2_args x) {
    static_assert(EXT || SCAN == 0, "BANW has no extension mode");
    static_assert(C == 1 || C == 2 || C == 4, "bands up to 256");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const dpx_fill_args &a = x.f;
    constexpr int Gd = 16 / C; /* steps per 16-byte store (a multiple of 4) */
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int p = blockIdx.x * (int)a.wavesPerBlock + wv;
    if (p >= a.numPairs) return;
    if (a.order) p = a.order[p];
    const dpx_pair_dev pr = a.pairs[p];
    const int n = pr.n, m = pr.m, B = a.band;
    const int match = a.match, mismatch = a.mismatch;
    const Bd2Gaps g = {a.gapOpen + a.gapExtend, a.gapExtend, x.gapOpen2 + x.gapExtend2, x.gapExtend2, a.gapOpen, x.gapOpen2};
    const int Z = x.zdrop, pen = max(0, -max(g.e1, g.e2));
    const int g1 = gap_of(g, 1);
    if (m <= 0 || n <= 0) { /* an empty sequence: no cell has a code and no diagonal step runs, so a table plays no part */
        if (lane == 0) {
            if constexpr (SCAN > 0) {
                scan_border_line2<SCAN == 2>(a, x.endBonus, x.ext, p, m, n, B, g, Z, pen);
            } else if constexpr (EXT) { /* the one border line carries g(k), convex in k: its first maximum is at k = 1 or at k = L */
                const int L = min(max(max(m, n), 0), B - 1);
                const int k = (L >= 1 && g1 >= gap_of(g, L)) ? 1 : L;
                const int v = k > 0 ? gap_of(g, k) : 0;
                const bool take = v > 0;
                a.score[p] = take ? v : 0;
                a.endRow[p] = (take && m > 0) ? k : 0;
                a.endCol[p] = (take && m <= 0) ? k : 0;
            } else {
                a.score[p] = (m > 0 || n > 0) ? gap_of(g, max(m, n)) : 0;
                a.endRow[p] = max(m, 0);
                a.endCol[p] = max(n, 0);
            }
        }
        return;
    }
    const unsigned char *ref = reinterpret_cast<const unsigned char *>(a.seq + pr.refIdx);
    const unsigned char *qry = reinterpret_cast<const unsigned char *>(a.seq + pr.qryIdx);
    /* the wave's LDS slice: [staged query][staged reference] and, TABLE, [table image]; a.ldsPerWave counts all of it */
    unsigned char *my = smem + (size_t)wv * a.ldsPerWave;
    const unsigned char *qL = stage_bytes(my, qry, m, lane, 64);
    const unsigned char *rL = stage_bytes(my + a.ldsRefOff, ref, n, lane, 64);
    const signed char *tabL = nullptr;
    const unsigned char *codeL = nullptr;
    if constexpr (TABLE) { /* (both arrays are 16-byte aligned: the host keeps them in one device allocation, the map behind the table) */
        unsigned char *img = my + (a.ldsPerWave - (uint32_t)DPX_SUBST_IMAGE_BYTES);
        reinterpret_cast<u32x4 *>(img)[lane] = reinterpret_cast<const u32x4 *>(x.table)[lane];
        if (lane < 16) reinterpret_cast<u32x4 *>(img + DPX_SUBST_TABLE_BYTES)[lane] = reinterpret_cast<const u32x4 *>(x.codeOf)[lane];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
        tabL = reinterpret_cast<const signed char *>(img);
        codeL = img + DPX_SUBST_TABLE_BYTES;
    }

    Bd2State<C> st;
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
            const int qb = qL[min(max(vi0 + s - 1, 0), m - 1)], rb = rL[min(max(vj0 - s - 1, 0), n - 1)];
            if constexpr (TABLE) {
                st.qch[c] = codeL[qb];
                st.rch[c] = (int)codeL[rb] << 5;
            } else {
                st.qch[c] = qb;
                st.rch[c] = rb;
            }
            const int bi0 = vi0 + s; /* the slot's cell on a = 1 is (bi0, 1 - bi0) */
            st.prevH[c] = (B >= 2 && (bi0 == 0 || bi0 == 1)) ? g1 : DPX_NEG;
            st.prev2H[c] = (s == ((B - 1) >> 1)) ? 0 : DPX_NEG;
            st.prevI1[c] = DPX_NEG;
            st.prevD1[c] = DPX_NEG;
            st.prevI2[c] = DPX_NEG;
            st.prevD2[c] = DPX_NEG;
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
    const int numGroups = (NS + Gd - 1) / Gd; /* == dpx_banddir2_chunks(m, n, B): no store goes past the pair's last chunk */
    unsigned char *base = reinterpret_cast<unsigned char *>(a.mat) + (size_t)pr.matOff * 2u;
    const uint64_t cs = (uint64_t)pr.chunkStride * 2u;
    int i0 = (1 + (B & 1) - (B - 1)) >> 1;
    int j0 = 1 - i0;
    /* the scan's state (k_bdx_fill's): (1, 0) is the only cell of row m that no step visits: in band when B >= 2, on anti-diagonal 1,
     * whose maximum g(1) sits at its smallest row, (0, 1) */
    int qeScore = (m == 1 && B >= 2) ? g1 : DPX_NEG / 2 /* (none yet: every cell is above it) */, qeCol = (m == 1 && B >= 2) ? 0 : -1;
    int best = 0, bi = 0, bj = 0, lastDiag = m + n;
    bool stop = false;
    if constexpr (SCAN == 2) {
        if (B >= 2 && zdrop_test(g1, 0, 1, Z, pen, best, bi, bj)) {
            lastDiag = 1;
            stop = true;
        }
    }
    auto store_group = [&](const int grp) {
        if (grp < numGroups)
            *reinterpret_cast<u32x4 *>(base + dpx_banddir_piece((uint64_t)grp, lane, cs)) = u32x4{st.w[0], st.w[1], st.w[2], st.w[3]};
    };
#define DPX_BD2_BODY(INTERIOR_)                                                                                                        \
    {                                                                                                                                  \
        bd2_step<C, EXT, TABLE, PB, INTERIOR_>(st, A0, i0, j0, lane, m, n, B, match, mismatch, g, cEnd, qL, rL, tabL, codeL);          \
        DPX_BD2_SCAN_AFTER(A0)                                                                                                         \
        if (stop) break; /* (a drop after the first step: the second does not run) */                                                  \
        bd2_step<C, EXT, TABLE, !PB, INTERIOR_>(st, A0 + 1, i0, j0, lane, m, n, B, match, mismatch, g, cEnd, qL, rL, tabL, codeL);     \
        DPX_BD2_SCAN_AFTER(A0 + 1)                                                                                                     \
        if (((A0 + 2) & (Gd - 1)) == 0) store_group((A0 + 1) / Gd);                                                                    \
        if (stop) break;                                                                                                               \
    }
    /* parity of step A is (A + B + 1) & 1; A0 is even, so even steps have parity PB and odd steps !PB.  k_bdir_fill's three phases
     * (head, interior, tail), each ending early on a drop.  When NS is odd the last pair of steps runs one step past NS - 1, which
     * holds no cell: its anti-diagonal is empty for the scan. */
    int A0 = 0;
    for (; !stop && A0 < NS && !(interior(A0) && interior(A0 + 1)); A0 += 2) DPX_BD2_BODY(false)
    for (; !stop && A0 + 2 < NS && interior(A0 + 1); A0 += 2) DPX_BD2_BODY(true)
    for (; !stop && A0 < NS; A0 += 2) DPX_BD2_BODY(false)
#undef DPX_BD2_BODY
    /* the partial last group, as in k_bdx_fill: `pushed` steps have entered the window, pushed % Gd of them since the last store; the
     * missing steps are shifted in as zeros so that step t of the group sits at byte t * C.  Without a drop the group is the pair's last
     * chunk, after one the chunk of the dropping step; a drop on anti-diagonal 1 ran no step and stores nothing. */
    const int pushed = stop ? lastDiag - 1 : A0;
    if (pushed & (Gd - 1)) {
        for (int t = pushed & (Gd - 1); t < Gd; t++) window_push<8 * C>(st.w, 0u);
        store_group(pushed / Gd);
    }
    if constexpr (!EXT) {
        if (cEnd >= 0) { a.score[p] = st.fin; a.endRow[p] = m; a.endCol[p] = n; }
    } else {
        /* the lane's candidate; across lanes max score, then min row, then min column.  A border slot decodes to i = 0 or j = 0.
         * (The border cells of anti-diagonal 1, which no step visits, need no candidate: they count only when g(1) > 0, and then the
         * pair cannot drop at anti-diagonal 1, so (1, 1) is computed and holds H >= 2 * g(1) > g(1).) */
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
        if constexpr (SCAN > 0) { /* row m: the highest score, then the smallest column */
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const int os = __shfl_xor(qeScore, off, 64), oc = __shfl_xor(qeCol, off, 64);
                if (os > qeScore || (os == qeScore && oc < qeCol)) { qeScore = os; qeCol = oc; }
            }
        }
        if (lane == 0) {
            const int maxRow = hv > 0 ? (int)(at >> 32) : 0, maxCol = hv > 0 ? (int)(at & 0xFFFFFFFFull) : 0;
            if constexpr (SCAN > 0) {
                write_results(a, x.endBonus, x.ext, p, m, max(hv, 0), maxRow, maxCol, qeCol >= 0 ? qeScore : INT_MIN, qeCol, lastDiag, stop);
            } else {
                a.score[p] = hv;
                a.endRow[p] = maxRow;
                a.endCol[p] = maxCol;
            }
        }
    }
}
#undef DPX_BD2_SCAN_AFTER

/* -----------------------------------------------------------------------------------------------------
 * Traceback: k_bdir_traceback over byte codes, five states.
 * ----------------------------------------------------------------------------------------------------- */
constexpr int kRing = 16;                                   /* chunks in LDS */
constexpr int kRingBytes = kRing * (int)DPX_BANDDIR_CHUNK_BYTES;

__global__ void __launch_bounds__(64) k_bd2_traceback(const dpx_fill_args a, int numPairs, const uint64_t *tbOff, char *tb, int32_t *tbLen) {
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
    const int sg = 4 - dpx_log2(dpx_band_cpl(B)); /* Gd = 2^sg */
    const int numChunks = (int)dpx_banddir2_chunks(m, n, B);
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
        const uint64_t off = dpx_banddir2_byte(ci, cj, B, DPX_BANDDIR_CHUNK_BYTES);
        return (int)ring[off & (uint64_t)(kRingBytes - 1)];
    };
    auto run_of = [&](const bool cont) -> int { /* leading lanes (from lane 0) whose condition holds */
        const unsigned long long mask = __ballot(cont);
        return ~mask == 0ull ? 64 : __builtin_ctzll(~mask);
    };
    auto put = [&](const int at, const int rc, const int xc, const int qc) { lr[at] = (char)rc; lx[at] = (char)xc; lq[at] = (char)qc; };
    int cur = 0; /* 0 SCORING, else the move number of the gap plane the walk stands in: 2 D1, 3 I1, 4 D2, 5 I2 */
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
        const int kind = cur != 0 ? cur : (c0 & 7);
        if (kind < 1 || kind > 5) break; /* (cannot happen: a stored cell has a move) */
        if (kind != 1) { /* a gap: step l is taken while the cells before it extend in this plane; the cell that opens ends it */
            const bool left = (kind & 1) != 0; /* 3, 5: along the row */
            const int bit = kind == 3 ? 8 : kind == 2 ? 16 : kind == 5 ? 32 : 64;
            const int c = left ? code(i, j - lane) : code(i - lane, j);
            const int k = run_of(c >= 0 && (c & bit));
            int steps = 64;
            cur = kind;
            if (k < 64) {
                const int ck = __shfl(c, k, 64);
                if (ck >= 0) { steps = k + 1; cur = 0; } /* cell k opened the gap */
                else steps = k;                          /* cell k lies below the ring (or off the stored cells): go on from it in the same state */
            }
            if (steps == 0) break; /* (cannot happen: lane 0's cell is c0) */
            if (lane < steps) {
                if (left) put(pos - 1 - lane, ref[j - 1 - lane], ' ', '_');
                else put(pos - 1 - lane, '_', ' ', qry[i - 1 - lane]);
            }
            pos -= steps;
            if (left) j -= steps; else i -= steps;
            continue;
        }
        /* the diagonal: step l leaves cell l of the walker's diagonal, which must itself say "diagonal" (lane 0 has said so) */
        const int c = lane == 0 ? c0 : code(i - lane, j - lane);
        const int steps = run_of(c >= 0 && (lane == 0 || (c & 7) == 1));
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

/* One pair's plane as the oracles write it (k_bdir_export's conventions): `which` 0 directionMain, 1 / 2 piece 1's I / D, 3 / 4 piece 2's
 * (directionIndel; I on the band's lower edge and D on its upper edge are GAP_OPEN by the geometry), 5 the piece of H's gap move. */
__global__ void __launch_bounds__(256) k_bd2_export(const unsigned char *codes, const dpx_pair_dev pr, const char *seq, int band, int which,
                                                    uint8_t *out) {
    const int n = pr.n, m = pr.m;
    const uint64_t total = (uint64_t)(m + 1) * (uint64_t)(n + 1);
    const bool iPlane = which == 1 || which == 3, dPlane = which == 2 || which == 4;
    for (uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * blockDim.x) {
        const int i = (int)(idx / (uint64_t)(n + 1)), j = (int)(idx % (uint64_t)(n + 1));
        uint8_t v = 0;
        if (in_band(i, j, band)) {
            if (i == 0 || j == 0) {
                v = (which != 0 || (i | j) == 0) ? 0 : (j == 0 ? 4 : 3); /* column 0: QUERY_DELETION, row 0: QUERY_INSERTION */
            } else if ((iPlane && i - j == band - 1) || (dPlane && j - i == band - 1)) {
                v = 1;
            } else {
                const int c = codes[(size_t)pr.matOff * 2u + dpx_banddir2_byte(i, j, band, (uint64_t)pr.chunkStride * 2u)];
                const int mv = c & 7;
                if (which == 1) v = (c & 8) ? 2 : 1;
                else if (which == 2) v = (c & 16) ? 2 : 1;
                else if (which == 3) v = (c & 32) ? 2 : 1;
                else if (which == 4) v = (c & 64) ? 2 : 1;
                else if (which == 5) v = (mv == 2 || mv == 3) ? 1 : (mv == 4 || mv == 5) ? 2 : 0;
                else v = (mv == 2 || mv == 4) ? 4 : (mv == 3 || mv == 5) ? 3 : (seq[pr.qryIdx + i - 1] == seq[pr.refIdx + j - 1] ? 1 : 2);
            }
        }
        out[idx] = v;
    }
}

/* (a direction batch sizes its LDS per wave, not as a four-wave request) */
template <class K>
hipError_t launch_bd2_kernel(K kernel, const dpx_bd2_args &x, hipStream_t s) {
    const unsigned wpb = x.f.wavesPerBlock ? x.f.wavesPerBlock : 1u;
    const size_t lds = (size_t)x.f.ldsPerWave * wpb;
    if (lds > 160u * 1024u) return hipErrorInvalidValue;
    if (lds > 64u * 1024u) { /* opt in to more than the default 64 KiB of dynamic LDS */
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const unsigned grid = ((unsigned)x.f.numPairs + wpb - 1) / wpb;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64u * wpb), lds, s, x);
    return hipGetLastError();
}

} // namespace

hipError_t dpx_launch_bd2_fill(const dpx_bd2_args &x, int C, bool ext, hipStream_t stream) {
    if (x.f.numPairs <= 0) return hipSuccess;
    const bool table = x.table != nullptr;
    const int scan = !ext ? 0 : x.zdrop >= 0 ? 2 : x.endBonus >= 0 ? 1 : 0;
    if ((table && !x.codeOf) || (scan && !x.ext) || x.f.band > DPX_BANDDIR2_MAX_BAND || C != dpx_band_cpl(x.f.band)) return hipErrorInvalidValue;
    const bool pb = ((x.f.band + 1) & 1) != 0; /* parity of step A = 0 */
    return dpx_dev::dispatch_int<1, 2, 4>(C, [&](auto c) {
        return dpx_dev::dispatch_bool(pb, [&](auto pbc) {
            return dpx_dev::dispatch_bool(table, [&](auto tb) {
                constexpr int kC = decltype(c)::value;
                constexpr bool kPB = decltype(pbc)::value, kTable = decltype(tb)::value;
                if (!ext) return launch_bd2_kernel(k_bd2_fill<kC, kPB, false, kTable, 0>, x, stream);
                if (scan == 2) return launch_bd2_kernel(k_bd2_fill<kC, kPB, true, kTable, 2>, x, stream);
                if (scan == 1) return launch_bd2_kernel(k_bd2_fill<kC, kPB, true, kTable, 1>, x, stream);
                return launch_bd2_kernel(k_bd2_fill<kC, kPB, true, kTable, 0>, x, stream);
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
