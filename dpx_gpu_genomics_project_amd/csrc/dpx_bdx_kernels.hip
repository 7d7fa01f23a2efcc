/*
 * dpx_bdx_kernels.hip -- banded direction batches (DPX_KEEP_BAND_DIRECTIONS) of BANW and BAXT under dpx_batch_set_direction_scoring for
 * gfx950: the fill, k_bdx_fill<C, PB, EXT, TABLE, SCAN>, and nothing else.  The walk and the export are dpx_banddir_kernels.hip's
 * (k_bdir_traceback follows stored codes and never scores a cell; the relation line and the H plane's MATCH / MISMATCH are byte
 * equality whatever scored the cell), and the host masks the exported planes behind the pair's last anti-diagonal.
 *
 * The kernel is k_bdir_fill's: its step (int32 cells, the code of dpx_dir.h from the recurrence's own compares), its schedule and
 * phases, its 128-bit code window with one 16-byte store per Gd = 32 / C steps, and its per-lane (H, row, step) tracker of the first
 * maximum in row-major order.  That unit stays as it is (regrouping shared code moves the compiled fills, dpx_band_affine.hpp), so the
 * step and window_push are copied here, not moved.  What is new:
 *   TABLE  the diagonal term is table[(codeOf[ref byte] << 5) + codeOf[qry byte]]: table and map lie in the wave's LDS slice behind the
 *          staged strings, a character is translated once as it enters its window, and the C byte reads of a step are issued before
 *          the first is used (subst_step's scheme).
 *   SCAN   BAXT's extension mode, the definition of k_zext_fill / k_zsub_fill over the same cells: 1 = the row-m pick-up, the record and
 *          the end-bonus choice; 2 = also the per-anti-diagonal drop test.  zdrop_test, write_results and scan_border_line are the
 *          shared ones.  Nothing of the int16 kernels' packed keys is used: scores reach 2^28 here and m + n passes 65 535.
 *            - the anti-diagonal's maximum is one wave_max_i32 of H (a slot without a cell holds DPX_NEG; a maximum at or below
 *              DPX_NEG / 2 means an empty anti-diagonal);
 *            - its holder with the smallest row: rows grow with the slot index, so it is the lowest lane, and in it the lowest register,
 *              whose H equals the maximum -- a ballot, a count of trailing zeros and one v_readlane;
 *            - row m's cells arrive in column order: "strictly greater replaces" on (score, column), kept by the lane that owns the
 *              cell's slot and reduced across lanes at the end (highest score, then smallest column);
 *            - the maximum cell is the tracker's, which the step updates before the test: it counts the dropping anti-diagonal and
 *              nothing after it.
 *          best, bi, bj, lastDiag and stop are wave-uniform.
 * EXT = 0 (BANW) takes TABLE = 1, SCAN = 0 only; EXT = 1 every (TABLE, SCAN) but (0, 0), which is k_bdir_fill: 6 modes x 4 C x 2 parities.
 *
 * Scalar registers.  At C = 8 the step alone takes most of the 102 scalar registers (every cell of a border step makes several compare
 * masks), and the scan's state is scalar too.  As a scalar pair behind a wave-uniform branch with one v_readlane, the row-m pick-up
 * made the C = 8 fills without the drop test 198 VGPRs wide; branch-free and per lane it costs two VGPRs.  How the owning register is
 * selected then decides between scalar spills to VGPR lanes only and a scratch frame, so DPX_BDX_SCAN_AFTER has two forms of one
 * function of the same values.  What each form compiled to at C = 8 (private_segment_fixed_size in bytes; every other instantiation
 * had none under any form; <C, PB, EXT, TABLE, SCAN>):
 *   (a) the per-lane register index m - i0 - lane * C compared with c, no geometry test -- used when SCAN == 1: no scratch there;
 *       with SCAN == 2: <8, 1, 1, 0, 2> 20 bytes, <8, 0, 1, 1, 2> 36 bytes
 *   (b) the wave-uniform index (m - i0) % C compared with c, a lane compare, and the geometry test of DPX_BAND_SCAN_AFTER, which (a)
 *       shows to be redundant -- used when SCAN == 2: no scratch there; with SCAN == 1: <8, 1, 1, 1, 1> and <8, 1, 1, 0, 1> 36 bytes
 *   (b) without the geometry test, with SCAN == 2: <8, 1, 1, 1, 2> 36 bytes
 * The frame is never accessed in any of these (the scalar spills go to VGPR lanes), but a kernel with one is launched with scratch.
 * Below C = 8 either form is safe to use for both modes; at C = 8 a change to this text, or a compiler update, has to be checked against
 * tests/test_bdx_kernels_isa.py, which holds all 48 instantiations to zero scratch.
 *
 * A drop.  The loop body runs two steps; a drop after the first does not run the second.  The window then holds a partial group: the
 * missing steps are shifted in as zeros and the group goes to chunk (lastDiag - 2) / Gd (the chosen end cell may lie in it), not to the
 * pair's last chunk.  A drop on anti-diagonal 1 stores nothing.  Nothing is stored past the drop: the chunks behind it keep what the
 * pool held, and no walk reads them (a walk only visits smaller anti-diagonals than its start).
 */
#include "dpx_band_affine.hpp"
#include "dpx_banddir.h"

namespace {

using namespace dpx_band;

template <int C>
struct BdxState {
    int prevH[C], prev2H[C]; /* H on anti-diagonals a-1 and a-2 */
    int prevI[C], prevD[C];  /* I and D on anti-diagonal a-1 */
    int qch[C], rch[C];      /* query / reference character of each slot's cell (TABLE: query code / reference code << 5) */
    long long bestKey;       /* EXT: the lane's running maximum of (H << 32 | ~row), signed: the highest H, then the smallest row ... */
    int bestA;               /* ... and the step of its first occurrence (the smallest column of that row) */
    int lim;                 /* B-1 - lane*C: slot c is inside the band on a step of parity p when c + p <= lim */
    int fin;                 /* !EXT: H[m][n], picked up on the last anti-diagonal by the lane that owns its slot */
    uint32_t w[4];           /* the code window: 32 nibbles, the oldest step lowest */
};

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

/* one anti-diagonal: bdir_step with the diagonal term from the table when TABLE.  INTERIOR: every in-band slot lies inside the matrix,
 * so validity is one compare against the per-lane constant `lim`; no border slot and not the last anti-diagonal */
template <int C, bool EXT, bool TABLE, bool P1, bool INTERIOR>
__device__ __forceinline__ void bdx_step(BdxState<C> &st, const int A, int &i0, int &j0, const int lane, const int m, const int n,
                                         const int B, const int match, const int mismatch, const int o, const int oe, const int e,
                                         const int cEnd, const unsigned char *qL, const unsigned char *rL, const signed char *tabL,
                                         const unsigned char *codeL) {
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
    uint32_t word = 0u;
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
        /* the definition's order: D >= diag takes the move, then I >= the winner takes it from either; sign bits of differences (every
         * operand lies within +-2^30, so no difference wraps) */
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

/* after step A_, whose H values stand in st.prevH and whose first slot is row i0: the row-m pick-up into the owning lane's (qeScore,
 * qeCol) -- no branch and no readlane, so that the body of two steps stays straight-line code as k_bdir_fill's is -- then (SCAN == 2) the anti-diagonal's maximum, its holder with the smallest row and the drop test, which sets lastDiag and stop.  A macro
 * over the kernel's own names, as DPX_BAND_SCAN_AFTER is (as a function taking the state by reference that text cost registers). */
#define DPX_BDX_SCAN_AFTER(A_)                                                                                            \
    if constexpr (SCAN > 0) {                                                                                             \
        const int a_ = (A_) + 2;                                                                                          \
        { /* row m on this step is slot m - i0: register (m - i0) % C of lane (m - i0) / C.  A slot holds a cell of the       */ \
          /* matrix (a border cell included) exactly when its H is not DPX_NEG, so no geometry is tested: a lane that does    */ \
          /* not own the slot, or an empty slot, offers DPX_NEG, which is below every qeScore.  (The two forms, and the        */ \
          /* redundant geometry test of the second: see "Scalar registers" at the top.)                                      */ \
            int pick_ = DPX_NEG;                                                                                          \
            if constexpr (SCAN == 2) {                                                                                    \
                const int sm_ = m - i0;                                                                                   \
                _Pragma("unroll") for (int c = 0; c < C; c++) pick_ = ((sm_ & (C - 1)) == c) ? st.prevH[c] : pick_;       \
                const bool on_ = a_ >= m && a_ - m <= n && abs(2 * m - a_) <= B - 1;                                      \
                pick_ = (on_ && lane == (sm_ >> kLogC)) ? pick_ : DPX_NEG;                                                \
            } else {                                                                                                      \
                const int cm_ = m - i0 - lane * C;                                                                        \
                _Pragma("unroll") for (int c = 0; c < C; c++) pick_ = (cm_ == c) ? st.prevH[c] : pick_;                   \
            }                                                                                                             \
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
__global__ void __launch_bounds__(DPX_FILL_THREADS) k_bdx_fill(const dpx_bdx_args x) {
    static_assert(EXT ? (TABLE || SCAN > 0) : (TABLE && SCAN == 0), "BANW: a table only; BAXT: every mode but none");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const dpx_fill_args &a = x.f;
    constexpr int Gd = 32 / C; /* steps per 16-byte store (a multiple of 4) */
    constexpr int kLogC = C == 8 ? 3 : C == 4 ? 2 : C == 2 ? 1 : 0;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int p = blockIdx.x * (int)a.wavesPerBlock + wv;
    if (p >= a.numPairs) return;
    if (a.order) p = a.order[p];
    const dpx_pair_dev pr = a.pairs[p];
    const int n = pr.n, m = pr.m, B = a.band;
    const int match = a.match, mismatch = a.mismatch, o = a.gapOpen, e = a.gapExtend, oe = a.gapOpen + a.gapExtend;
    const int Z = x.zdrop, pen = e < 0 ? -e : 0;
    if (m <= 0 || n <= 0) { /* an empty sequence: no cell has a code and no diagonal step runs, so a table plays no part */
        if (lane == 0) {
            if constexpr (SCAN > 0) {
                scan_border_line<SCAN == 2>(a, x.endBonus, x.ext, p, m, n, B, o, e, Z, pen);
            } else if constexpr (EXT) { /* k_bdir_fill's: the first maximum of the one border line, when it is above the 0 of (0, 0) */
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

    BdxState<C> st;
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
            st.prevH[c] = (B >= 2 && (bi0 == 0 || bi0 == 1)) ? oe : DPX_NEG;
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
    /* the scan's state.  Row m: every lane keeps (score, column) of the row-m cells its own slots held, replaced when strictly greater
     * (a lane meets them in column order), reduced across lanes at the end; (1, 0) is the only cell of row m that no step visits: in
     * band when B >= 2, on anti-diagonal 1.  That anti-diagonal is non-empty when B >= 2, and its maximum o + e sits at its smallest
     * row, (0, 1) */
    int qeScore = (m == 1 && B >= 2) ? oe : DPX_NEG / 2 /* (none yet: every cell is above it) */, qeCol = (m == 1 && B >= 2) ? 0 : -1;
    int best = 0, bi = 0, bj = 0, lastDiag = m + n;
    bool stop = false;
    if constexpr (SCAN == 2) {
        if (B >= 2 && zdrop_test(oe, 0, 1, Z, pen, best, bi, bj)) {
            lastDiag = 1;
            stop = true;
        }
    }
    auto store_group = [&](const int grp) {
        if (grp < numGroups)
            *reinterpret_cast<u32x4 *>(base + dpx_banddir_piece((uint64_t)grp, lane, cs)) = u32x4{st.w[0], st.w[1], st.w[2], st.w[3]};
    };
#define DPX_BDX_BODY(INTERIOR_)                                                                                                        \
    {                                                                                                                                  \
        bdx_step<C, EXT, TABLE, PB, INTERIOR_>(st, A0, i0, j0, lane, m, n, B, match, mismatch, o, oe, e, cEnd, qL, rL, tabL, codeL);   \
        DPX_BDX_SCAN_AFTER(A0)                                                                                                         \
        if (stop) break; /* (a drop after the first step: the second does not run) */                                                  \
        bdx_step<C, EXT, TABLE, !PB, INTERIOR_>(st, A0 + 1, i0, j0, lane, m, n, B, match, mismatch, o, oe, e, cEnd, qL, rL, tabL, codeL); \
        DPX_BDX_SCAN_AFTER(A0 + 1)                                                                                                     \
        if (((A0 + 2) & (Gd - 1)) == 0) store_group((A0 + 1) / Gd);                                                                    \
        if (stop) break;                                                                                                               \
    }
    /* parity of step A is (A + B + 1) & 1; A0 is even, so even steps have parity PB and odd steps !PB.  k_bdir_fill's three phases
     * (head, interior, tail), each ending early on a drop.  When NS is odd the last pair of steps runs one step past NS - 1, which
     * holds no cell: its anti-diagonal is empty for the scan. */
    int A0 = 0;
    for (; !stop && A0 < NS && !(interior(A0) && interior(A0 + 1)); A0 += 2) DPX_BDX_BODY(false)
    for (; !stop && A0 + 2 < NS && interior(A0 + 1); A0 += 2) DPX_BDX_BODY(true)
    for (; !stop && A0 < NS; A0 += 2) DPX_BDX_BODY(false)
#undef DPX_BDX_BODY
    /* the partial last group.  `pushed` steps have entered the window, pushed % Gd of them since the last store (a drop on step A left
     * lastDiag = A + 2; a group that the dropping step completed has been stored already); the missing steps are shifted in as zeros
     * so that step t of the group sits at nibble t * C.  Without a drop the group is the pair's last chunk, after one the chunk of the
     * dropping step; a drop on anti-diagonal 1 ran no step and stores nothing. */
    const int pushed = stop ? lastDiag - 1 : A0;
    if (pushed & (Gd - 1)) {
        for (int t = pushed & (Gd - 1); t < Gd; t++) window_push<4 * C>(st.w, 0u);
        store_group(pushed / Gd);
    }
    if constexpr (!EXT) {
        if (cEnd >= 0) { a.score[p] = st.fin; a.endRow[p] = m; a.endCol[p] = n; }
    } else {
        /* the lane's candidate; across lanes max score, then min row, then min column.  A border slot decodes to i = 0 or j = 0.
         * (The border cells of anti-diagonal 1, which no step visits, need no candidate: they count only when o + e > 0, and then the
         * pair cannot drop at anti-diagonal 1, so (1, 1) is computed and holds H >= 2 * (o + e) > o + e.) */
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
#undef DPX_BDX_SCAN_AFTER

/* (a direction batch sizes its LDS per wave, not as a four-wave request) */
template <class K>
hipError_t launch_bdx_kernel(K kernel, const dpx_bdx_args &x, hipStream_t s) {
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

hipError_t dpx_launch_bdx_fill(const dpx_bdx_args &x, int C, bool ext, hipStream_t stream) {
    if (x.f.numPairs <= 0) return hipSuccess;
    const bool table = x.table != nullptr;
    const int scan = !ext ? 0 : x.zdrop >= 0 ? 2 : x.endBonus >= 0 ? 1 : 0;
    if ((table && !x.codeOf) || (scan && !x.ext) || (!table && !scan)) return hipErrorInvalidValue;
    return dispatch_fill(C, x.f.band, table, [&](auto c, auto pb, auto tb) {
        constexpr int kC = decltype(c)::value;
        constexpr bool kPB = decltype(pb)::value, kTable = decltype(tb)::value;
        if (!ext) {
            if constexpr (kTable) return launch_bdx_kernel(k_bdx_fill<kC, kPB, false, true, 0>, x, stream);
            else return hipErrorInvalidValue;
        }
        if (scan == 2) return launch_bdx_kernel(k_bdx_fill<kC, kPB, true, kTable, 2>, x, stream);
        if (scan == 1) return launch_bdx_kernel(k_bdx_fill<kC, kPB, true, kTable, 1>, x, stream);
        if constexpr (kTable) return launch_bdx_kernel(k_bdx_fill<kC, kPB, true, true, 0>, x, stream);
        else return hipErrorInvalidValue;
    });
}
