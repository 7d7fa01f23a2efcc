/*
 * dpx_band_affine.hpp -- what the banded affine-gap units without a zero floor share: dpx_banw_kernels.hip (BANW), dpx_baxt_kernels.hip
 * (BAXT), dpx_zext_kernels.hip (BAXT in extension mode), dpx_subst_kernels.hip (either, scored by a table), dpx_zsub_kernels.hip (BAXT in
 * extension mode, scored by a table) and, through dpx_banddir_dev.hpp, the three band-direction units (dpx_banddir_kernels.hip,
 * dpx_bdx_kernels.hip, dpx_bd2_kernels.hip: either algorithm, storing direction codes; what those three share among themselves is in
 * dpx_banddir_dev.hpp and dpx_banddir_fill.inc).  dpx_basw_kernels.hip, whose step has a zero floor and a start cell, is a different kernel and does
 * not include it.  Everything here is a __forceinline__ function or a template: each kernel stays in its own unit under its own name.
 *
 * Shared are end_key, the band geometry and BandView, the step of the two fills that track slot keys (slot_key_step: k_baxt_fill and
 * k_zext_fill), the step under a table (subst_step: k_subst_fill and k_zsub_fill), the scan of extension mode (wave_max_i32, zdrop_test,
 * write_results, scan_border_line, DPX_BAND_SCAN_AFTER, scan_finish: k_zext_fill and k_zsub_fill) and both walks over the stored planes
 * as templates on a Scorer (band_walk_lane, band_walk_wave: BANW's with the byte compare, the substitution walks with the table).  The helpers of every family (stage_bytes, store8, wave_max_u64, CharWin) and the
 * launch helper and dispatcher of every fill (launch_fill, dispatch_fill) come from dpx_device.hpp under their old names.
 *
 * NOT shared is one step for all fills.  band_step<C, P1, INTERIOR, Scorer, Tracker> over shared geometry / slide-and-gather / select
 * pieces, a shared prologue and shared phase loops computed every value the five steps compute and left every GPU test passing, but
 * the compiler's code for these kernels moves with any change of how the same operations are grouped into functions, and against
 * the build before (4096 x 4096, 5 fresh processes per library alternating, rule: median <= the old median + the old max - min) the
 * fills at one and two cells per lane lost: k_baxt_fill +4.2 % at band 128, k_zext_fill +1.1 % at band 64, k_subst_fill<EXT> +3.2 % at
 * band 128, k_bdir_fill<EXT> +1.1 % at band 64 and +0.7 % at band 256 (k_banw_fill +3.6 % at band 128, inside a 5 % spread); with the
 * phase loops as a function template over step and trip callables, 7 to 9 % at band 128.  (In the interior loop the wait for the
 * character read from LDS came 6 instructions behind the read instead of 12.)  So every fill keeps the step, prologue and loops it
 * had, and with them the code it compiled to before; profiles/band_sharing_ab.md has the table.  What does not move a fill is text
 * included inside the kernel itself: the band-direction fills share their frame that way (dpx_banddir_fill.inc,
 * profiles/banddir_sharing_ab.md) and keep three steps.
 *
 * The recurrence is ANW's Gotoh recurrence restricted to the band |i-j| <= B-1, border cells included: H[0][0] = 0, the in-band border
 * cells carry H = gapOpen + k * gapExtend (k <= B-1), everything outside the band is -infinity (DPX_NEG) in H, I and D; no zero floor.
 * The schedule: the wave walks anti-diagonals a = i+j, step A holds a = A + 2, slot s = (i-j+B-1)>>1, lane l owns the C = ceil(B/64)
 * slots [l*C, l*C+C); on step A slot s holds the cell (i0 + s, j0 - s).  With p = (a+B-1)&1
 *       p=1: up = prev[s], left = prev[s+1]        p=0: up = prev[s-1], left = prev[s]
 * and a step moves two values with DPP: H and I (wave_shl:1) on a p=1 step, H and D (wave_shr:1) on a p=0 step.  The lane that has no
 * neighbour receives DPX_NEG for both.  A slot that holds no cell hands H = I = D = DPX_NEG to the next step, except the (at most
 * two) slots of an anti-diagonal a <= B-1 that are the in-band border cells (0, a) and (a, 0): they hand on H = gapOpen + a * gapExtend.
 * Such slots exist only while slot 0 is above row 1, that is in the head phase.
 */
#ifndef DPX_BAND_AFFINE_HPP
#define DPX_BAND_AFFINE_HPP

#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include <type_traits>

#include "dpx_device.hpp"
#include "dpx_kernels.h"
#include "dpx_layout.h"
#include "dpx_prims.hpp"
#include "dpx_table_dev.hpp"

namespace dpx_band {

using dpx::pack_lo16;
using dpx::wave_shl1;
using dpx::wave_shr1;

using dpx_dev::bool_c;
using dpx_dev::CharWin;
using dpx_dev::dispatch_fill;
using dpx_dev::int_c;
using dpx_dev::launch_fill;
using dpx_dev::stage_bytes;
using dpx_dev::store8;
using dpx_dev::u32x4;
using dpx_dev::wave_max_u64;
using dpx_table::table_stage_rows;

/* (score, min row, min column) as one unsigned key; score > 0 */
__device__ __forceinline__ unsigned long long end_key(const int hv, const int i, const int j) {
    return ((unsigned long long)(unsigned)hv << 40) | ((unsigned long long)(0xFFFFFu - (unsigned)i) << 20) |
           (unsigned long long)(0xFFFFFu - (unsigned)j);
}

/* ---- geometry shared by the exports and the walks.  A cell (i, j), borders included, is in the band when |i - j| <= B-1; the fill stores
 * the in-band cells with i, j >= 1; I on the lower edge and D on the upper edge are -infinity whatever the fill stored there ---- */
__device__ __forceinline__ bool in_band(const int i, const int j, const int band) {
    const int dlt = i - j;
    return dlt <= band - 1 && -dlt <= band - 1;
}
__device__ __forceinline__ bool cell_in_band(const int i, const int j, const int band) { /* ... and has storage */
    return i >= 1 && j >= 1 && in_band(i, j, band);
}
/* H of the in-band border cell (i, j), i == 0 or j == 0 */
__device__ __forceinline__ int border(const int i, const int j, const int o, const int e) { return (i | j) == 0 ? 0 : o + (i + j) * e; }
/* is `plane` of the stored cell (i, j) minus infinity? */
__device__ __forceinline__ bool edge(const int i, const int j, const int band, const int plane) {
    return (plane == 1 && i - j == band - 1) || (plane == 2 && j - i == band - 1);
}

/* one pair's three stored planes */
struct BandView {
    const int16_t *mat;
    uint64_t off;
    uint32_t cs;
    int band, o, e;
    /* a stored cell, or (plane 0) an in-band border cell */
    __device__ __forceinline__ int get(int i, int j, int plane) const {
        if (i == 0 || j == 0) return plane == 0 ? border(i, j, o, e) : DPX_NEG;
        if (edge(i, j, band, plane) || !in_band(i, j, band)) return DPX_NEG;
        return (int)mat[off + dpx_band_plane_index(i, j, band, plane, cs)];
    }
};

/* ---------------------------------------------------------- scorers ----------------------------------------------------------
 * The diagonal term.  q() / r() translate a query / reference byte once, when it enters a character window; at() scores a pair of
 * translated characters.  kTable: the score is a table read (the fill issues all C reads of a step before the first use). */
struct ByteScorer {
    static constexpr bool kTable = false;
    int match, mismatch;
    __device__ __forceinline__ int q(const int byte) const { return byte; }
    __device__ __forceinline__ int r(const int byte) const { return byte; }
    __device__ __forceinline__ int at(const int qv, const int rv) const { return qv == rv ? match : mismatch; }
};
/* s(r, q) = tab[code[r] * 32 + code[q]]: the window registers hold the query code as it is and the reference code as code << 5, so a
 * cell's score is one address add and one signed-byte read (codes are < 32: the address stays inside the 1-KiB table) */
struct TableScorer {
    static constexpr bool kTable = true;
    const signed char *tab;
    const unsigned char *code;
    __device__ __forceinline__ int q(const int byte) const { return code[byte]; }
    __device__ __forceinline__ int r(const int byte) const { return (int)code[byte] << 5; }
    __device__ __forceinline__ int at(const int qv, const int rv) const { return (int)tab[rv + qv]; }
};

/* ---- the step of k_baxt_fill and k_zext_fill (the latter had a copy of it); the key is explained in dpx_baxt_kernels.hip ---- */
template <int C>
struct SlotKeyState {
    int prevH[C], prev2H[C]; /* H on anti-diagonals a-1 and a-2 */
    int prevI[C], prevD[C];  /* I and D on anti-diagonal a-1 */
    int qch[C], rch[C];      /* query / reference character of each slot's cell */
    int key[C];              /* running signed max of (H << 16 | 0xFFFF - A): max score, then earliest step */
    int lim;                 /* B-1 - lane*C: slot c is inside the band on a step of parity p when c + p <= lim */
};

/* INTERIOR: every in-band slot of this anti-diagonal lies inside the matrix, so validity is one compare against the per-lane
 * constant `lim` instead of two against the step's slot window, and there is no border slot */
template <int C, bool P1, bool INTERIOR>
__device__ __forceinline__ void slot_key_step(SlotKeyState<C> &st, const int A, int &i0, int &j0, const int lane, const int m, const int n,
                                              const int B, const int match, const int mismatch, const int o, const int oe, const int e,
                                              const unsigned char *qL, const unsigned char *rL, int *outH, int *outI, int *outD) {
    const int p = P1 ? 1 : 0;
    if constexpr (P1) i0++; else j0++;
    const int smin = INTERIOR ? 0 : max(max(1 - i0, j0 - n), 0);
    const int smax = INTERIOR ? 0 : min(min(m - i0, j0 - 1), B - 1 - p);
    /* the in-band border cells of this anti-diagonal: (0, a) in slot -i0 and (a, 0) in slot j0, both H = o + a * e, while a <= B-1 */
    const int a = A + 2;
    const int bord = (INTERIOR || a > B - 1) ? DPX_NEG : o + a * e;
    const int sTop = (INTERIOR || a > n) ? -1 : -i0, sLeft = (INTERIOR || a > m) ? -1 : j0;
    const int lo = smin - lane * C, cnt = max(smax - smin + 1, 0), cTop = sTop - lane * C, cLeft = sLeft - lane * C;
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
    const int negA = 0xFFFF - A;
#pragma unroll
    for (int c = 0; c < C; c++) {
        const int sc = (st.qch[c] == st.rch[c]) ? match : mismatch;
        int d = max(upH[c] + oe, upD[c] + e);
        int ii = max(leftH[c] + oe, leftI[c] + e);
        int h = max(max(d, ii), st.prev2H[c] + sc); /* (no floor; the diagonal neighbour of an in-band cell is in band, so h is finite) */
        if constexpr (INTERIOR) {
            const bool valid = (c + p) <= st.lim;
            h = valid ? h : DPX_NEG;
            d = valid ? d : DPX_NEG;
            ii = valid ? ii : DPX_NEG;
        } else {
            /* slot lane * C + c against the step's window [smin, smax] and its two border slots, as compares of the constant c with
             * per-lane values: one unsigned range compare (cnt = 0 when the window is empty) */
            const bool valid = (unsigned)(c - lo) < (unsigned)cnt;
            h = valid ? h : ((c == cTop || c == cLeft) ? bord : DPX_NEG);
            d = valid ? d : DPX_NEG;
            ii = valid ? ii : DPX_NEG;
        }
        st.key[c] = max(st.key[c], (int)(((unsigned)h << 16) | (unsigned)negA)); /* (after the border select: border cells take part) */
        st.prev2H[c] = st.prevH[c];
        st.prevH[c] = h;
        st.prevI[c] = ii;
        st.prevD[c] = d;
        outH[c] = h;
        outI[c] = ii;
        outD[c] = d;
    }
}

/* ---- the step of k_subst_fill and k_zsub_fill: slot_key_step / banw_step with the table lookup ---- */
template <int C, bool EXT>
struct SubstState {
    int prevH[C], prev2H[C]; /* H on anti-diagonals a-1 and a-2 */
    int prevI[C], prevD[C];  /* I and D on anti-diagonal a-1 */
    int qcd[C], rcd[C];      /* query code / reference code << 5 of each slot's cell */
    int key[EXT ? C : 1];    /* EXT: running signed max of (H << 16 | 0xFFFF - A): max score, then earliest step */
    int lim;                 /* B-1 - lane*C: slot c is inside the band on a step of parity p when c + p <= lim */
    int fin;                 /* !EXT: H[m][n], picked up on the last anti-diagonal by the lane that owns its slot */
};

/* banw_step / slot_key_step with the table lookup.  INTERIOR: every in-band slot of this anti-diagonal lies inside the matrix, so validity
 * is one compare against the per-lane constant `lim`; no border slot and (!EXT) not the last anti-diagonal */
template <int C, bool P1, bool INTERIOR, bool EXT>
__device__ __forceinline__ void subst_step(SubstState<C, EXT> &st, const int A, int &i0, int &j0, const int lane, const int m, const int n,
                                           const int B, const int o, const int oe, const int e, const int cEnd, const unsigned char *qL,
                                           const unsigned char *rL, const signed char *tabL, const unsigned char *codeL, int *outH,
                                           int *outI, int *outD) {
    const int p = P1 ? 1 : 0;
    if constexpr (P1) i0++; else j0++;
    const int smin = INTERIOR ? 0 : max(max(1 - i0, j0 - n), 0);
    const int smax = INTERIOR ? 0 : min(min(m - i0, j0 - 1), B - 1 - p);
    /* the in-band border cells of this anti-diagonal: (0, a) in slot -i0 and (a, 0) in slot j0, both H = o + a * e, while a <= B-1 */
    const int a = A + 2;
    const int bord = (INTERIOR || a > B - 1) ? DPX_NEG : o + a * e;
    const int sTop = (INTERIOR || a > n) ? -1 : -i0, sLeft = (INTERIOR || a > m) ? -1 : j0;
    const int lo = smin - lane * C, cnt = max(smax - smin + 1, 0), cTop = sTop - lane * C, cLeft = sLeft - lane * C;
    const bool last = !EXT && !INTERIOR && a == m + n;
    int upH[C], upD[C], leftH[C], leftI[C];
    if constexpr (P1) {
        const int newq = codeL[INTERIOR ? qL[i0 + 64 * C - 2] : qL[min(max(i0 + 64 * C - 2, 0), m - 1)]];
        const int tq = wave_shl1(st.qcd[0], newq);
#pragma unroll
        for (int c = 0; c < C - 1; c++) st.qcd[c] = st.qcd[c + 1];
        st.qcd[C - 1] = tq;
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
        const int newr = (int)codeL[INTERIOR ? rL[j0 - 1] : rL[min(max(j0 - 1, 0), n - 1)]] << 5;
        const int tr = wave_shr1(st.rcd[C - 1], newr);
#pragma unroll
        for (int c = C - 1; c > 0; c--) st.rcd[c] = st.rcd[c - 1];
        st.rcd[0] = tr;
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
    int sc[C]; /* all C byte reads are in flight before the first is used (codes are < 32: the address stays inside the 1-KiB table) */
#pragma unroll
    for (int c = 0; c < C; c++) sc[c] = (int)tabL[st.rcd[c] + st.qcd[c]];
    const int negA = 0xFFFF - A;
#pragma unroll
    for (int c = 0; c < C; c++) {
        int d = max(upH[c] + oe, upD[c] + e);
        int ii = max(leftH[c] + oe, leftI[c] + e);
        int h = max(max(d, ii), st.prev2H[c] + sc[c]); /* (no floor; the diagonal neighbour of an in-band cell is in band, so h is finite) */
        if constexpr (INTERIOR) {
            const bool valid = (c + p) <= st.lim;
            h = valid ? h : DPX_NEG;
            d = valid ? d : DPX_NEG;
            ii = valid ? ii : DPX_NEG;
        } else {
            /* slot lane * C + c against the step's window [smin, smax] and its two border slots, as compares of the constant c with
             * per-lane values: one unsigned range compare (cnt = 0 when the window is empty) */
            const bool valid = (unsigned)(c - lo) < (unsigned)cnt;
            h = valid ? h : ((c == cTop || c == cLeft) ? bord : DPX_NEG);
            d = valid ? d : DPX_NEG;
            ii = valid ? ii : DPX_NEG;
            if constexpr (!EXT) st.fin = (last && c == cEnd) ? h : st.fin;
        }
        if constexpr (EXT) st.key[c] = max(st.key[c], (int)(((unsigned)h << 16) | (unsigned)negA)); /* (after the border select: border cells take part) */
        st.prev2H[c] = st.prevH[c];
        st.prevH[c] = h;
        st.prevI[c] = ii;
        st.prevD[c] = d;
        outH[c] = h;
        outI[c] = ii;
        outD[c] = d;
    }
}

/* ---- the scan of extension mode, after every step of k_zext_fill and k_zsub_fill ---- */
/* the signed maximum over the 64 lanes, on the VALU: row_shr 1, 2, 4, 8 bring each row's maximum to its lane 15, row_bcast:15 and
 * row_bcast:31 carry it on to lane 63.  A lane without a source keeps INT_MIN.  All 64 lanes must be active. */
template <int CTRL, int ROWS>
__device__ __forceinline__ int dpp_max(const int v) {
    return max(v, __builtin_amdgcn_update_dpp(INT_MIN, v, CTRL, ROWS, 0xf, false));
}
__device__ __forceinline__ int wave_max_i32(int v) {
    v = dpp_max<0x111, 0xf>(v);
    v = dpp_max<0x112, 0xf>(v);
    v = dpp_max<0x114, 0xf>(v);
    v = dpp_max<0x118, 0xf>(v);
    v = dpp_max<0x142, 0xa>(v);
    v = dpp_max<0x143, 0xc>(v);
    return __builtin_amdgcn_readlane(v, 63);
}

/* the scan's update-or-drop rule for one non-empty anti-diagonal whose maximum dm sits at (ia, ja); true = the pair is dropped here */
__device__ __forceinline__ bool zdrop_test(const int dm, const int ia, const int ja, const int Z, const int pen, int &best, int &bi, int &bj) {
    if (dm > best) {
        best = dm;
        bi = ia;
        bj = ja;
        return false;
    }
    return ia >= bi && ja >= bj && best - dm > Z + pen * abs((ia - bi) - (ja - bj));
}

/* the pair's results from lane 0: the record into ext, and the chosen score and end cell where BAXT's go (E: the end bonus) */
__device__ __forceinline__ void write_results(const dpx_fill_args &f, const int E, int32_t *ext, const int p, const int m, const int maxScore, const int maxRow,
                                              const int maxCol, const int qeScore, const int qeCol, const int lastDiag, const bool dropped) {
    const bool reached = E >= 0 && !dropped && qeCol >= 0 && qeScore + E > maxScore;
    f.score[p] = reached ? qeScore : maxScore;
    f.endRow[p] = reached ? m : maxRow;
    f.endCol[p] = reached ? qeCol : maxCol;
#ifndef DPX_BANDDIR_SCORE_ONLY
    u32x4 *rec = reinterpret_cast<u32x4 *>(ext + (size_t)p * 8u);
    const u32x4 w0 = {(unsigned)maxScore, (unsigned)maxRow, (unsigned)maxCol, (unsigned)qeScore};
    const u32x4 w1 = {(unsigned)qeCol, (unsigned)lastDiag, (dropped ? 1u : 0u) | (reached ? 2u : 0u), 0u};
    rec[0] = w0;
    rec[1] = w1;
#else
    /* the DPX_LONG_SCORES units (dpx_banddir_fill.inc) write the same record field by field: once per pair, and it keeps their code free
     * of 16-byte global stores, which tests/test_bscore_kernels_isa.py reads as "no code group is stored".  volatile keeps the eight
     * stores apart (plain and nontemporal ones are merged again); the global address space keeps them global_store, not flat_store */
    using gptr = volatile __attribute__((address_space(1))) int32_t *;
    const gptr rec = (gptr)(ext + (size_t)p * 8u);
    const int32_t v[8] = {maxScore, maxRow, maxCol, qeScore, qeCol, lastDiag, (int32_t)((dropped ? 1u : 0u) | (reached ? 2u : 0u)), 0};
#pragma unroll
    for (int k = 0; k < 8; k++) rec[k] = v[k];
#endif
}

/* an empty sequence (m <= 0 or n <= 0), on one lane: the in-band cells are one border line, cell k (1 <= k <= L = min(max(m, n), B-1))
 * on anti-diagonal k with H = bord(k) (o + k*e; two-piece gaps: the better piece), and 0 at k = 0.  The scan, the maximum and the row-m
 * rule run over it; no diagonal step, so a substitution table plays no part. */
template <bool ZDROP, class Bord>
__device__ __forceinline__ void scan_border_line(const dpx_fill_args &f, const int E, int32_t *ext, const int p, const int m, const int n, const int B, const Bord &bord,
                                                 const int Z, const int pen) {
    const int len = max(max(m, n), 0), L = min(len, B - 1);
    int best = 0, kb = 0, last = len, maxScore = 0, kmax = 0;
    bool dropped = false;
    for (int k = 1; k <= L; k++) {
        const int v = bord(k);
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
        if (bord(k) > maxScore) { maxScore = bord(k); kmax = k; }
    int qeScore = INT_MIN, qeCol = -1;
    if (m <= 0) { /* row m is row 0: the line itself (or the single cell (0, 0)) */
        qeScore = 0;
        qeCol = 0;
        for (int k = 1; k <= (n > 0 ? seen : 0); k++)
            if (bord(k) > qeScore) { qeScore = bord(k); qeCol = k; }
    } else if (m <= seen) { /* n == 0: row m holds the one cell (m, 0) */
        qeScore = bord(m);
        qeCol = 0;
    }
    write_results(f, E, ext, p, max(m, 0), maxScore, m > 0 ? kmax : 0, m > 0 ? 0 : kmax, qeScore, qeCol, last, dropped);
}

/* after step A_ (h_: its C values of H): the row-m pick-up into qe, then (ZDROP) the anti-diagonal's maximum and the drop test, which
 * sets lastDiag and stop.  The rules are explained at the top of dpx_zext_kernels.hip.  A macro over the kernel's own names (C, ZDROP, m,
 * n, B, Z, pen, lane, the step's i0, and the scan state qe, best, bi, bj, lastDiag, stop), not a function: as a function taking the state
 * by reference the same text compiled k_zext_fill<2, ., true, true> to 83 VGPRs instead of 64, from 8 waves per SIMD to 5. */
#define DPX_BAND_SCAN_AFTER(A_, h_)                                                                                       \
    {                                                                                                                     \
        const int a_ = (A_) + 2;                                                                                          \
        if (a_ >= m && a_ - m <= n && abs(2 * m - a_) <= B - 1) {                                                         \
            const int sm_ = m - i0, ln_ = sm_ / C, cc_ = sm_ % C; /* (0 <= sm_ <= B-1: the cell is in the band) */          \
            int v_ = 0;                                                                                                   \
            _Pragma("unroll") for (int c = 0; c < C; c++)                                                                 \
                if (cc_ == c) v_ = __builtin_amdgcn_readlane((h_)[c], ln_);                                               \
            qe = max(qe, (int)(((unsigned)v_ << 16) | (0xFFFFu - (unsigned)(a_ - 1))));                                   \
        }                                                                                                                 \
        if constexpr (ZDROP) {                                                                                            \
            const int rb_ = 0xFFFF - i0 - lane * C;                                                                       \
            int k_ = INT_MIN;                                                                                             \
            _Pragma("unroll") for (int c = 0; c < C; c++) k_ = max(k_, (int)pack_lo16(rb_ - c, max((h_)[c], -32768)));    \
            k_ = wave_max_i32(k_);                                                                                        \
            const int dm_ = k_ >> 16;                                                                                     \
            if (dm_ > -32768) { /* (else: no cell on this anti-diagonal) */                                               \
                const int ia_ = 0xFFFF - (k_ & 0xFFFF);                                                                   \
                if (zdrop_test(dm_, ia_, a_ - ia_, Z, pen, best, bi, bj)) {                                               \
                    lastDiag = a_;                                                                                        \
                    stop = true;                                                                                          \
                }                                                                                                         \
            }                                                                                                             \
        }                                                                                                                 \
    }

/* after the loops: the maximum of H over the computed cells and its first cell in row-major order, as k_baxt_fill finds it: every
 * slot's first maximum (within a slot cells arrive in row-major order); across slots max score, min row, min col.  The border cells of
 * anti-diagonal 1 need no candidate: they count only when o + e > 0, and then the pair cannot drop at anti-diagonal 1, so (1, 1)
 * is computed and holds H >= 2 * (o + e) > o + e.  Then the record, from lane 0. */
template <int C>
__device__ __forceinline__ void scan_finish(const dpx_fill_args &f, const int E, int32_t *ext, const int p, const int *key, const int lane, const int m, const int B, const int qe,
                                            const int lastDiag, const bool stop) {
    unsigned long long mine = 0ull;
#pragma unroll
    for (int c = 0; c < C; c++) {
        const int hv = key[c] >> 16;
        if (hv > 0) {
            const int A = 0xFFFF - (key[c] & 0xFFFF);
            const int aa = A + 2;
            const int pp = (aa + B - 1) & 1;
            const int u = 2 * (lane * C + c) + pp;
            const int i = (aa + u - (B - 1)) >> 1;
            const int j = aa - i;
            const unsigned long long k = end_key(hv, i, j);
            mine = k > mine ? k : mine;
        }
    }
    const unsigned long long top = wave_max_u64(mine);
    const int qeTop = qe;
    if (lane == 0) {
        const int hv = (int)(top >> 40);
        const int maxRow = hv > 0 ? (int)(0xFFFFFu - (unsigned)((top >> 20) & 0xFFFFFu)) : 0;
        const int maxCol = hv > 0 ? (int)(0xFFFFFu - (unsigned)(top & 0xFFFFFu)) : 0;
        const bool none = qeTop == INT_MIN;
        const int qeScore = none ? INT_MIN : (qeTop >> 16);
        const int qeCol = none ? -1 : (0xFFFF - (qeTop & 0xFFFF)) + 1 - m;
        write_results(f, E, ext, p, m, hv, maxRow, maxCol, qeScore, qeCol, lastDiag, stop);
    }
}

/* ---------------------------------------------------------- the walks -------------------------------------------------------- */

/* ---- traceback: one lane per pair, ANW's three-state walk (dpx_traceback_kernels.hip: tb_walk_lane) over the band layout, with ANW's two tails.
 * The walk stands on stored cells only; the neighbours it reads are in band (the diagonal one always; the left / upper one because the
 * gap it came through is finite) or border cells, which open the gap.  mm = H_diag + the scorer's term; the relation character is the
 * byte compare whatever the scorer. ---- */
template <class Scorer>
__device__ __forceinline__ void band_walk_lane(const dpx_fill_args &a, const Scorer &sc, int numPairs, const int32_t *endRow, const int32_t *endCol,
                                               const uint64_t *tbOff, char *tb, int32_t *tbLen) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= numPairs) return;
    const dpx_pair_dev pr = a.pairs[p];
    const int n = pr.n, m = pr.m, band = a.band;
    const unsigned char *ref = reinterpret_cast<const unsigned char *>(a.seq + pr.refIdx);
    const unsigned char *qry = reinterpret_cast<const unsigned char *>(a.seq + pr.qryIdx);
    const int cap = (m + n + 1 + 3) & ~3; /* line capacity, dword-aligned like tbOff[] */
    char *lr = tb + tbOff[p], *lx = lr + cap, *lq = lx + cap;
    int pos = cap; /* lines grow from the back */
    uint32_t accR = 0, accX = 0, accQ = 0; /* the last <= 4 characters of each line, earliest in the highest byte */
    const int o = a.gapOpen, e = a.gapExtend;
    const BandView v{a.mat, pr.matOff, pr.chunkStride, band, o, e};
    auto emit = [&](const int rc, const int xc, const int qc) {
        --pos;
        accR = (accR << 8) | (uint32_t)(unsigned char)rc;
        accX = (accX << 8) | (uint32_t)(unsigned char)xc;
        accQ = (accQ << 8) | (uint32_t)(unsigned char)qc;
        if ((pos & 3) == 0) {
            *reinterpret_cast<uint32_t *>(lr + pos) = accR;
            *reinterpret_cast<uint32_t *>(lx + pos) = accX;
            *reinterpret_cast<uint32_t *>(lq + pos) = accQ;
        }
    };
    int i = endRow[p], j = endCol[p];
    CharWin qw{qry}, rw{ref};
    int cur = 0; /* 0 SCORING, 1 INSERTION, 2 DELETION */
    while (i != 0 && j != 0) {
        if (cur == 0) {
            const int qc = qw.get(i - 1), rc = rw.get(j - 1);
            const bool eq = qc == rc;
            const int dg = v.get(i - 1, j - 1, 0);
            const int rv = sc.r(rc), qv = sc.q(qc);
            const int mm = dg + sc.at(qv, rv);
            const int D = v.get(i, j, 2), I = v.get(i, j, 1);
            const int vmax = max(D, mm);
            if (I >= vmax) cur = 1;
            else if (D >= mm) cur = 2;
            else { emit(rw.get(j - 1), eq ? '*' : '|', qw.get(i - 1)); i--; j--; }
        } else if (cur == 1) {
            const bool open = (j == 1) || (v.get(i, j - 1, 0) + o + e >= v.get(i, j - 1, 1) + e); /* (a border neighbour opens the gap) */
            if (open) cur = 0;
            emit(rw.get(j - 1), ' ', '_'); j--;
        } else {
            const bool open = (i == 1) || (v.get(i - 1, j, 0) + o + e >= v.get(i - 1, j, 2) + e);
            if (open) cur = 0;
            emit('_', ' ', qw.get(i - 1)); i--;
        }
    }
    while (i > 0) { emit('_', ' ', qw.get(i - 1)); i--; }  /* column-0 border: QUERY_DELETION */
    while (j > 0) { emit(rw.get(j - 1), ' ', '_'); j--; }  /* row-0 border: QUERY_INSERTION */
    if (pos & 3) { /* the 1-3 newest characters have not filled a dword: the newest sits in the lowest byte, at `pos` */
        const int left = 4 - (pos & 3);
        for (int t = 0; t < left; t++) {
            lr[pos + t] = (char)(accR >> (8 * t)); lx[pos + t] = (char)(accX >> (8 * t)); lq[pos + t] = (char)(accQ >> (8 * t));
        }
    }
    tbLen[p] = cap - pos;
}

/* -----------------------------------------------------------------------------------------------------
 * Wave-cooperative traceback: k_traceback_wave's scheme (dpx_traceback_kernels.hip) for the three band-layout planes.  One WAVE owns a pair; lane c
 * fetches column cLo + c of a window of 48 rows x 64 columns of H, I and D around the walker into LDS (one 112-byte line per column and
 * plane; in-band border cells carry their H, every other cell without storage and every edge I / D is -32768, the window's minus
 * infinity, which cell() turns into DPX_NEG) -- only the three 8-row groups around the walker's diagonal unless the
 * walk left the last window sideways -- and the walk takes RUNS: every lane decides one cell of the line the path would follow next (the
 * walker's diagonal in SCORING, its row in INSERTION, its column in DELETION) and a ballot gives the number of steps the path really
 * follows.  The band layout has no 16-byte column pieces (the rows of a column lie on consecutive anti-diagonals): 2-byte loads through
 * dpx_band_plane_index, as the linear-gap banded walk does.  Unlike k_basw_traceback_wave's window, a cell without storage must not read 0:
 * scores are negative here, and a 0 in I or D would win "I >= max(D, mm)".  After the runs come ANW's two tails (the rest of column 0 as
 * deletions, the rest of row 0 as insertions), written by all lanes at once.
 *
 * A table scorer (tableSrc: the 1-KiB table in global memory, sc.code: the map in global memory) keeps the table in LDS behind the
 * window, translates a lane's two characters when it loads a window -- cdR, and the query code in bits 8.. of chQ -- and reads
 * mm = H_diag + table[cdR + query code].
 * ----------------------------------------------------------------------------------------------------- */
struct BandWin {
    static constexpr int G = 6;             /* row groups of a window */
    static constexpr int GL = 3;            /* row groups of a banded (diagonal-following) window column */
    static constexpr int WR = 8 * G;        /* rows R0+1 .. R0+WR; columns cLo .. cLo+63, one per lane */
    static constexpr int CS = WR + 8;       /* int16 elements between two columns in LDS */
    static constexpr int kBytes = 3 * 64 * CS * 2;
};

template <class Scorer>
__device__ __forceinline__ void band_walk_wave(const dpx_fill_args &a, Scorer sc, const void *tableSrc, unsigned char *smemTb,
                                               int numPairs, const int32_t *endRow, const int32_t *endCol, const uint64_t *tbOff, char *tb,
                                               int32_t *tbLen) {
    constexpr int G = BandWin::G, GL = BandWin::GL, WR = BandWin::WR, CS = BandWin::CS;
    int16_t *win = reinterpret_cast<int16_t *>(smemTb); /* win[(plane * 64 + (jj - cLo)) * CS + (ii - R0 - 1)] = plane[ii][jj] */
    const int p = blockIdx.x;
    const int lane = threadIdx.x;
    if (p >= numPairs) return;
    if constexpr (Scorer::kTable) /* 64 x 16 B = the 1-KiB table, behind the window; load_window's fences order it before the first read.
                                   * Not table_stage_rows: that copies the map too, and the walk's LDS holds kBytes + the table alone */
        reinterpret_cast<u32x4 *>(smemTb + BandWin::kBytes)[lane] = reinterpret_cast<const u32x4 *>(tableSrc)[lane];
    const dpx_pair_dev pr = a.pairs[p];
    const int n = pr.n, m = pr.m, B = a.band;
    const unsigned char *ref = reinterpret_cast<const unsigned char *>(a.seq + pr.refIdx);
    const unsigned char *qry = reinterpret_cast<const unsigned char *>(a.seq + pr.qryIdx);
    const int16_t *base = a.mat + pr.matOff;
    const uint32_t cs = pr.chunkStride;
    const int cap = (m + n + 1 + 3) & ~3;
    char *lr = tb + tbOff[p], *lx = lr + cap, *lq = lx + cap;
    int pos = cap;
    const int g = a.gapOpen, ext = a.gapExtend;
    constexpr uint32_t kNegInf16 = 0x8000u; /* -32768: below every finite value the range check admits */
    int i = __builtin_amdgcn_readfirstlane(endRow[p]), j = __builtin_amdgcn_readfirstlane(endCol[p]);
    int R0 = 1 << 28, cLo = 1 << 28;
    int diag0 = 0;         /* i - j of the cell the window was anchored on */
    bool banded = false;   /* ... and whether only the groups around that diagonal were fetched */
    bool wantFull = false; /* the walk left the last window sideways (a long gap): fetch whole columns next time */
    uint32_t chR = 0u, chQ = 0u; /* reference character of this lane's column; query character of window row `lane` (kTable: its code in bits 8..) */
    uint32_t cdR = 0u;           /* kTable: sc.r(chR) */
    auto stored = [&](const int ii, const int jj) -> bool { return ii <= m && jj <= n && cell_in_band(ii, jj, B); };
    /* the loads of NPL planes (from plane PL0) of a window, nothing else: every load is in flight before the wave waits for the first */
    auto issue = [&](auto pl0C, auto nplC, auto cntC, auto &raw, const int gBase, const int gFirst, const int jc) {
        constexpr int PL0 = decltype(pl0C)::value, NPL = decltype(nplC)::value, CNT = decltype(cntC)::value;
#pragma unroll
        for (int gi = 0; gi < CNT; gi++) {
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const int ii2 = (gBase + gFirst + gi) * 8 + 1 + e;
                const bool ok = stored(ii2, jc);
                const int16_t *at = ok ? base + dpx_band_plane_index(ii2, jc, B, PL0, cs) : a.mat; /* (no storage: the pool's first bytes, masked below) */
#pragma unroll
                for (int pl = 0; pl < NPL; pl++)
                    raw[(pl * CNT + gi) * 8 + e] = (uint32_t)*reinterpret_cast<const uint16_t *>(at + (ok ? pl * DPX_BAND_PLANE_ELEMS : 0));
            }
        }
    };
    /* what issue() loaded becomes the window in LDS: stored cells (edge I / D as minus infinity), the H of in-band border cells, minus
     * infinity everywhere else */
    auto commit = [&](auto pl0C, auto nplC, auto cntC, const auto &raw, const int gBase, const int gFirst, const int jc) {
        constexpr int PL0 = decltype(pl0C)::value, NPL = decltype(nplC)::value, CNT = decltype(cntC)::value;
#pragma unroll
        for (int pl = 0; pl < NPL; pl++) {
#pragma unroll
            for (int gi = 0; gi < CNT; gi++) {
                uint32_t d[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    const int ii2 = (gBase + gFirst + gi) * 8 + 1 + e;
                    uint32_t val = kNegInf16;
                    if (stored(ii2, jc)) val = edge(ii2, jc, B, PL0 + pl) ? kNegInf16 : raw[(pl * CNT + gi) * 8 + e];
                    else if (PL0 + pl == 0 && (ii2 == 0 || jc == 0) && ii2 >= 0 && jc >= 0 && ii2 <= m && jc <= n && in_band(ii2, jc, B))
                        val = (uint32_t)border(ii2, jc, g, ext) & 0xFFFFu;
                    d[e >> 1] |= val << ((e & 1) * 16);
                }
                *reinterpret_cast<u32x4 *>(win + ((PL0 + pl) * 64 + lane) * CS + (gFirst + gi) * 8) = u32x4{d[0], d[1], d[2], d[3]};
            }
        }
    };
    /* first fetched row group (relative to the window's first) of this lane's column in a banded window whose last column holds the
     * diagonal's row iiDiag */
    auto band_first = [&](const int iiDiag, const int r0) -> int {
        const int dl = (iiDiag - r0 - 1) - 63 + lane;
        return min(max((dl - 8) >> 3, 0), G - GL);
    };
    auto load_window = [&](const int ii, const int jj) {
        const int gBase = ((ii - 1) >> 3) - (G - 1);
        R0 = gBase * 8;
        cLo = jj - 63;
        const int jc = cLo + lane;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local"); /* the previous window's reads are done before it is overwritten */
        __builtin_amdgcn_wave_barrier();
        diag0 = ii - jj;
        banded = !wantFull;
        const int gFirst = banded ? band_first(ii, R0) : 0;
        /* the lane's two characters: the query character of row R0 + 1 + lane, the reference character of its column */
        const int qi = R0 + lane;
        const bool okQ = lane < WR && qi >= 0 && qi < m, okR = jc >= 1 && jc <= n;
        const uint32_t rq = *(okQ ? qry + qi : reinterpret_cast<const unsigned char *>(a.seq));
        const uint32_t rr = *(okR ? ref + (jc - 1) : reinterpret_cast<const unsigned char *>(a.seq));
        using I0 = int_c<0>;
        using I1 = int_c<1>;
        using I2 = int_c<2>;
        using I3 = int_c<3>;
        if (banded) { /* the usual window: three row groups of all three planes at once (72 two-byte loads in flight) */
            uint32_t raw[3 * GL * 8];
            issue(I0{}, I3{}, int_c<GL>{}, raw, gBase, gFirst, jc);
            commit(I0{}, I3{}, int_c<GL>{}, raw, gBase, gFirst, jc);
        } else { /* whole columns (after a long gap; rare): plane by plane, 48 loads in flight, to keep the kernel's registers down */
            uint32_t raw[G * 8];
            issue(I0{}, I1{}, int_c<G>{}, raw, gBase, gFirst, jc);
            commit(I0{}, I1{}, int_c<G>{}, raw, gBase, gFirst, jc);
            issue(I1{}, I1{}, int_c<G>{}, raw, gBase, gFirst, jc);
            commit(I1{}, I1{}, int_c<G>{}, raw, gBase, gFirst, jc);
            issue(I2{}, I1{}, int_c<G>{}, raw, gBase, gFirst, jc);
            commit(I2{}, I1{}, int_c<G>{}, raw, gBase, gFirst, jc);
        }
        /* the two characters are waited for here, not in every trip of the walk; a table scorer translates them here, once per window */
        if constexpr (Scorer::kTable) {
            chR = okR ? rr : 0u;
            cdR = (uint32_t)sc.r((int)chR);
            chQ = okQ ? rq : 0u;
            chQ |= (uint32_t)sc.q((int)chQ) << 8;
            asm volatile("" : "+v"(chQ), "+v"(chR), "+v"(cdR));
        } else {
            chQ = okQ ? rq : 0u;
            chR = okR ? rr : 0u;
            asm volatile("" : "+v"(chQ), "+v"(chR));
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
    };
    /* rows i-1, i and columns j-1, j must lie inside the window */
    auto need_window = [&]() -> bool {
        if (i - 1 <= R0 || i > R0 + WR || j - 1 < cLo || j > cLo + 63) return true;
        if (banded) { const int dev = (i - j) - diag0; if (dev < -7 || dev > 6) { wantFull = true; return true; } } /* outside the fetched groups */
        return false;
    };
    auto cell = [&](const int pl, const int col, const int row) -> int {
        const int v = (int)win[(pl * 64 + col) * CS + row];
        return v == -32768 ? DPX_NEG : v;
    };
    /* number of lanes that continue a run which starts at lane `from` and goes DOWN the lanes while `on` holds (lane 0 is never on) */
    auto run_down = [&](const bool on, const int from) -> int {
        const unsigned long long inv = ~__builtin_amdgcn_ballot_w64(on) << (63 - from);
        return inv ? __builtin_clzll(inv) : 64;
    };
    /* the query byte of window row `row`, as every lane holds it in chQ */
    auto query_of = [&](const int row, int &packed) -> int {
        packed = __builtin_amdgcn_ds_bpermute(row << 2, (int)chQ);
        return Scorer::kTable ? (packed & 0xFF) : packed;
    };
    /* SCORING decision of window cell (rq, cq) (>= 1 each): 0 diagonal, 1 to INSERTION, 2 to DELETION, 3 not a cell (row / column <= 0) */
    auto decide_cell = [&](const int rq, const int cq, int &qcOut) -> uint32_t {
        int qpk;
        qcOut = query_of(rq, qpk);
        const int ii = R0 + 1 + rq, jc = cLo + cq;
        const int dg = cell(0, cq - 1, rq - 1), I = cell(1, cq, rq), D = cell(2, cq, rq);
        int mm;
        if constexpr (Scorer::kTable) mm = dg + sc.at(qpk >> 8, (int)cdR);
        else mm = dg + sc.at(qpk, (int)chR);
        uint32_t d = I >= max(D, mm) ? 1u : (D >= mm ? 2u : 0u);
        if (ii <= 0 || jc <= 0) d = 3u;
        return d;
    };
    /* (r, c) = the walker's window cell; lane l decides the cell of the walker's diagonal in its own column */
    auto decide_diag = [&](const int r, const int c, int &qcOut) -> uint32_t {
        const int rr = r - (c - lane);
        const bool usable = lane <= c && lane >= 1 && rr >= 1;
        const uint32_t d = decide_cell(usable ? rr : 1, usable ? lane : 1, qcOut);
        return usable ? d : 3u;
    };
    auto emit_diag = [&](const int c, const int len, const int qc) {
        const int k = c - lane;
        if (k >= 0 && k < len) {
            const int at = pos - 1 - k;
            lr[at] = (char)chR; lx[at] = ((uint32_t)qc == chR) ? '*' : '|'; lq[at] = (char)qc;
        }
        pos -= len;
    };
    auto emit_left = [&](const int c, const int len) {
        const int k = c - lane;
        if (k >= 0 && k < len) { const int at = pos - 1 - k; lr[at] = (char)chR; lx[at] = ' '; lq[at] = '_'; }
        pos -= len;
    };
    auto emit_up = [&](const int r, const int len) {
        int qpk;
        const int qc = query_of(max(r - lane, 0), qpk);
        if (lane < len) { const int at = pos - 1 - lane; lr[at] = '_'; lx[at] = ' '; lq[at] = (char)qc; }
        pos -= len;
    };
    int cur = 0; /* 0 SCORING, 1 INSERTION, 2 DELETION */
    while (i > 0 && j > 0) {
        if (need_window()) { load_window(i, j); wantFull = false; }
        const int r = i - R0 - 1, c = j - cLo;
        if (cur == 0) {
            int qc;
            const uint32_t d = decide_diag(r, c, qc);
            const int run = run_down(d == 0u, c);
            if (run) {
                emit_diag(c, run, qc); i -= run; j -= run;
                const int cx = c - run, rx = r - run; /* the cell that ends the run has been decided with it */
                if (cx >= 1 && rx >= 1 && i > 0 && j > 0) {
                    const int dx = __builtin_amdgcn_readlane((int)d, cx);
                    if (dx == 1 || dx == 2) cur = dx;
                }
                continue;
            }
            cur = __builtin_amdgcn_readlane((int)d, c); /* 1: to INSERTION, 2: to DELETION */
            if (cur == 3) break;                         /* (cannot happen: the walker stands on a cell) */
        } else if (cur == 1) {
            /* INSERTION: steps to the left along row i until (and including) the cell where the gap was opened; lane l decides the cell in
             * column l.  The left neighbour in column 0: opened; on the band's lower edge: its I is minus infinity, opened. */
            const int cq = max(lane, 1), jc = cLo + cq;
            const bool opened = !cell_in_band(i, jc - 1, B) || cell(0, cq - 1, r) + g + ext >= cell(1, cq - 1, r) + ext;
            const bool usable = lane <= c && lane >= 1 && jc >= 1 && (!banded || (i - j) - diag0 + (c - lane) <= 6);
            const int cont = run_down(usable && !opened, c); /* cells the gap passes through */
            const bool stops = c - cont >= 1 && cLo + c - cont >= 1 && (!banded || (i - j) - diag0 + cont <= 6); /* ... then a usable cell that opened it (else: the window's edge) */
            const int len = cont + (stops ? 1 : 0);
            emit_left(c, len); j -= len;
            if (stops) cur = 0;
        } else {
            /* DELETION: steps up along column j; lane k decides the cell k rows above the walker.  The upper neighbour in row 0: opened; on the
             * band's upper edge: its D is minus infinity, opened. */
            const int rq = max(r - lane, 1), ii = R0 + 1 + rq;
            const bool opened = !cell_in_band(ii - 1, j, B) || cell(0, c, rq - 1) + g + ext >= cell(2, c, rq - 1) + ext;
            const bool usable = r - lane >= 1 && ii >= 1 && (!banded || (i - j) - diag0 - lane >= -7);
            const unsigned long long m64 = __builtin_amdgcn_ballot_w64(!(usable && !opened)); /* first lane that ends the run */
            const int cont = m64 ? __builtin_ctzll(m64) : 64;
            const bool stops = r - cont >= 1 && R0 + 1 + r - cont >= 1 && (!banded || (i - j) - diag0 - cont >= -7);
            const int len = cont + (stops ? 1 : 0);
            emit_up(r, len); i -= len;
            if (stops) cur = 0;
        }
    }
    /* ANW's tails: the rest of column 0 as deletions, then the rest of row 0 as insertions (at most one of the two is left) */
    for (int k = lane; k < i; k += 64) { const int at = pos - 1 - k; lr[at] = '_'; lx[at] = ' '; lq[at] = (char)qry[i - 1 - k]; }
    pos -= max(i, 0);
    for (int k = lane; k < j; k += 64) { const int at = pos - 1 - k; lr[at] = (char)ref[j - 1 - k]; lx[at] = ' '; lq[at] = '_'; }
    pos -= max(j, 0);
    if (lane == 0) tbLen[p] = cap - pos;
}

} // namespace dpx_band
#endif
