/*
 * dpx_affine_dev.hpp -- device helpers of the Gotoh fills on the stripe schedule, shared by dpx_affine_kernels.hip (the plain ANW / ASW /
 * ASG kernels) and dpx_scoretab_kernels.hip (the score-only kernels under a substitution table): the cell updates of the one-wave-per-
 * pair body (dpx_affine_fill.inc) and of the lane-packed body (dpx_affine_lanes.inc), and the two result publishers.  TABLE = false is
 * the byte compare; TABLE = true reads the diagonal term from the wave's LDS table image, which table_stage() keeps TRANSPOSED (the
 * entry of reference code c and query code q at (q << 5) + c): `rc` is then the reference code and `qc` the LDS address of the query
 * code's column (table_column()), a cell's byte sits at qc + rc (table_byte()), and `match` / `mismatch` are not read.
 * __forceinline__ everywhere: the code lands in the kernels as it did when these lived in dpx_affine_kernels.hip's anonymous namespace.
 */
#ifndef DPX_AFFINE_DEV_HPP
#define DPX_AFFINE_DEV_HPP

#include "dpx_fill_common.hpp"
#include "dpx_kernels.h"
#include "dpx_prims.hpp"
#include "dpx_table_dev.hpp"

namespace dpx_affine {

using dpx::wave_shr1;
using dpx_dev::wave_max_u64;
using dpx_fill::ramp_stores;
using dpx_fill::store_tile;
using dpx_table::table_stage;
using dpx_table::table_translate;

/* =====================================================================================================
 * Affine-gap (Gotoh) global fill: AffineNeedlemanWunsch (c++/AffineNeedlemanWunsch.cpp:167-240).
 *   D[i][j] = (i==1) ? H[i-1][j]+o+e : max(H[i-1][j]+o+e, D[i-1][j]+e)      vertical gap   (:185-197)
 *   I[i][j] = (j==1) ? H[i][j-1]+o+e : max(H[i][j-1]+o+e, I[i][j-1]+e)      horizontal gap (:201-213)
 *   H[i][j] = max(I, max(D, H[i-1][j-1]+s))                                                (:229-236)
 * The i==1 / j==1 special cases are expressed by virtual borders D[0][j] = I[i][0] = DPX_NEG, which gives the
 * identical values for every stored cell.  Three int16 planes (H, I, D) are written per step.
 * Affine-gap Smith-Waterman (ASW, LOCAL = true) shares the body: H = max(0, ...) with zero borders, and the start cell is tracked
 * as in k_linear_fill (per-row (H << 16 | 0xFFFF - j) keys folded per stripe, one wave reduction at the end).
 * ===================================================================================================== */
/* ---- the substitution table in LDS (TABLE kernels) ----
 * table_stage() and table_translate() are dpx_table_dev.hpp's.  Pointers into LDS are kept in the LDS address space, where they are
 * 32-bit offsets. */
typedef __attribute__((address_space(3))) signed char lds_i8;

/* the LDS address of query byte q's column of the transposed table (rows past the query's end arrive as 0x100: some code, never read back) */
__device__ __forceinline__ int table_column(unsigned char *img, const unsigned char *codeL, const int q) {
    return (int)reinterpret_cast<uintptr_t>((lds_i8 *)img) + ((int)codeL[q & 0xFF] << 5);
}
__device__ __forceinline__ int table_byte(const int column, const int rc) { return *reinterpret_cast<const lds_i8 *>((uintptr_t)(uint32_t)(column + rc)); }

template <int R>
struct AffState {
    int Hl[R], Il[R]; /* H[row][j-1], I[row][j-1] */
    int Dl[R];        /* D[row][j] just computed (needed only for the store and the lane hand-off) */
    int qc[R];
    unsigned key[R];  /* ASW: per-row running max of (H << 16 | 0xFFFF - j); ASG: key[0] alone, of ((H + 0x8000) << 16 | 0xFFFF - j) in register rsel */
    int dtop;
};

template <int R, int MODE, bool TABLE = false> /* 0 ANW, 1 ASW, 2 ASG */
__device__ __forceinline__ void aff_cells(AffState<R> &st, const int upH, const int upD, const int rc, const int match,
                                          const int mismatch, const int oe, const int e, const unsigned negj, [[maybe_unused]] const int rsel = 0) {
    int uH = upH, uD = upD, d = st.dtop;
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int lH = st.Hl[r];
        int s;
        if constexpr (TABLE) s = table_byte(st.qc[r], rc); /* one signed byte from LDS */
        else s = (st.qc[r] == rc) ? match : mismatch;
        const int Dn = max(uH + oe, uD + e);
        const int In = max(lH + oe, st.Il[r] + e);
        int h = max(max(Dn, d + s), In); /* v_max3_i32 */
        if constexpr (MODE == 1) {
            h = max(h, 0);
            st.key[r] = max(st.key[r], ((unsigned)h << 16) | negj);
        }
        d = lH;
        uH = h;
        uD = Dn;
        st.Hl[r] = h;
        st.Il[r] = In;
        st.Dl[r] = Dn;
    }
    st.dtop = upH;
    if constexpr (MODE == 2) { /* ASG: no floor; the running (max, first column) of ONE row, register rsel = (m-1) % R of every lane (the lane
                                * that owns row m reads it).  H may be negative: biased into 0 .. 65535.  A select chain on the wave-uniform
                                * rsel, not an indexed read: the registers stay registers. */
        int hm = st.Hl[0];
#pragma unroll
        for (int r = 1; r < R; r++) hm = (r == rsel) ? st.Hl[r] : hm;
        st.key[0] = max(st.key[0], ((unsigned)(hm + 0x8000) << 16) | negj);
    }
}

template <int R, int MODE, bool STORE, bool MASKED, bool WHOLE, bool TABLE = false>
__device__ __forceinline__ void aff_step(AffState<R> &st, const int t, const int lane, const int n, const bool laneHasRows,
                                         const int match, const int mismatch, const int oe, const int e, const int e0H,
                                         const int e0D, const int rc, int16_t *edgeH, int16_t *edgeD,
                                         const bool writeEdge, int16_t *tileDst, const int storeLanes, const int rampLines,
                                         [[maybe_unused]] const int rsel = 0) {
    const int j = t - lane + 1;
    const int upH = wave_shr1(st.Hl[R - 1], e0H);
    const int upD = wave_shr1(st.Dl[R - 1], e0D);
    bool active = true;
    if constexpr (MASKED) active = laneHasRows && (j >= 1) && (j <= n);
    if (active) {
        if constexpr (TABLE) aff_cells<R, MODE, true>(st, upH, upD, rc, match, mismatch, oe, e, 0xFFFFu - (unsigned)j, rsel);
        else aff_cells<R, MODE>(st, upH, upD, rc, match, mismatch, oe, e, 0xFFFFu - (unsigned)j, rsel);
        if (writeEdge && lane == 63) {
            edgeH[j] = (int16_t)st.Hl[R - 1];
            edgeD[j] = (int16_t)st.Dl[R - 1];
        }
        if constexpr (STORE && MASKED && !WHOLE) {
            store_tile<R>(tileDst, st.Hl);
            store_tile<R>(tileDst + 64 * R, st.Il);
            store_tile<R>(tileDst + 128 * R, st.Dl);
        }
    }
    if constexpr (STORE && (!MASKED || WHOLE)) { /* whole lines, also on the skew ramps (see lin_step) */
        bool doStore = lane < storeLanes;
        if constexpr (MASKED) doStore = doStore && ramp_stores<R>(lane, t, n, rampLines);
        if (doStore) {
            store_tile<R>(tileDst, st.Hl);
            store_tile<R>(tileDst + 64 * R, st.Il);
            store_tile<R>(tileDst + 128 * R, st.Dl);
        }
    }
}

/* first strict maximum in row-major order over the lanes' bests (k_linear_fill, c++/LinearSmithWaterman.cpp:145-157) */
__device__ __forceinline__ void sw_publish(const dpx_fill_args &a, const int p, const int lane, const int bestv, const int bestrow, const int bestcol) {
    const unsigned long long mine = ((unsigned long long)(unsigned)bestv << 32) | (unsigned)(0x7FFFFFFF - bestrow);
    const unsigned long long top = wave_max_u64(mine);
    if ((int)(top >> 32) == 0) {
        if (lane == 0) { a.score[p] = 0; a.endRow[p] = 0; a.endCol[p] = 0; }
    } else if (mine == top) { /* rows are unique per lane: exactly one lane matches, and it holds the row's first column */
        a.score[p] = bestv;
        a.endRow[p] = bestrow;
        a.endCol[p] = bestcol;
    }
}

/* ASG: score and end cell of row m from that row's biased key (the lane that owns row m calls this with its own key): the first
 * maximum over columns 0 .. n, column 0 being the border H[m][0] = o + m*e, which wins a tie as the smallest column */
__device__ __forceinline__ void asg_publish(const dpx_fill_args &a, const int p, const int m, const unsigned key, const int colZero) {
    const int hv = (int)(key >> 16) - 0x8000, col = 0xFFFF - (int)(key & 0xFFFFu);
    const bool zero = colZero >= hv;
    a.score[p] = zero ? colZero : hv;
    a.endRow[p] = m;
    a.endCol[p] = zero ? 0 : col;
}

/* Affine lane-packed kernel: the Gotoh recurrence of k_affine_fill on the several-pairs-per-wave schedule of
 * k_linear_lanes (`up` of H and D through wave_shr:1, a slot's first lane takes the row-0 borders); the three planes H,
 * I, D leave through the same LDS line stage into the 8 x 8 tile layout, three whole-line stores per step.  One wave per
 * workgroup: the stage needs 27 KiB of LDS per wave (three planes), so small workgroups keep five of them on a CU. */
/* Round 3: the cell update keeps its state as H + (o+e), I + e, D + e (aff_cells_g: 9 vector instructions per cell instead of 10, rows
 * in place), eight steps per trip, routing in registers, loop control on the scalar unit -- as in k_linear_lanes.  Tried and dropped:
 * a HALF-LINE stage (4 columns per lane and plane, 15 KiB of LDS per wave instead of 27: ten waves per CU instead of five; the two
 * 64-byte halves of a line stored four steps apart by the same wave) -- bit-exact, 2.42 ms instead of 1.67 on 100k short reads: a
 * 128-byte line that is written in two pieces costs far more than the residency buys. */

template <int R>
struct AffStateG {
    int Hoe[R], Ie[R]; /* H[row][j-1] + (o+e), I[row][j-1] + e */
    int qc[R];
    int dtopOe;        /* H[row0][j-1] + (o+e) */
    int DeLast;        /* D[row0+R][j] + e of the column just computed (the next lane's "D above") */
    unsigned key[R];   /* ASW: per-row running max of (H << 16 | 0xFFFF - j); ASG: key[0] alone, of ((H + 0x8000) << 16 | 0xFFFF - j) in register rsel */
};

/* D = max(H_up + oe, D_up + e);  I = max(H_left + oe, I_left + e);  H = max3(D, H_diag + s, I)   (c++/AffineNeedlemanWunsch.cpp:185-236)
 * TABLE: the state stays biased; the diagonal term is (H_diag + oe) + s + (-oe), the table byte and the constant in ONE three-operand add
 * (v_add3_u32) per cell -- `matchG` carries -(o+e) then and `mismatchG` is not read. */
template <int R, int MODE, bool TABLE = false> /* 0 ANW, 1 ASW, 2 ASG */
__device__ __forceinline__ void aff_cells_g(AffStateG<R> &st, const int upHoe, const int upDe, const int rc, const int matchG, const int mismatchG,
                                            const int oe, const int e, int (&Hv)[R], int (&Iv)[R], int (&Dv)[R], const unsigned negj,
                                            [[maybe_unused]] const int rsel = 0) {
    int dterm[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        if constexpr (TABLE) dterm[r] = ((r == 0) ? st.dtopOe : st.Hoe[r - 1]) + table_byte(st.qc[r], rc) + matchG; /* s + (-oe) */
        else dterm[r] = ((r == 0) ? st.dtopOe : st.Hoe[r - 1]) + ((st.qc[r] == rc) ? matchG : mismatchG); /* (s - oe) */
    }
    int ug = upHoe, ud = upDe;
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int Dn = max(ug, ud);
        const int In = max(st.Hoe[r], st.Ie[r]);
        int h = max(max(Dn, dterm[r]), In); /* v_max3_i32 */
        if constexpr (MODE == 1) { /* ASW: the zero floor, and the row's start-cell key */
            h = max(h, 0);
            st.key[r] = max(st.key[r], ((unsigned)h << 16) | negj);
        }
        Hv[r] = h; Iv[r] = In; Dv[r] = Dn;
        ug = h + oe;
        ud = Dn + e;
        st.Hoe[r] = ug;
        st.Ie[r] = In + e;
    }
    st.DeLast = ud;
    st.dtopOe = upHoe;
    if constexpr (MODE == 2) { /* ASG: the biased key of one row, register rsel = (m-1) % 8 of the slot's lanes (aff_cells) */
        int hm = Hv[0];
#pragma unroll
        for (int r = 1; r < R; r++) hm = (r == rsel) ? Hv[r] : hm;
        st.key[0] = max(st.key[0], ((unsigned)(hm + 0x8000) << 16) | negj);
    }
}

} // namespace dpx_affine

#endif
