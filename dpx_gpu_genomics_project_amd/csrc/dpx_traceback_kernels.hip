/*
 * dpx_traceback_kernels.hip -- what reads the int16 score matrices of the stripe and band layouts back: the export of one plane as a
 * row-major matrix (k_export_matrix) and the three walks from the end cell (one lane per pair: k_traceback / k_asw_traceback /
 * k_asg_traceback; one wave per pair over an LDS window: k_traceback_wave).  The banded affine units have walks of their own.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpx_device.hpp"
#include "dpx_kernels.h"
#include "dpx_layout.h"
#include "dpx_prims.hpp"

namespace {

using namespace dpx_dev;

/* =====================================================================================================
 * Export: un-tile one pair's plane into the reference's row-major (m+1) x (n+1) layout, borders included.
 * ===================================================================================================== */
__global__ void k_export_matrix(const int16_t *mat, dpx_pair_dev pr, int algo, int R, int planes, int plane, int gapOpen,
                                int gapExtend, int band, int16_t *out) {
    const int n = pr.n, m = pr.m;
    if (pr.rows) R = pr.rows;
    const size_t total = (size_t)(m + 1) * (size_t)(n + 1);
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int i = (int)(idx / (size_t)(n + 1));
        const int j = (int)(idx % (size_t)(n + 1));
        int v;
        if (i == 0 || j == 0) {
            const int len = i + j; /* one of them is 0 */
            if (plane != 0) v = 0;                                   /* I / D are zero-initialised (ANW.cpp:24-27) */
            else if (algo == DPX_K_LNW) v = len * gapOpen;           /* LNW.cpp:31-41 */
            else if (algo == DPX_K_ANW) v = len == 0 ? 0 : gapOpen + len * gapExtend; /* ANW.cpp:43-53 */
            else if (algo == DPX_K_ASG) v = i == 0 ? 0 : gapOpen + i * gapExtend; /* ASG: free row 0, ANW's column 0 */
            else v = 0;                                              /* LSW / BSW / ASW */
        } else if (algo == DPX_K_BSW) {
            const int dlt = i - j;
            v = (dlt <= band - 1 && -dlt <= band - 1) ? mat[pr.matOff + dpx_band_index(i, j, band, pr.chunkStride)] : 0;
        } else {
            v = mat[pr.matOff + dpx_cell_index(i, j, n, R, plane, planes, pr.chunkStride, pr.lanes)];
        }
        out[idx] = (int16_t)v;
    }
}

/* =====================================================================================================
 * Device traceback (the reference's on-device backtracking(), cuda/LNW/
 * LinearNeedlemanWunschV19.cu:26-110, and host back-trackers c++/backtrack.cpp:21-356).
 * One lane per pair walks back from the end cell.  Directions are not stored: they are recomputed from the
 * int16 score matrices with the reference's own tie rules (a >= b wins for the FIRST argument of __vibmax):
 *   LSW (c++/LinearSmithWaterman.cpp:106-108): UPPER, then LEFT, then CORNER; stop when the next cell is 0 (:222)
 *   LNW (c++/LinearNeedlemanWunsch.cpp:122-125): INSERTION if left >= max(up, diag), else DELETION if up >= diag
 *   ANW (c++/AffineNeedlemanWunsch.cpp:185-233, :258-360): 3-state walk over H / I / D, GAP_OPEN wins ties
 * The three lines (reference / relation / query) are written right-aligned into the pair's buffer.
 * ===================================================================================================== */
struct TbView {
    const int16_t *mat;
    uint64_t off;
    uint32_t cs, lanes;
    int n, m, R, planes, algo, band, gapOpen, gapExtend;
    __device__ __forceinline__ int get(int i, int j, int plane) const {
        if (i == 0 || j == 0) { /* closed-form borders, as in k_export_matrix */
            const int len = i + j;
            if (plane != 0) return 0;
            if (algo == DPX_K_LNW) return len * gapOpen;
            if (algo == DPX_K_ANW) return len == 0 ? 0 : gapOpen + len * gapExtend;
            return 0;
        }
        if (algo == DPX_K_BSW) {
            const int dlt = i - j;
            if (dlt > band - 1 || -dlt > band - 1) return 0;
            return mat[off + dpx_band_index(i, j, band, cs)];
        }
        return mat[off + dpx_cell_index(i, j, n, R, plane, planes, cs, lanes)];
    }
};

/* The H plane seen through two registers-resident column vectors.  In the wavefront-tiled and the tile layout with R >= 8 the 8 rows
 * (i0 & ~7 .. +7) of one column are 16 contiguous, 16-byte aligned bytes: `cur` holds them for column j, `prev` for
 * column j-1.  A path step then needs at most ONE new 16-byte load (the next column on a left / diagonal move; two when
 * the walk climbs into the 8-row group above) instead of three 2-byte loads that each miss every cache. */
struct TileWalker {
    const int16_t *mat;
    uint64_t off;
    uint32_t cs, lanes;
    int n, sr, border; /* sr = log2(rows per lane); border: value of H on row 0 / column 0 is border * (i + j) */
    int i = 0, j = 0;
    u32x4 cur, prev;

    __device__ __forceinline__ u32x4 column(int i0, int jj) const { /* the 8-row group of row i0 (0-based), column jj >= 1 */
        const int r = i0 & ((1 << sr) - 1), sub = r >> 3;
        uint64_t T, tile;
        if (lanes == 16) { /* tile layout: the column's 8 rows are one 16-byte piece of a line of the wave's stream (cs = first lane) */
            return *reinterpret_cast<const u32x4 *>(mat + off + (dpx_wtile_index(i0 + 1, jj, 0, 1, 1 << sr, cs) & ~(uint64_t)7));
        } else {
            const int k = i0 >> (sr + 6), l = (i0 >> sr) & 63;
            T = (uint64_t)k * (uint64_t)n + (uint64_t)(jj - 1) + (uint64_t)l;
            tile = (uint64_t)(((sub << 6) + l) << 3);
        }
        return *reinterpret_cast<const u32x4 *>(mat + off + T * (uint64_t)cs + tile);
    }
    static __device__ __forceinline__ int elem(const u32x4 &v, int rr) { /* int16 number rr (0..7) of the vector */
        const uint32_t d = rr < 4 ? (rr < 2 ? v.x : v.y) : (rr < 6 ? v.z : v.w);
        return (int)(int16_t)(d >> (16 * (rr & 1)));
    }
    __device__ __forceinline__ void load_both() {
        if (i >= 1 && j >= 1) cur = column(i - 1, j);
        if (i >= 1 && j >= 2) prev = column(i - 1, j - 1);
    }
    __device__ __forceinline__ void start(int i_, int j_) { i = i_; j = j_; load_both(); }
    /* a single cell outside the two cached columns' 8-row group (the row above the group): plain 2-byte load */
    __device__ __forceinline__ int single(int ii, int jj) const {
        if (ii == 0 || jj == 0) return border * (ii + jj);
        return mat[off + dpx_cell_index(ii, jj, n, 1 << sr, 0, 1, cs, lanes)];
    }
    __device__ __forceinline__ int here() const { return (i == 0 || j == 0) ? border * (i + j) : elem(cur, (i - 1) & 7); }
    __device__ __forceinline__ int up() const {
        if (i <= 1 || j == 0) return border * (i - 1 + j);
        const int rr = (i - 1) & 7;
        return rr ? elem(cur, rr - 1) : single(i - 1, j);
    }
    __device__ __forceinline__ int left() const {
        if (j <= 1 || i == 0) return border * (i + j - 1);
        return elem(prev, (i - 1) & 7);
    }
    __device__ __forceinline__ int diag() const {
        if (i <= 1 || j <= 1) return border * (i - 1 + j - 1);
        const int rr = (i - 1) & 7;
        return rr ? elem(prev, rr - 1) : single(i - 1, j - 1);
    }
    __device__ __forceinline__ void move(bool rowUp, bool colLeft) {
        const bool newGroup = rowUp && (((i - 1) & 7) == 0); /* leaving the 8-row group through its top row */
        i -= rowUp ? 1 : 0;
        j -= colLeft ? 1 : 0;
        if (i == 0 || j == 0) return; /* on the border: closed form from here on */
        if (newGroup) {
            load_both();
        } else if (colLeft) {
            cur = prev;
            if (j >= 2) prev = column(i - 1, j - 1);
        }
    }
};

/* one lane walks one pair (MODE 1: k_asw_traceback, algo DPX_K_ASW, the ANW walk's local form; MODE 2: k_asg_traceback, algo DPX_K_ASG, the ANW
 * walk under ASG's borders, which stops on row 0) */
template <int MODE>
__device__ void tb_walk_lane(const dpx_fill_args &a, const int p, int algo, int R, int planes, int cachedWalk, const int32_t *endRow,
                             const int32_t *endCol, const uint64_t *tbOff, char *tb, int32_t *tbLen) {
    const dpx_pair_dev pr = a.pairs[p];
    const int n = pr.n, m = pr.m;
    const unsigned char *ref = reinterpret_cast<const unsigned char *>(a.seq + pr.refIdx);
    const unsigned char *qry = reinterpret_cast<const unsigned char *>(a.seq + pr.qryIdx);
    const int cap = (m + n + 1 + 3) & ~3; /* line capacity, dword-aligned like tbOff[] (see EMIT) */
    char *lr = tb + tbOff[p], *lx = lr + cap, *lq = lx + cap;
    int pos = cap; /* lines grow from the back */
    uint32_t accR = 0, accX = 0, accQ = 0; /* the last <= 4 characters of each line, earliest in the highest byte */
    const int match = a.match, mismatch = a.mismatch;
    TbView v{a.mat, pr.matOff, pr.chunkStride, pr.lanes, n, m, pr.rows ? (int)pr.rows : R, planes, algo, a.band, a.gapOpen, a.gapExtend};
    /* Characters are produced back to front; four of them are collected per line and written as one aligned dword
     * (three scattered dword stores per four path steps instead of twelve byte stores). */
#define EMIT(rc_, xc_, qc_)                                                                      \
    {                                                                                            \
        --pos;                                                                                   \
        accR = (accR << 8) | (uint32_t)(unsigned char)(rc_);                                     \
        accX = (accX << 8) | (uint32_t)(unsigned char)(xc_);                                     \
        accQ = (accQ << 8) | (uint32_t)(unsigned char)(qc_);                                     \
        if ((pos & 3) == 0) {                                                                    \
            *reinterpret_cast<uint32_t *>(lr + pos) = accR;                                      \
            *reinterpret_cast<uint32_t *>(lx + pos) = accX;                                      \
            *reinterpret_cast<uint32_t *>(lq + pos) = accQ;                                      \
        }                                                                                        \
    }
    int i = endRow[p], j = endCol[p];
    CharWin qw{qry}, rw{ref};
    /* register-cached columns: LSW / LNW on the wavefront-tiled or the tile layout with 8-row sub-tiles (rows per lane >= 8), for
     * batches with enough lanes in flight that the walk is bound by sector requests (measured: 100k short pairs -25 %);
     * smaller batches are bound by the latency of one dependent load per step instead, and there the plain
     * three-loads-in-parallel step is the shorter chain (5000 x 1024^2: cached +40 %, 20k x 300^2: +10 %).  The host decides. */
    const bool cached = (algo == DPX_K_LSW || algo == DPX_K_LNW) && v.R >= 8 && cachedWalk && pr.lanes != 32;
    if (cached) {
        const int g = a.gapOpen;
        TileWalker w{a.mat, pr.matOff, pr.chunkStride, pr.lanes, n, dpx_log2(v.R), algo == DPX_K_LNW ? g : 0};
        w.start(i, j);
        if (algo == DPX_K_LSW) {
            int h = (i > 0 && j > 0) ? w.here() : 0;
            while (h > 0) {
                const int up = w.up(), left = w.left();
                if (up + g == h) { EMIT('_', ' ', qw.get(w.i - 1)); w.move(true, false); h = up; }
                else if (left + g == h) { EMIT(rw.get(w.j - 1), ' ', '_'); w.move(false, true); h = left; }
                else {
                    const int dg = w.diag(), qc = qw.get(w.i - 1), rc = rw.get(w.j - 1);
                    EMIT(rc, qc == rc ? '*' : '|', qc);
                    w.move(true, true);
                    h = dg;
                }
            }
        } else {
            while (w.i != 0 || w.j != 0) {
                if (w.i == 0) { EMIT(rw.get(w.j - 1), ' ', '_'); w.move(false, true); continue; }  /* row-0 border: QUERY_INSERTION */
                if (w.j == 0) { EMIT('_', ' ', qw.get(w.i - 1)); w.move(true, false); continue; }  /* column-0 border: QUERY_DELETION */
                const int qc = qw.get(w.i - 1), rc = rw.get(w.j - 1);
                const bool eq = qc == rc;
                const int mm = w.diag() + (eq ? match : mismatch);
                const int del = w.up() + g, ins = w.left() + g;
                const int vmax = max(del, mm);
                if (ins >= vmax) { EMIT(rc, ' ', '_'); w.move(false, true); }
                else if (del >= mm) { EMIT('_', ' ', qc); w.move(true, false); }
                else { EMIT(rc, eq ? '*' : '|', qc); w.move(true, true); }
            }
        }
    } else if (algo == DPX_K_LSW || algo == DPX_K_BSW) {
        const int g = a.gapOpen;
        int h = (i > 0 && j > 0) ? v.get(i, j, 0) : 0;
        while (h > 0) {
            const int up = v.get(i - 1, j, 0), left = v.get(i, j - 1, 0), dg = v.get(i - 1, j - 1, 0);
            if (up + g == h) { EMIT('_', ' ', qw.get(i - 1)); i--; h = up; }
            else if (left + g == h) { EMIT(rw.get(j - 1), ' ', '_'); j--; h = left; }
            else { const int qc = qw.get(i - 1), rc = rw.get(j - 1); EMIT(rc, qc == rc ? '*' : '|', qc); i--; j--; h = dg; }
        }
    } else if (algo == DPX_K_LNW) {
        const int g = a.gapOpen;
        while (i != 0 || j != 0) {
            if (i == 0) { EMIT(rw.get(j - 1), ' ', '_'); j--; continue; }  /* row-0 border: QUERY_INSERTION */
            if (j == 0) { EMIT('_', ' ', qw.get(i - 1)); i--; continue; }  /* column-0 border: QUERY_DELETION */
            const int qc = qw.get(i - 1), rc = rw.get(j - 1);
            const bool eq = qc == rc;
            const int mm = v.get(i - 1, j - 1, 0) + (eq ? match : mismatch);
            const int del = v.get(i - 1, j, 0) + g, ins = v.get(i, j - 1, 0) + g;
            const int vmax = max(del, mm);
            if (ins >= vmax) { EMIT(rc, ' ', '_'); j--; }
            else if (del >= mm) { EMIT('_', ' ', qc); i--; }
            else { EMIT(rc, eq ? '*' : '|', qc); i--; j--; }
        }
    } else { /* ANW; ASW (k_asw_traceback): the same walk, which stops where H = 0 and has no end gaps; ASG (k_asg_traceback): no row-0 tail */
        const int o = a.gapOpen, e = a.gapExtend;
        int cur = 0; /* 0 SCORING, 1 INSERTION, 2 DELETION */
        while (i != 0 && j != 0) {
            if (cur == 0) {
                if constexpr (MODE == 1) {
                    if (v.get(i, j, 0) <= 0) break;
                }
                const bool eq = qw.get(i - 1) == rw.get(j - 1);
                int dg;
                if constexpr (MODE == 2) dg = i == 1 ? 0 : (j == 1 ? o + (i - 1) * e : v.get(i - 1, j - 1, 0)); /* ASG's borders (the only border cell this walk reads) */
                else dg = v.get(i - 1, j - 1, 0);
                const int mm = dg + (eq ? match : mismatch);
                const int D = v.get(i, j, 2), I = v.get(i, j, 1);
                const int vmax = max(D, mm);
                if (I >= vmax) cur = 1;
                else if (D >= mm) cur = 2;
                else { EMIT(rw.get(j - 1), eq ? '*' : '|', qw.get(i - 1)); i--; j--; }
            } else if (cur == 1) {
                const bool open = (j == 1) || (v.get(i, j - 1, 0) + o + e >= v.get(i, j - 1, 1) + e);
                if (open) cur = 0;
                EMIT(rw.get(j - 1), ' ', '_'); j--;
            } else {
                const bool open = (i == 1) || (v.get(i - 1, j, 0) + o + e >= v.get(i - 1, j, 2) + e);
                if (open) cur = 0;
                EMIT('_', ' ', qw.get(i - 1)); i--;
            }
        }
        if constexpr (MODE != 1) {
            while (i > 0) { EMIT('_', ' ', qw.get(i - 1)); i--; }
            if constexpr (MODE == 0) {
                while (j > 0) { EMIT(rw.get(j - 1), ' ', '_'); j--; }
            }
        }
    }
#undef EMIT
    if (pos & 3) { /* the 1-3 newest characters have not filled a dword: the newest sits in the lowest byte, at `pos` */
        const int left = 4 - (pos & 3);
        for (int t = 0; t < left; t++) {
            lr[pos + t] = (char)(accR >> (8 * t)); lx[pos + t] = (char)(accX >> (8 * t)); lq[pos + t] = (char)(accQ >> (8 * t));
        }
    }
    tbLen[p] = cap - pos;
}

__global__ void k_traceback(const dpx_fill_args a, int numPairs, int algo, int R, int planes, int cachedWalk, const int32_t *endRow,
                            const int32_t *endCol, const uint64_t *tbOff, char *tb, int32_t *tbLen) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= numPairs) return;
    tb_walk_lane<0>(a, p, algo, R, planes, cachedWalk, endRow, endCol, tbOff, tb, tbLen);
}

__global__ void k_asw_traceback(const dpx_fill_args a, int numPairs, int R, int planes, const int32_t *endRow, const int32_t *endCol,
                                const uint64_t *tbOff, char *tb, int32_t *tbLen) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= numPairs) return;
    tb_walk_lane<1>(a, p, DPX_K_ASW, R, planes, 0, endRow, endCol, tbOff, tb, tbLen);
}

__global__ void k_asg_traceback(const dpx_fill_args a, int numPairs, int R, int planes, const int32_t *endRow, const int32_t *endCol,
                                const uint64_t *tbOff, char *tb, int32_t *tbLen) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= numPairs) return;
    tb_walk_lane<2>(a, p, DPX_K_ASG, R, planes, 0, endRow, endCol, tbOff, tb, tbLen);
}

/* -----------------------------------------------------------------------------------------------------
 * Wave-cooperative traceback (LSW / LNW / ANW / banded SW, every matrix layout of the fill kernels).
 * The lane-per-pair walk above pays one dependent HBM round trip per path step (1100 of them on a 1024 x 1024 pair).  Here
 * one WAVE owns a pair: lane c fetches column cLo + c of a window of the matrix around the walker -- 64 rows (ANW: 48 rows of
 * every plane) x 64 columns, the 8 rows of a row group with one 16-byte load (layouts with fewer than 8 rows per lane: 8- or
 * 4-byte pieces) -- into LDS (one 144-byte line per column and plane, borders included as ordinary cells), and the walk runs
 * until it leaves the window through its top or its left edge: one HBM round trip per ~64 steps of a diagonal path.
 * Round 4: the walk takes RUNS, not steps.  Round 3 walked on the scalar unit, one cell per trip: an LDS round trip for three
 * scores and two characters, five v_readfirstlane and the branches on them -- about 340 issue cycles per path step, and the
 * traceback of a batch cost as much as its fill (10 000 pairs of 1024 x 1024: 4.4 ms against 3.2 ms).  Which way the path leaves a
 * cell depends on that cell's neighbourhood only, so the 64 lanes each decide ONE cell of the line the path would follow next --
 * lane l the cell of the walker's diagonal in column l; in ANW's gap states the cells of the walker's row (INSERTION) or column
 * (DELETION) -- from four LDS reads at their own address, and a ballot gives the number of steps the path really follows that
 * line: the length of the run of "diagonal" decisions below the walker's lane (LSW: up / left / diagonal / stop at H = 0; LNW:
 * INSERTION over DELETION over diagonal, borders included; ANW: the SCORING state's choice, "the gap was opened here" for the two
 * gap states, c++/backtrack.cpp:214-356).  The lanes of the run store their own three characters.  Alignments worth computing
 * are mostly long diagonal runs: a 1024 x 1024 pair of the benchmark is ~90 trips instead of ~2050 -- ~50 since a trip also takes the
 * step that ENDS its run (the lane below the run has decided that cell in the same pass: a diagonal run and the single gap step
 * after it are one trip).  Measured per wave (s_memrealtime around the phases, 1024 x 1024 LSW): 19 windows of ~1.3 us load latency
 * on an idle chip (4 us with 1700 waves loading at once: ~200 distinct lines per wave and window against the CUs' miss queues) and
 * ~50 trips of 0.43 us; the batch's kernel time is its SLOWEST pair -- the benchmark's 1 % unrelated pairs, whose alignments under
 * +3 / -1 / -2 are 300 short runs: 0.19-0.25 ms against 0.06-0.13 for the others.  A prefetch of the next window along the diagonal
 * was built and measured (19 of 21 windows adopted): no gain with 1700 waves in flight (the loads are queued, not late), removed.
 * Banded SW (round 4, BAND): the same walk with LSW's rule; the window is gathered from the anti-diagonal-major band layout with
 * 2-byte loads (issue<3, .>), cells outside the band are 0.  4000 pairs of 4096 x 4096, band 128: 1.7 ms per batch of 1712 against
 * 10 ms for one lane per pair.
 * ----------------------------------------------------------------------------------------------------- */
template <int PLANES> struct TbWin {
    static constexpr int G = PLANES == 3 ? 6 : 8;      /* row groups of a window */
    static constexpr int WR = 8 * G;                   /* rows R0+1 .. R0+WR; columns cLo .. cLo+63, one per lane */
    static constexpr int CS = WR + 8;                  /* int16 elements between two columns in LDS: 16-byte aligned lines, banks spread */
    static constexpr int kBytes = PLANES * 64 * CS * 2;
};
size_t dpx_traceback_wave_lds(int planes) { return planes == 3 ? (size_t)TbWin<3>::kBytes : (size_t)TbWin<1>::kBytes; }

/* the 8 rows 8*grp+1 .. 8*grp+8 of column jc (>= 1) of `plane`, whatever the layout: one 16-byte piece where a lane owns >= 8 rows
 * (wavefront-tiled with 8-row sub-tiles, tile layout), otherwise the pieces of 8 / Rr neighbouring lanes (they sit in different chunks) */
__device__ __forceinline__ u32x4 tb_load_group8(const int16_t *base, const dpx_pair_dev &pr, const int Rr, const int planes, const int plane,
                                                const int grp, const int jc, const int n) {
    const int i1 = grp * 8 + 1;
    if (Rr >= 8) return *reinterpret_cast<const u32x4 *>(base + dpx_cell_index(i1, jc, n, Rr, plane, planes, pr.chunkStride, pr.lanes));
    if (Rr == 4) {
        const uint2 lo = *reinterpret_cast<const uint2 *>(base + dpx_cell_index(i1, jc, n, 4, plane, planes, pr.chunkStride, pr.lanes));
        const uint2 hi = *reinterpret_cast<const uint2 *>(base + dpx_cell_index(i1 + 4, jc, n, 4, plane, planes, pr.chunkStride, pr.lanes));
        return u32x4{lo.x, lo.y, hi.x, hi.y};
    }
    u32x4 v;
    v.x = *reinterpret_cast<const uint32_t *>(base + dpx_cell_index(i1, jc, n, 2, plane, planes, pr.chunkStride, pr.lanes));
    v.y = *reinterpret_cast<const uint32_t *>(base + dpx_cell_index(i1 + 2, jc, n, 2, plane, planes, pr.chunkStride, pr.lanes));
    v.z = *reinterpret_cast<const uint32_t *>(base + dpx_cell_index(i1 + 4, jc, n, 2, plane, planes, pr.chunkStride, pr.lanes));
    v.w = *reinterpret_cast<const uint32_t *>(base + dpx_cell_index(i1 + 6, jc, n, 2, plane, planes, pr.chunkStride, pr.lanes));
    return v;
}

template <int PLANES, bool BAND, int ALGO>
__global__ void __launch_bounds__(64) k_traceback_wave(const dpx_fill_args a, int numPairs, int R, const int32_t *endRow,
                                                       const int32_t *endCol, const uint64_t *tbOff, char *tb, int32_t *tbLen) {
    using W = TbWin<PLANES>;
    /* BAND: a banded SW matrix (anti-diagonal-major band layout, dpx_band_index) walked by LSW's rule; cells outside the band read 0
     * (TbView::get, c++/BandedSmithWaterman.cpp's back-tracker sees the zero-initialised matrix there) */
    constexpr int algo = BAND ? DPX_K_LSW : ALGO; /* (compile-time: the walk of one algorithm carries no branches for the others) */
    constexpr int G = W::G, WR = W::WR, CS = W::CS;
    extern __shared__ __attribute__((aligned(16))) unsigned char smemTb[];
    int16_t *win = reinterpret_cast<int16_t *>(smemTb); /* win[(plane * 64 + (jj - cLo)) * CS + (ii - R0 - 1)] = plane[ii][jj] */
    const int p = blockIdx.x;
    const int lane = threadIdx.x;
    if (p >= numPairs) return;
    const dpx_pair_dev pr = a.pairs[p];
    const int n = pr.n, m = pr.m;
    const int Rr = pr.rows ? (int)pr.rows : R;
    /* (the host launches this kernel for LSW / LNW / banded SW with one plane and ANW / ASW / ASG with three; rows per lane are
     * 2, 4, 8 or 16 in every full-matrix layout; empty sequences walk along a border or not at all) */
    const unsigned char *ref = reinterpret_cast<const unsigned char *>(a.seq + pr.refIdx);
    const unsigned char *qry = reinterpret_cast<const unsigned char *>(a.seq + pr.qryIdx);
    const int16_t *base = a.mat + pr.matOff;
    const int cap = (m + n + 1 + 3) & ~3;
    char *lr = tb + tbOff[p], *lx = lr + cap, *lq = lx + cap;
    int pos = cap;
    const int match = a.match, mismatch = a.mismatch, g = a.gapOpen, ext = a.gapExtend;
    /* H on row 0 / column 0, `len` cells from the corner (TbView::get): LNW len * gap, ANW open + len * extend (0 in the corner), LSW / ASW 0 */
    auto bval = [&](const int len) -> int { return algo == DPX_K_LNW ? len * g : ((algo == DPX_K_ANW || algo == DPX_K_ASG) ? (len ? g + len * ext : 0) : 0); };
    auto bvalRow = [&](const int len) -> int { return algo == DPX_K_ASG ? 0 : bval(len); }; /* ASG: row 0 is free, column 0 is ANW's */
    /* where the 16-byte piece (8 rows of a row group, one column) lies: shifts only for the two layouts whose lanes own >= 8 rows */
    const int Q = Rr >> 3, lgQ = Q == 2 ? 1 : 0;
    const int kind = Rr >= 8 ? (pr.lanes == 64 ? 0 : pr.lanes == 16 ? 1 : 2) : 2;
    const uint32_t cs = pr.chunkStride; /* (tile layout: the pair's first lane) */
    const int swBand = a.band, bandSc = BAND ? dpx_log2(dpx_band_cpl(a.band)) : 0; /* banded SW: band width, log2(cells per lane) */
    /* where the 16-byte piece (rows 8*grp+1 .. +8 of column jc, plane pl) lies, for the two layouts whose lanes own >= 8 rows */
    auto piece_at = [&](auto kindC, const int pl, const int grp, const int jc) -> const int16_t * {
        if constexpr (decltype(kindC)::value == 0) { /* wavefront-tiled (dpx_tiled_index + dpx_tile_off) */
            const int l = (grp >> lgQ) & 63, kk = grp >> (lgQ + 6), sub = grp & (Q - 1);
            const size_t T = (size_t)kk * (size_t)n + (size_t)(jc - 1) + (size_t)l;
            return base + T * cs + (size_t)(((((pl << lgQ) + sub) << 6) + l) << 3);
        } else { /* tile layout of the lane-packed kernels (dpx_wtile_index) */
            const int l = grp >> lgQ, h = grp & (Q - 1), lam = (int)cs + l, skew = l + ((int)cs & 7), j0 = jc - 1;
            const size_t t = (size_t)(((j0 >> 3) + 1) * 8 + skew - 1);
            return base + t * (size_t)(PLANES * Q * 512) + (size_t)((((pl << lgQ) + h) << 9) + ((lam >> 3) << 6) + ((j0 & 7) << 3));
        }
    };
    int i = __builtin_amdgcn_readfirstlane(endRow[p]), j = __builtin_amdgcn_readfirstlane(endCol[p]);
    int R0 = 1 << 28, cLo = 1 << 28;
    int diag0 = 0;        /* LSW / LNW: i - j of the cell the window was anchored on */
    bool banded = false;  /* ... and whether only the band around that diagonal was fetched */
    bool wantFull = false; /* the walk left the last band sideways (a long gap): fetch whole columns next time */
    uint32_t chR = 0u, chQ = 0u; /* reference character of this lane's column; query character of window row `lane` */
    /* window with (ii, jj) in its bottom-right corner region */
    /* Window with (ii, jj) in its bottom-right corner region.  Only a BAND of it is fetched unless the walk left the last one sideways
     * -- the three row groups of every column (and plane) around the diagonal through the anchor (rows d-8 .. d+7 at least, d = the
     * diagonal's row in that column).  The walk follows that diagonal or leaves it by a few gap steps; need_window() re-anchors when it
     * is more than 7 rows above / 6 below.  In the wavefront-tiled layouts every column's piece lies in its own 64-byte sector, so 3
     * instead of 8 pieces per column are 3/8 of the traffic and of the requests (the traceback of 10 000 pairs of 1024 x 1024 read
     * ~5 GB for paths that touch ~0.3 GB).
     * fill_window<KIND, CNT>: the loads of one layout (0 wavefront-tiled, 1 tile layout, 2 any layout through dpx_cell_index, 3 band
     * layout) and one group count, straight-line -- round 4 found a window's loads spending ~3000 cycles in the nest of uniform
     * branches that one loop over "whatever layout, however many groups" compiled to (a taken branch is a fetch bubble).  Cells
     * without storage (rows past m, columns outside 1..n, outside the band) load the pool's first bytes instead of branching and are
     * masked to 0 afterwards. */
    constexpr int GL = 3; /* row groups of a banded column */
    /* issue<KIND, CNT>: the loads of a window -- CNT row groups from group gBase + gFirst (per lane) of column jc, the query characters of
     * rows r0 + 1 + lane and the reference character of the column -- into `raw`, nothing else: no value is touched, so every load of the window is
     * in flight before the wave waits for the first. */
    auto issue = [&](auto kindC, auto cntC, auto &raw, uint32_t &rawQ, uint32_t &rawR, const int gBase, const int gFirst, const int jc, const int r0) {
        constexpr int KIND = decltype(kindC)::value, CNT = decltype(cntC)::value;
        if constexpr (KIND == 3) {
            /* Band layout (dpx_band_index, its shifts hoisted): the rows of a column lie on consecutive anti-diagonals -- 2-byte loads,
             * 24 per lane in a banded window (neighbouring columns and rows share 64-byte sectors: ~60 distinct ones for the wave). */
            const int sg = 3 - bandSc;
#pragma unroll
            for (int gi = 0; gi < CNT; gi++) {
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    const int ii2 = (gBase + gFirst + gi) * 8 + 1 + e, dlt = ii2 - jc, A = ii2 + jc - 2, sl = (dlt + swBand - 1) >> 1;
                    const bool ok = ii2 >= 1 && ii2 <= m && jc >= 1 && jc <= n && dlt < swBand && -dlt < swBand;
                    const size_t off = (size_t)(A >> sg) * cs + (size_t)(((sl >> bandSc) << 3) + ((A & ((1 << sg) - 1)) << bandSc) + (sl & ((1 << bandSc) - 1)));
                    const int16_t *at = ok ? base + off : a.mat;
                    raw[gi * 8 + e] = (uint32_t)*reinterpret_cast<const uint16_t *>(at);
                }
            }
        } else {
#pragma unroll
            for (int pl = 0; pl < PLANES; pl++) {
#pragma unroll
                for (int gi = 0; gi < CNT; gi++) {
                    const int grp = gBase + gFirst + gi;
                    const bool ok = grp >= 0 && grp * 8 < m && jc >= 1 && jc <= n;
                    u32x4 x;
                    if constexpr (KIND == 2) {
                        x = u32x4{0u, 0u, 0u, 0u};
                        if (ok) x = tb_load_group8(base, pr, Rr, PLANES, pl, grp, jc, n);
                    } else {
                        const int16_t *at = ok ? piece_at(kindC, pl, grp, jc) : a.mat;
                        x = *reinterpret_cast<const u32x4 *>(at);
                    }
                    const int k = (pl * CNT + gi) * 4;
                    raw[k] = x.x; raw[k + 1] = x.y; raw[k + 2] = x.z; raw[k + 3] = x.w;
                }
            }
        }
        const int qi = r0 + lane;
        const unsigned char *atQ = (lane < WR && qi >= 0 && qi < m) ? qry + qi : reinterpret_cast<const unsigned char *>(a.seq);
        const unsigned char *atR = (jc >= 1 && jc <= n) ? ref + (jc - 1) : reinterpret_cast<const unsigned char *>(a.seq);
        rawQ = *atQ;
        rawR = *atR;
    };
    /* commit<KIND, CNT>: what issue() loaded becomes the window in LDS -- cells without storage masked to 0, the borders of H added as
     * ordinary cells -- and the lane's two characters */
    auto commit = [&](auto kindC, auto cntC, const auto &raw, const uint32_t rawQ, const uint32_t rawR, const int gBase, const int gFirst, const int jc, const int r0) {
        constexpr int KIND = decltype(kindC)::value, CNT = decltype(cntC)::value;
        u32x4 v[PLANES][CNT];
        if constexpr (KIND == 3) {
#pragma unroll
            for (int gi = 0; gi < CNT; gi++) {
                uint32_t d[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    const int ii2 = (gBase + gFirst + gi) * 8 + 1 + e, dlt = ii2 - jc;
                    const bool ok = ii2 >= 1 && ii2 <= m && jc >= 1 && jc <= n && dlt < swBand && -dlt < swBand;
                    d[e >> 1] |= (ok ? raw[gi * 8 + e] : 0u) << ((e & 1) * 16);
                }
                v[0][gi] = u32x4{d[0], d[1], d[2], d[3]};
            }
        } else {
#pragma unroll
            for (int pl = 0; pl < PLANES; pl++) {
#pragma unroll
                for (int gi = 0; gi < CNT; gi++) {
                    const int grp = gBase + gFirst + gi, k = (pl * CNT + gi) * 4;
                    const bool ok = grp >= 0 && grp * 8 < m && jc >= 1 && jc <= n;
                    v[pl][gi] = ok ? u32x4{raw[k], raw[k + 1], raw[k + 2], raw[k + 3]} : u32x4{0u, 0u, 0u, 0u};
                }
            }
        }
        { const int qi = r0 + lane; chQ = (lane < WR && qi >= 0 && qi < m) ? rawQ : 0u; } /* query character of row r0 + 1 + lane */
        chR = (jc >= 1 && jc <= n) ? rawR : 0u;
        if (algo != DPX_K_LSW && algo != DPX_K_ASW) { /* the borders of H as cells: column 0 and row 0 (LSW / ASW: zeros, as loaded) */
#pragma unroll
            for (int gi = 0; gi < CNT; gi++) {
                const int grp = gBase + gFirst + gi;
                if (jc == 0 || grp < 0) {
                    uint32_t d[4];
#pragma unroll
                    for (int e = 0; e < 8; e += 2) {
                        const int r0b = grp * 8 + 1 + e, r1b = r0b + 1;
                        const int v0 = jc == 0 ? (r0b >= 0 ? bval(r0b) : 0) : (r0b == 0 && jc > 0 ? bvalRow(jc) : 0);
                        const int v1 = jc == 0 ? (r1b >= 0 ? bval(r1b) : 0) : (r1b == 0 && jc > 0 ? bvalRow(jc) : 0);
                        d[e >> 1] = ((uint32_t)(uint16_t)v1 << 16) | (uint32_t)(uint16_t)v0;
                    }
                    v[0][gi] = u32x4{d[0], d[1], d[2], d[3]};
                }
            }
        }
#pragma unroll
        for (int pl = 0; pl < PLANES; pl++)
#pragma unroll
            for (int gi = 0; gi < CNT; gi++) *reinterpret_cast<u32x4 *>(win + (pl * 64 + lane) * CS + (gFirst + gi) * 8) = v[pl][gi];
    };
    /* first fetched row group (relative to the window's first) of this lane's column in a banded window whose last column holds the
     * diagonal's row iiDiag */
    auto band_first = [&](const int iiDiag, const int r0) -> int {
        const int dl = (iiDiag - r0 - 1) - 63 + lane;
        return min(max((dl - 8) >> 3, 0), G - GL);
    };
    constexpr int kRawFull = BAND ? G * 8 : PLANES * G * 4, kRawBand = BAND ? GL * 8 : PLANES * GL * 4;
    using std::integral_constant;
    auto load_window = [&](const int ii, const int jj) {
        const int gBase = ((ii - 1) >> 3) - (G - 1);
        R0 = gBase * 8;
        cLo = jj - 63;
        const int jc = cLo + lane;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local"); /* the previous window's reads are done before it is overwritten (LDS only: the walk's byte stores are not waited for) */
        __builtin_amdgcn_wave_barrier();
        diag0 = ii - jj;
        banded = !wantFull;
        const int gFirst = banded ? band_first(ii, R0) : 0;
        uint32_t rq, rr;
        auto both = [&](auto kindC, auto cntC, auto &raw) {
            issue(kindC, cntC, raw, rq, rr, gBase, gFirst, jc, R0);
            commit(kindC, cntC, raw, rq, rr, gBase, gFirst, jc, R0);
        };
        if (banded) {
            uint32_t raw[kRawBand];
            if constexpr (BAND) both(integral_constant<int, 3>{}, integral_constant<int, GL>{}, raw);
            else if (kind == 0) both(integral_constant<int, 0>{}, integral_constant<int, GL>{}, raw);
            else if (kind == 1) both(integral_constant<int, 1>{}, integral_constant<int, GL>{}, raw);
            else both(integral_constant<int, 2>{}, integral_constant<int, GL>{}, raw);
        } else {
            uint32_t raw[kRawFull];
            if constexpr (BAND) both(integral_constant<int, 3>{}, integral_constant<int, G>{}, raw);
            else if (kind == 0) both(integral_constant<int, 0>{}, integral_constant<int, G>{}, raw);
            else if (kind == 1) both(integral_constant<int, 1>{}, integral_constant<int, G>{}, raw);
            else both(integral_constant<int, 2>{}, integral_constant<int, G>{}, raw);
        }
        /* the two characters are needed HERE: without this the compiler waits for them (s_waitcnt vmcnt(0)) where the walk first uses them --
         * in every trip of the loop, where the wait also covers the byte stores of the previous trips (3 us per trip, measured) */
        asm volatile("" : "+v"(chQ), "+v"(chR));
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
    };
    /* rows i-1, i and columns j-1, j must lie inside the window (borders are cells of it) */
    auto need_window = [&]() -> bool {
        if (i - 1 <= R0 || i > R0 + WR || j - 1 < cLo || j > cLo + 63) return true;
        if (banded) { const int dev = (i - j) - diag0; if (dev < -7 || dev > 6) { wantFull = true; return true; } } /* outside the fetched band */
        return false;
    };
    auto cell = [&](const int pl, const int col, const int row) -> int { return (int)win[(pl * 64 + col) * CS + row]; };
    /* number of lanes that continue a run which starts at lane `from` and goes DOWN the lanes while `on` holds (lane 0 is never on) */
    auto run_down = [&](const bool on, const int from) -> int {
        const unsigned long long inv = ~__builtin_amdgcn_ballot_w64(on) << (63 - from);
        return inv ? __builtin_clzll(inv) : 64;
    };
    /* Decision of window cell (rq, cq) (>= 1 each: callers clamp), rc = the reference character of its column: 0 diagonal, 1 up, 2 left,
     * 3 stop / other (ANW: the SCORING state's 1 = to INSERTION, 2 = to DELETION).  qcOut = the query character of its row. */
    auto decide_cell = [&](const int rq, const int cq, const uint32_t rc, int &qcOut) -> uint32_t {
        const int qc = __builtin_amdgcn_ds_bpermute(rq << 2, (int)chQ);
        qcOut = qc;
        const int ii = R0 + 1 + rq, jc = cLo + cq;
        uint32_t d;
        if constexpr (PLANES == 1) {
            const int h = cell(0, cq, rq), up = cell(0, cq, rq - 1), left = cell(0, cq - 1, rq);
            if (algo == DPX_K_LSW) {
                d = h <= 0 ? 3u : (up + g == h ? 1u : (left + g == h ? 2u : 0u)); /* UPPER, LEFT, CORNER; stop at 0 (c++/backtrack.cpp:21-97) */
            } else {
                const int dg = cell(0, cq - 1, rq - 1);
                const int mm = dg + ((uint32_t)qc == rc ? match : mismatch);
                const int del = up + g, ins = left + g;
                d = ins >= max(del, mm) ? 2u : (del >= mm ? 1u : 0u); /* INSERTION over DELETION over the diagonal */
                if (ii == 0) d = 2u;       /* row 0: QUERY_INSERTION to the corner */
                else if (jc == 0) d = 1u;  /* column 0: QUERY_DELETION */
            }
        } else {
            const int dg = cell(0, cq - 1, rq - 1), I = cell(1, cq, rq), D = cell(2, cq, rq);
            const int mm = dg + ((uint32_t)qc == rc ? match : mismatch);
            d = I >= max(D, mm) ? 1u : (D >= mm ? 2u : 0u);
            if (algo == DPX_K_ASW && cell(0, cq, rq) <= 0) d = 3u; /* ASW: H = 0, the local alignment starts here */
            if (ii <= 0 || jc <= 0) d = 3u;
        }
        return d;
    };
    /* (r, c) = the walker's window cell; lane l decides the cell of the walker's diagonal in its own column (3 outside the usable part) */
    auto decide_diag = [&](const int r, const int c, int &qcOut) -> uint32_t {
        const int rr = r - (c - lane);
        const bool usable = lane <= c && lane >= 1 && rr >= 1;
        const uint32_t d = decide_cell(usable ? rr : 1, usable ? lane : 1, chR, qcOut); /* (clamped: every lane reads inside the window) */
        return usable ? d : 3u;
    };
    /* LSW / LNW gaps in runs as well (round 4: the end gaps of a global alignment of short reads are 30 steps along one row): the cells to the
     * left of the walker on its row (lane l: column l) or above it in its column (lane k: k rows up) that decide like it.  In a banded
     * window a run ends where it leaves the fetched band (`dev` = the walker's distance from the anchor's diagonal). */
    auto left_run = [&](const int r, const int c, const int dev) -> int {
        int qc;
        const bool usable = lane <= c && lane >= 1 && (!banded || dev + (c - lane) <= 6);
        const uint32_t d = decide_cell(r, usable ? lane : 1, chR, qc);
        return run_down(usable && d == 2u, c);
    };
    auto up_run = [&](const int r, const int c, const int dev) -> int {
        int qc;
        const bool usable = r - lane >= 1 && (!banded || dev - lane >= -7);
        const uint32_t d = decide_cell(usable ? r - lane : 1, c, (uint32_t)__builtin_amdgcn_readlane((int)chR, c), qc);
        const unsigned long long ends = __builtin_amdgcn_ballot_w64(!(usable && d == 1u));
        return ends ? __builtin_ctzll(ends) : 64;
    };
    /* the lanes c, c-1, ... c-len+1 store the characters of a diagonal run (their own column's reference character, their row's query character) */
    auto emit_diag = [&](const int c, const int len, const int qc) {
        const int k = c - lane;
        if (k >= 0 && k < len) {
            const int at = pos - 1 - k;
            lr[at] = (char)chR; lx[at] = ((uint32_t)qc == chR) ? '*' : '|'; lq[at] = (char)qc;
        }
        pos -= len;
    };
    /* `len` steps to the left from column c: the lanes store their reference characters against gaps */
    auto emit_left = [&](const int c, const int len) {
        const int k = c - lane;
        if (k >= 0 && k < len) { const int at = pos - 1 - k; lr[at] = (char)chR; lx[at] = ' '; lq[at] = '_'; }
        pos -= len;
    };
    /* `len` steps up from row r: lane k stores the query character of row r - k */
    auto emit_up = [&](const int r, const int len) {
        const int qc = __builtin_amdgcn_ds_bpermute(max(r - lane, 0) << 2, (int)chQ);
        if (lane < len) { const int at = pos - 1 - lane; lr[at] = '_'; lx[at] = ' '; lq[at] = (char)qc; }
        pos -= len;
    };
    int cur = 0; /* ANW: 0 SCORING, 1 INSERTION, 2 DELETION */
    for (;;) {
        if ((algo == DPX_K_LSW || algo == DPX_K_ASW) ? !(i > 0 && j > 0) : (algo == DPX_K_ASG ? i == 0 : !(i != 0 || j != 0))) break; /* (ASG: row 0 ends the walk) */
        if (need_window()) { load_window(max(i, 1), max(j, 1)); wantFull = false; } /* (a window anchored on row 1 / column 1 also serves row 0 / column 0) */
        const int r = i - R0 - 1, c = j - cLo;
        if constexpr (PLANES == 1) {
            if (algo != DPX_K_LSW && (i == 0 || j == 0)) { /* LNW on a border: to the corner in runs (row 0: QUERY_INSERTION, column 0: QUERY_DELETION) */
                if (i == 0) { const int len = min(j, c); emit_left(c, len); j -= len; }
                else { const int len = min(i, r); emit_up(r, len); i -= len; }
                continue;
            }
            int qc;
            const uint32_t d = decide_diag(r, c, qc);
            const int run = run_down(d == 0u, c);
            if (run) {
                /* ... and the step that ends the run with it: the lane below the run has decided that cell already (paths of related
                 * sequences are diagonal runs separated by single gap steps: half the trips) */
                emit_diag(c, run, qc); i -= run; j -= run;
                const int cx = c - run, rx = r - run;
                if (cx >= 1 && rx >= 1 && i > 0 && j > 0) {
                    const uint32_t dx = (uint32_t)__builtin_amdgcn_readlane((int)d, cx);
                    if (dx == 1u) { emit_up(rx, 1); i--; }
                    else if (dx == 2u) { emit_left(cx, 1); j--; }
                    else if (algo == DPX_K_LSW) break; /* H = 0: the local alignment starts here */
                }
                continue;
            }
            const uint32_t dc = (uint32_t)__builtin_amdgcn_readlane((int)d, c);
            if (algo == DPX_K_LSW && dc == 3u) break;
            const int dev = (i - j) - diag0;
            if (dc == 1u) { const int len = max(up_run(r, c, dev), 1); emit_up(r, len); i -= len; }
            else { const int len = max(left_run(r, c, dev), 1); emit_left(c, len); j -= len; }
        } else {
            if (i == 0 || j == 0) { /* along a border to the corner: first up column 0, then left along row 0 (c++/backtrack.cpp:214-356) */
                if (i > 0) { const int len = min(i, r); emit_up(r, len); i -= len; }   /* (rows r, r-1, ... 1 of the window hold query rows) */
                else { const int len = min(j, c); emit_left(c, len); j -= len; }
                continue;
            }
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
                        else if (algo == DPX_K_ASW) break; /* H = 0 */
                    }
                    continue;
                }
                cur = __builtin_amdgcn_readlane((int)d, c); /* 1: to INSERTION, 2: to DELETION */
                if (algo == DPX_K_ASW && cur == 3) break;    /* (ASW: 3 = H is 0 here) */
            } else if (cur == 1) {
                /* INSERTION: steps to the left along row r until (and including) the cell where the gap was opened; lane l decides the cell in column l */
                const int cq = max(lane, 1), jc = cLo + cq;
                const bool opened = jc == 1 || cell(0, cq - 1, r) + g + ext >= cell(1, cq - 1, r) + ext;
                const bool usable = lane <= c && lane >= 1 && jc >= 1 && (!banded || (i - j) - diag0 + (c - lane) <= 6); /* (column l-1, row r inside the band) */
                const int cont = run_down(usable && !opened, c);          /* cells the gap passes through */
                const bool stops = c - cont >= 1 && cLo + c - cont >= 1 && (!banded || (i - j) - diag0 + cont <= 6); /* ... and then a usable cell that opened it (else: the window's / band's edge) */
                const int len = cont + (stops ? 1 : 0);
                emit_left(c, len); j -= len;
                if (stops) cur = 0;
            } else {
                /* DELETION: steps up along column c; lane k decides the cell k rows above the walker */
                const int rq = max(r - lane, 1), ii = R0 + 1 + rq;
                const bool opened = ii == 1 || cell(0, c, rq - 1) + g + ext >= cell(2, c, rq - 1) + ext;
                const bool usable = r - lane >= 1 && ii >= 1 && (!banded || (i - j) - diag0 - lane >= -7); /* (column c, row r-k-1 inside the band) */
                const unsigned long long m64 = __builtin_amdgcn_ballot_w64(!(usable && !opened)); /* first lane that ends the run: opened, or not usable */
                const int cont = m64 ? __builtin_ctzll(m64) : 64;
                const bool stops = r - cont >= 1 && R0 + 1 + r - cont >= 1 && (!banded || (i - j) - diag0 - cont >= -7);
                const int len = cont + (stops ? 1 : 0);
                emit_up(r, len); i -= len;
                if (stops) cur = 0;
            }
        }
    }
    if (lane == 0) tbLen[p] = cap - pos;
}

} // namespace

hipError_t dpx_launch_export(const int16_t *mat, const dpx_pair_dev &pr, int algo, int R, int planes, int plane, int gapOpen,
                             int gapExtend, int band, int16_t *out, hipStream_t stream) {
    const size_t total = (size_t)(pr.m + 1) * (size_t)(pr.n + 1);
    unsigned blocks = (unsigned)((total + 255) / 256);
    if (blocks > 4096u) blocks = 4096u;
    hipLaunchKernelGGL(k_export_matrix, dim3(blocks), dim3(256), 0, stream, mat, pr, algo, R, planes, plane, gapOpen,
                       gapExtend, band, out);
    return hipGetLastError();
}

hipError_t dpx_launch_traceback(const dpx_fill_args &a, int numPairs, int algo, int R, int planes, int walk,
                                const uint64_t *tbOff, char *tb, int32_t *tbLen, hipStream_t stream) {
    if (numPairs <= 0) return hipSuccess;
    const bool cachedWalk = walk == 1;
    if (walk == 2) { /* one wave per pair with an LDS window (k_traceback_wave) */
        const bool affine = algo == DPX_K_ANW || algo == DPX_K_ASW || algo == DPX_K_ASG;
        const size_t lds = dpx_traceback_wave_lds(affine ? 3 : 1);
        auto wave = [&](auto planesC, auto bandC, auto algoC) {
            hipLaunchKernelGGL((k_traceback_wave<decltype(planesC)::value, decltype(bandC)::value, decltype(algoC)::value>), dim3((unsigned)numPairs),
                               dim3(64), lds, stream, a, numPairs, R, a.endRow, a.endCol, tbOff, tb, tbLen);
        };
        if (algo == DPX_K_ANW) wave(int_c<3>{}, bool_c<false>{}, int_c<DPX_K_ANW>{});
        else if (algo == DPX_K_ASW) wave(int_c<3>{}, bool_c<false>{}, int_c<DPX_K_ASW>{});
        else if (algo == DPX_K_ASG) wave(int_c<3>{}, bool_c<false>{}, int_c<DPX_K_ASG>{});
        else if (algo == DPX_K_BSW) wave(int_c<1>{}, bool_c<true>{}, int_c<DPX_K_LSW>{});
        else if (algo == DPX_K_LNW) wave(int_c<1>{}, bool_c<false>{}, int_c<DPX_K_LNW>{});
        else wave(int_c<1>{}, bool_c<false>{}, int_c<DPX_K_LSW>{});
        return hipGetLastError();
    }
    if (algo == DPX_K_ASW) /* (walk 1 caches linear-gap columns only: the ASW walk is walk 0's) */
        hipLaunchKernelGGL(k_asw_traceback, dim3((unsigned)((numPairs + 63) / 64)), dim3(64), 0, stream, a, numPairs, R, planes, a.endRow,
                           a.endCol, tbOff, tb, tbLen);
    else if (algo == DPX_K_ASG) /* (likewise; ASG's borders are this walk's own) */
        hipLaunchKernelGGL(k_asg_traceback, dim3((unsigned)((numPairs + 63) / 64)), dim3(64), 0, stream, a, numPairs, R, planes, a.endRow,
                           a.endCol, tbOff, tb, tbLen);
    else
        hipLaunchKernelGGL(k_traceback, dim3((unsigned)((numPairs + 63) / 64)), dim3(64), 0, stream, a, numPairs, algo, R, planes,
                           cachedWalk ? 1 : 0, a.endRow, a.endCol, tbOff, tb, tbLen);
    return hipGetLastError();
}
