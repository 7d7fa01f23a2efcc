/*
 * dpx_kernels.hip -- hand-written gfx950 (CDNA4) kernels of the pairwise-alignment DP fill: the linear-gap fills (LNW / LSW), the
 * headline.  The other families have units of their own: dpx_affine_kernels.hip (Gotoh fills), dpx_bsw_kernels.hip (banded SW),
 * dpx_traceback_kernels.hip (matrix export and the walks), dpx_output_kernels.hip (result text); dpx_device.hpp and
 * dpx_fill_common.hpp hold what they share.
 *
 * One 64-lane wavefront per alignment pair.  Lane l owns R consecutive query rows of a 64*R-row stripe and
 * sweeps the reference columns with a skew of one column per lane, so the wave is always on one anti-diagonal
 * (of R-row tiles).  Per step and lane:
 *   - `up` of the lane's top row comes from the previous lane's bottom row through ONE DPP move
 *     (v_mov_b32_dpp wave_shr:1 -- the reference's __shfl_up_sync, cuda/LNW/LinearNeedlemanWunschV12.cu:149);
 *     the diagonal is last step's `up`, carried in a register (the V10 trick, V10.cu:157-162);
 *   - the R cells of the lane are chained in registers (left/diag/up never touch memory);
 *   - the stripe's bottom row goes to LDS for the next stripe (V12.cu:110-113,141-143: warpEdgeScore);
 *   - the cell update is v_cmp/v_cndmask + v_add + v_max + v_add + v_max3_i32 (FakeDPX __vibmax/__vimax3,
 *     c++/FakeDPX.cpp:11-13,145-153; the >= predicates are not needed here because the traceback recomputes
 *     directions from the stored scores with the same rule);
 *   - the wave's R x 64 scores of this step leave as one fully coalesced int16 store (dpx_layout.h).
 * No MFMA (integer max-plus recurrence), no LDS transposes, no atomics.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "dpx_fill_common.hpp"
#include "dpx_kernels.h"
#include "dpx_layout.h"
#include "dpx_prims.hpp"

namespace {

using dpx::pack_lo16;
using dpx::wave_shr1;
using dpx::wave_shl1;
using dpx::s16x2;
using dpx::u16x2;
using dpx::as_s16x2;
using dpx::as_u16x2;
using dpx::as_u32;
using namespace dpx_dev;
using namespace dpx_fill;

/* =====================================================================================================
 * Linear-gap fill: LinearNeedlemanWunsch (LOCAL = false) and LinearSmithWaterman (LOCAL = true).
 *   NW cell (c++/LinearNeedlemanWunsch.cpp:105-128):  H = max(left+g, max(up+g, diag+s))
 *   SW cell (c++/LinearSmithWaterman.cpp:82-103):     H = max(0, max(up+g, left+g, diag+s))
 * ===================================================================================================== */
template <int R, bool LOCAL>
struct LinState {
    int Hl[R];        /* H[row][j-1] of the lane's R rows (the "left" values, then overwritten by H[row][j]) */
    int qc[R];        /* query characters of the lane's rows */
    unsigned key[R];  /* SW: per-row running max of (H << 16 | 0xFFFF - j): max score, then smallest column */
    int dtop;         /* H[row0][j-1]: diagonal of the lane's top row */
};

/* the R chained cells of one lane for one column (shared by the striped and the rolling schedule) */
template <int R, bool LOCAL, bool KEYS>
__device__ __forceinline__ void lin_cells(LinState<R, LOCAL> &st, const int upin, const int rc, const int j, const int match,
                                          const int mismatch, const int gap) {
    int u = upin, d = st.dtop;
    const unsigned negj = 0xFFFFu - (unsigned)j;
#if DPX_EXP_NOCOMPUTE /* ablation build only (tools/): stores without the recurrence */
    st.Hl[0] += u + d + rc + (int)negj;
#else
    /* the diagonal terms first (row r's diagonal is row r-1's LEFT value), then every row in place: the new H[r] overwrites the old
     * one in its own register.  Written the other way round (diagonal taken from a rotating `d`) the values move one register
     * down per step and the compiler has to move them back at the loop edge: 8 v_mov per step at R = 8 (round 3, ISA of
     * k_linear_lanes: 74 vector instructions per step, of which 48 are the recurrence) */
    int dterm[R];
#pragma unroll
    for (int r = 0; r < R; r++) dterm[r] = ((r == 0) ? d : st.Hl[r - 1]) + ((st.qc[r] == rc) ? match : mismatch);
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int g = max(u, st.Hl[r]) + gap;
        int h;
        if constexpr (LOCAL) h = max(max(g, dterm[r]), 0); /* v_max3_i32 */
        else h = max(g, dterm[r]);
        u = h;
        st.Hl[r] = h;
        if constexpr (LOCAL && KEYS) st.key[r] = max(st.key[r], ((unsigned)h << 16) | negj);
    }
#endif
    st.dtop = upin;
}

/* The cell update of the int32 kernels (round 3; k_linear_stream still uses lin_cells).  The lane's state is kept as Hg = H + gap: then
 *     H[r][j] = max3(Hg[r-1][j], Hg[r][j-1], Hg[r-1][j-1] + (s - gap))          (one v_max3_i32, SW: the diagonal term clamped at 0 first)
 * and Hg[r][j] = H[r][j] + gap is the only op left on the chain from one row to the next: 5 vector instructions per NW cell
 * instead of 6 (v_cmp, v_cndmask, v_add, v_max3, v_add), two dependent ones per row instead of three.  The diagonal terms are
 * computed first and every row is updated in place (no register rotation, see lin_cells).  h[] returns the plain scores. */
template <int R, bool LOCAL>
__device__ __forceinline__ void lin_cells_g(LinState<R, LOCAL> &st, const int upinG, const int rc, const unsigned negj, const int matchG,
                                            const int mismatchG, const int gap, int (&h)[R]) {
    int dterm[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        dterm[r] = ((r == 0) ? st.dtop : st.Hl[r - 1]) + ((st.qc[r] == rc) ? matchG : mismatchG);
        if constexpr (LOCAL) dterm[r] = max(dterm[r], 0);
    }
    int ug = upinG;
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int v = max(max(ug, st.Hl[r]), dterm[r]); /* v_max3_i32 */
        h[r] = v;
        ug = v + gap;
        st.Hl[r] = ug;
        if constexpr (LOCAL) st.key[r] = max(st.key[r], ((unsigned)v << 16) | negj);
    }
    st.dtop = upinG;
}

/* pack the lane's R scores into R/2 dwords (the store format) */
template <int R, bool LOCAL>
__device__ __forceinline__ void lin_pack(LinState<R, LOCAL> &st, uint32_t (&w)[(R + 1) / 2]) {
#pragma unroll
    for (int q = 0; q < R / 2; q++) w[q] = pack_lo16(st.Hl[2 * q], st.Hl[2 * q + 1]);
}

template <int R>
__device__ __forceinline__ void store_words(int16_t *dst, const uint32_t (&w)[(R + 1) / 2]) {
    if constexpr (R == 2) {
        stream_store(reinterpret_cast<uint32_t *>(dst), w[0]);
    } else if constexpr (R == 4) {
        u32x2 v = {w[0], w[1]};
        stream_store(reinterpret_cast<u32x2 *>(dst), v);
    } else {
#pragma unroll
        for (int q = 0; q < R / 8; q++) {
            u32x4 v = {w[4 * q + 0], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]};
            stream_store(reinterpret_cast<u32x4 *>(dst + q * 512), v); /* sub-tile q: its own 1 KiB [lane][8] block */
        }
    }
}

/* WHOLE: store for every lane (the chunk is private to this stripe); otherwise only lanes on a real cell store.
 * SW tracks per-row (score, column) keys in registers, so the start cell needs no second pass over the matrix. */
template <int R, bool LOCAL, bool STORE, bool MASKED, bool WHOLE>
__device__ __forceinline__ void lin_step(LinState<R, LOCAL> &st, const int t, const int lane, const int n,
                                         const bool laneHasRows, const int matchG, const int mismatchG, const int gap,
                                         const int e0, const int rc, int16_t *edge, const bool writeEdge,
                                         int16_t *tileDst, const int storeLanes, const int rampLines) {
    /* the state is H + gap (lin_cells_g); e0 = the plain H of the row above lane 0 (edge row / row-0 border) */
    const int j = t - lane + 1;
    /* cross-lane traffic happens with all lanes enabled: a finished lane must still feed its neighbour */
    const int upin = wave_shr1(st.Hl[R - 1], e0 + gap);
    bool active = true;
    if constexpr (MASKED) active = laneHasRows && (j >= 1) && (j <= n);
    uint32_t w[(R + 1) / 2];
    if (active) {
        int h[R];
        lin_cells_g<R, LOCAL>(st, upin, rc, 0xFFFFu - (unsigned)j, matchG, mismatchG, gap, h);
        if (writeEdge && lane == 63) edge[j] = (int16_t)h[R - 1];
        if constexpr (STORE) {
#pragma unroll
            for (int q = 0; q < R / 2; q++) w[q] = pack_lo16(h[2 * q], h[2 * q + 1]);
            if constexpr (MASKED && !WHOLE) store_words<R>(tileDst, w);
        }
    } else if constexpr (STORE) {
        lin_pack<R, LOCAL>(st, w); /* (a lane that is not on a cell stores into padding that nothing reads: any value) */
    }
    /* Every lane stores, also lanes that are not on a real cell during the skew ramps: the wave then always writes
     * its whole 64*R*2-byte chunk.  Partial chunks (masked stores) measured ~2.5x the cost of full ones -- a chunk
     * with a partly written 64-B sector becomes a read-modify-write at the HBM.  The extra bytes land in the skew
     * padding of the pair's block, which nothing ever reads. */
    if constexpr (STORE && (!MASKED || WHOLE) && !(MASKED && DPX_EXP_NORAMPSTORE)) {
        bool doStore = lane < storeLanes; /* storeLanes == 64 unless the pair is shorter than the stripe */
        if constexpr (MASKED) doStore = doStore && ramp_stores<R>(lane, t, n, rampLines);
        if (doStore) store_words<R>(tileDst, w);
    }
}

template <int R, bool LOCAL, bool STORE>
__global__ void __launch_bounds__(DPX_FILL_THREADS) k_linear_fill(const dpx_fill_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int p = blockIdx.x * (int)a.wavesPerBlock + wv; /* wave-uniform: everything per-pair lives in SGPRs */
    if (p >= a.numPairs) return;
    if (a.order) p = a.order[p];
    const dpx_pair_dev pr = a.pairs[p];
    const int n = pr.n, m = pr.m;
    const int gap = a.gapOpen, matchG = a.match - gap, mismatchG = a.mismatch - gap; /* the lanes' state is H + gap (lin_cells_g) */

    if (m <= 0 || n <= 0) { /* empty sequence: only borders exist */
        if (lane == 0) {
            a.score[p] = LOCAL ? 0 : (m <= 0 ? n * gap : m * gap);
            a.endRow[p] = LOCAL ? 0 : max(m, 0);
            a.endCol[p] = LOCAL ? 0 : max(n, 0);
        }
        return;
    }
    const unsigned char *ref = reinterpret_cast<const unsigned char *>(a.seq + pr.refIdx);
    const unsigned char *qry = reinterpret_cast<const unsigned char *>(a.seq + pr.qryIdx);
    unsigned char *my = smem + (size_t)wv * a.ldsPerWave;
    int16_t *edge = reinterpret_cast<int16_t *>(my); /* edge[j], j = 0..n+1: H of the row above the current stripe */
    /* refl[64 + (j-1)], 64 bytes of slack either side; staged with 16-byte loads (stage_bytes) */
    const unsigned char *refl = stage_bytes(my + a.ldsRefOff + 64, ref, n, lane, 64) - 64;
    /* row-0 border (LinearNeedlemanWunsch.cpp:38-41; all zero for SW) is the first stripe's "row above" */
    for (int x = lane; x <= n + 1; x += 64) edge[x] = (int16_t)(LOCAL ? 0 : x * gap);

    int16_t *Hp = a.mat + pr.matOff;
    const size_t cs = pr.chunkStride;
    const int S = dpx_tiled_stripes(m, R);

    int bestv = 0, bestrow = 0, bestcol = 0;
    LinState<R, LOCAL> st;

    if (STORE && S >= 2 && n >= 128) { /* (score-only fills are VALU-bound: the plain striped loop is leaner there) */
        /* ---------- rolling schedule: a lane that finishes column n of its stripe starts column 1 of the next one
         * on the following step, so the skew ramp is paid once per pair instead of once per stripe and every
         * chunk between the two ramps is a whole one. ---------- */
        const unsigned char *ql = stage_bytes(my + a.ldsQryOff, qry, m, lane, 64); /* staged query: the stripe switch must not wait on global memory */
        int row0 = lane * R;
        int nrows = min(max(m - row0, 0), R);
        int jl = 1 - lane; /* this lane's column; <= 0: not started yet */
        int kl = 0;        /* this lane's stripe */
        load_query_rows<R>(st.qc, qry, row0, nrows);
#pragma unroll
        for (int r = 0; r < R; r++) {
            st.Hl[r] = (LOCAL ? 0 : (row0 + 1 + r) * gap) + gap;
            st.key[r] = 0u;
        }
        st.dtop = (LOCAL ? 0 : row0 * gap) + gap;
        int j0 = 1;      /* lane 0's column (wave-uniform): index of its `up` in the edge row */
        bool sw = false; /* this lane wrapped at the end of the previous step */
        int rcN = refl[63 + jl];
        int e0N = edge[1];
        int16_t *tile = Hp + (size_t)lane * (R < 8 ? R : 8);
        const int total = S * n + 63;
        auto roll_step = [&](const int T) {
            const int rc = rcN, e0 = e0N;
            const int jn = (jl >= n) ? 1 : jl + 1;
            rcN = refl[63 + jn];
            j0 = (j0 >= n) ? 1 : j0 + 1;
            e0N = edge[j0]; /* read n-64 steps after lane 63 wrote it, 63 steps before lane 63 overwrites it */
            /* the neighbour's bottom row must be taken BEFORE a switching lane resets its registers */
            const int upin = wave_shr1(st.Hl[R - 1], e0 + gap);
            if (sw) { /* stripe switch (one lane per step for 64 steps around each stripe boundary) */
                if constexpr (LOCAL) {
                    fold_row_keys<R>(st.key, row0, nrows, bestv, bestrow, bestcol);
                }
                row0 += 64 * R;
                nrows = min(max(m - row0, 0), R);
#pragma unroll
                for (int r = 0; r < R; r++) {
                    st.qc[r] = (r < nrows) ? (int)ql[row0 + r] : 0x100;
                    st.Hl[r] = (LOCAL ? 0 : (row0 + 1 + r) * gap) + gap;
                    st.key[r] = 0u;
                }
                st.dtop = (LOCAL ? 0 : row0 * gap) + gap;
            }
            uint32_t w[(R + 1) / 2];
            if (jl >= 1 && kl < S && nrows > 0) {
                int h[R];
                lin_cells_g<R, LOCAL>(st, upin, rc, 0xFFFFu - (unsigned)jl, matchG, mismatchG, gap, h);
                if (lane == 63 && kl + 1 < S) edge[jl] = (int16_t)h[R - 1];
                if constexpr (STORE) {
#pragma unroll
                    for (int q = 0; q < R / 2; q++) w[q] = pack_lo16(h[2 * q], h[2 * q + 1]);
                }
            } else if constexpr (STORE) {
                lin_pack<R, LOCAL>(st, w);
            }
            if constexpr (STORE) { /* whole chunk every step; on the pair's two ramps only the lines with cells (ramp_stores) */
                if (ramp_stores<R>(lane, T, S * n, a.rampLines)) store_words<R>(tile + (size_t)T * cs, w);
            }
            sw = false;
            if (jl >= n) { jl = 1; kl++; sw = kl < S; }
            else jl++;
        };
        int T = 0;
        for (; T + 1 < total; T += 2) { /* two steps per iteration: lets the register allocator ping-pong the H chain */
            roll_step(T);
            roll_step(T + 1);
        }
        if (T < total) roll_step(T);
        if constexpr (LOCAL) fold_row_keys<R>(st.key, row0, nrows, bestv, bestrow, bestcol);
    } else {
        /* ---------- striped schedule (single stripe, or references too short to roll) ---------- */
        const int W = n + 63;
        for (int k = 0; k < S; k++) {
            const int base = k * 64 * R;
            const int row0 = base + lane * R; /* rows above the lane's first row */
            const int nrows = min(max(m - row0, 0), R);
            const bool laneHasRows = nrows > 0;
            const bool hasNext = (k + 1 < S);
            load_query_rows<R>(st.qc, qry, row0, nrows);
#pragma unroll
            for (int r = 0; r < R; r++) {
                st.Hl[r] = (LOCAL ? 0 : (row0 + 1 + r) * gap) + gap; /* column-0 border, LinearNeedlemanWunsch.cpp:31-34 (+ gap: lin_cells_g) */
                st.key[r] = 0u;
            }
            st.dtop = (LOCAL ? 0 : row0 * gap) + gap;
            int16_t *tile = Hp + (size_t)k * (size_t)n * cs + (size_t)lane * (R < 8 ? R : 8);

            /* software pipeline: the LDS reads of step t+1 (reference character of the lane's next column, and
             * lane 0's `up` from the edge row) are issued before the arithmetic of step t */
            const unsigned char *rp = refl + 64 - lane; /* rp[t] = reference character of column j = t - lane + 1 */
            int rcN = rp[0];
            int e0N = edge[1];
#define DPX_LIN_STEP(T_, MASKED_, WHOLE_, HASROWS_)                                                                    \
            {                                                                                                         \
                const int rc = rcN, e0 = e0N;                                                                         \
                rcN = rp[(T_) + 1];                                                                                   \
                e0N = edge[min((T_) + 2, n + 1)];                                                                     \
                lin_step<R, LOCAL, STORE, MASKED_, WHOLE_>(st, (T_), lane, n, HASROWS_, matchG, mismatchG, gap, e0, rc, edge, \
                                                           hasNext, tile + (size_t)(T_) * cs, storeLanes, a.rampLines); \
            }
            const bool fast = (base + 64 * R <= m) && (n >= 64);
            const int storeLanes = (S == 1) ? store_lanes<R>(m) : 64;
            if (S == 1) { /* the ramp chunks belong to this stripe alone: store them whole */
                if (fast) {
                    int t = 0;
                    for (; t < 63; t++) DPX_LIN_STEP(t, true, true, true)
                    for (; t + 1 < n; t += 2) { /* two steps per trip: the left/diagonal registers swap roles instead of moving */
                        DPX_LIN_STEP(t, false, true, true)
                        DPX_LIN_STEP(t + 1, false, true, true)
                    }
                    for (; t < n; t++) DPX_LIN_STEP(t, false, true, true)
                    for (; t < W; t++) DPX_LIN_STEP(t, true, true, true)
                } else {
                    for (int t = 0; t < W; t++) DPX_LIN_STEP(t, true, true, laneHasRows)
                }
            } else { /* several stripes of a short reference share their ramp chunks: masked stores there */
                for (int t = 0; t < W; t++) DPX_LIN_STEP(t, true, false, laneHasRows)
            }
#undef DPX_LIN_STEP
            if constexpr (LOCAL) fold_row_keys<R>(st.key, row0, nrows, bestv, bestrow, bestcol);
        }
    }

    if constexpr (LOCAL) {
        /* first strict maximum in row-major order (c++/LinearSmithWaterman.cpp:145-157):
         * max score, then smallest row; then the smallest column of that row */
        const unsigned long long mine = ((unsigned long long)(unsigned)bestv << 32) | (unsigned)(0x7FFFFFFF - bestrow);
        const unsigned long long top = wave_max_u64(mine);
        if ((int)(top >> 32) == 0) {
            if (lane == 0) { a.score[p] = 0; a.endRow[p] = 0; a.endCol[p] = 0; }
        } else if (mine == top) { /* rows are unique per lane, so exactly one lane matches; it holds the row's first column */
            a.score[p] = bestv;
            a.endRow[p] = bestrow;
            a.endCol[p] = bestcol;
        }
    } else {
        /* score = H[m][n] (LinearNeedlemanWunsch.cpp:176): after the last stripe Hl[] holds column n */
        const int lastBase = (S - 1) * 64 * R;
        const int lm = (m - 1 - lastBase) / R, rm = (m - 1 - lastBase) % R;
        if (lane == lm) {
            int v = st.Hl[0];
#pragma unroll
            for (int r = 1; r < R; r++) v = (r == rm) ? st.Hl[r] : v;
            a.score[p] = v - gap; /* (the state is H + gap) */
            a.endRow[p] = m;
            a.endCol[p] = n;
        }
    }
}

/* =====================================================================================================
 * Lane-packed kernels for short and medium queries (the reference's own dataset shape: reads of 80-150 bases,
 * cuda/LNW V12 on bsw/small): SEVERAL pairs per wave.  A pair of m rows takes ceil(m/R) consecutive lanes (R = 8: 13
 * lanes for a 100-row query), the host packs pairs of similar reference length into the 64 lanes of a wave
 * (dpx_wave_desc: up to 8 slots), so nearly every lane owns rows -- one pair per wave kept 13 (or 25) of 64 lanes
 * busy, round 1's four-per-wave quad kernels 13 of 16.  Lane l of a slot owns rows [l*R, l*R+R) and runs column
 * j = t - l - d + 1 in step t (d = the slot's first lane mod 8, see below); `up` moves with v_mov_b32_dpp wave_shr:1,
 * a slot's first lane takes the row-0 border instead; n, m, pointers are per-lane values, the wave runs
 * max(n + lanes + d) steps and every lane masks itself.
 *
 * Writeback: 8 x 8 tile layout (dpx_layout.h), one whole 128-byte line per (row block, column block), through an LDS
 * transpose.  Per step a lane parks its R new scores -- 16 B per row block -- in its own LDS line (ds_write_b128); a
 * lane's line is complete when its column index reaches a multiple of 8.  With the delay d that happens for the lanes
 * lambda = (t+1) mod 8 of every 8-lane group in step t, whatever slots they belong to: eight lines, read back so that
 * lane x of the wave holds piece x%8 of the line of lane 8*(x/8) + (t+1)%8 (ds_read_b128) and written by ONE
 * global_store_dwordx4 of eight whole lines.  The fill is bound by store INSTRUCTIONS (about 104 cycles per
 * global_store_dwordx4 and CU whether 64 or 48 lanes are active, profiles/README.md), so what counts is that every
 * store instruction carries eight lines of real cells: no skew-ramp padding, rows rounded up to 8 instead of 64/128
 * (round 1's [step][lane][rows] chunks wrote 1.40x the algorithmic bytes on short reads), no idle lanes.
 * Where a line goes (pointer, column-block stride, the owner's skew and last column block) sits in the 16 spare bytes
 * of the owner's LDS line; the reading lanes pick it up one step ahead.  LDS lines are 144 bytes apart and column c
 * of lane lambda's line sits in slot (c + lambda) % 8 -- which is t % 8 for every lane of the wave in step t, the skew
 * cancels: conflict-free for the b128 write groups (8 contiguous lanes, banks 4*lambda + const) and for the b128 read
 * groups of MI355X_MICROARCH.md (4 x 16 lanes).  The store of the lines read in step t is issued in step t+1, behind
 * that step's arithmetic.
 * ===================================================================================================== */

template <int Q, int PLANES>
struct LineStage {
    static constexpr int kBytes = PLANES * Q * 64 * kStageLine; /* per wave */
    static constexpr int kStepElems = PLANES * Q * 512;         /* int16 elements a wave stores per step (dpx_layout.h) */
    u32x4 pend[PLANES * Q];
    int16_t *pendDst = nullptr; /* this lane's 16 bytes of (plane 0, sub-tile 0) in the step's chunk; plane p, sub-tile h: + (p*Q + h)*512 elements */
    int pendN = 0;              /* sub-tiles of the owner lane that hold rows (0: nothing to store) */
    uint32_t route = 0;         /* routing word of the owner whose lines complete in the NEXT step */

    /* routing word of a lane, written once into the 16 spare bytes of its LDS line: skew | n8 << 8 | valid sub-tiles << 28 */
    static __device__ __forceinline__ void set_route(unsigned char *tile, int lane, int skew, int n8, int nValid) {
        *reinterpret_cast<uint32_t *>(tile + lane * kStageLine + 128) = (uint32_t)skew | ((uint32_t)n8 << 8) | ((uint32_t)nValid << 28);
    }
    /* park the lane's 8 rows of sub-tile h, plane p, in slot t % 8 of its line (t = the wave's step) */
    static __device__ __forceinline__ void put(unsigned char *tile, int lane, int p, int h, int t, u32x4 v) {
#if DPX_EXP_QUAD == 2
        if (t == -5)
#endif
        *reinterpret_cast<u32x4 *>(tile + ((p * Q + h) * 64 + lane) * kStageLine + ((t & 7) << 4)) = v;
    }
    /* write out what fetch() read one step ago */
    __device__ __forceinline__ void store() {
#if DPX_EXP_QUAD == 1
        if (pendN == 77) /* never */
#endif
#pragma unroll
        for (int h = 0; h < Q; h++) {
            if (h < pendN) {
#pragma unroll
                for (int p = 0; p < PLANES; p++) stream_store(reinterpret_cast<u32x4 *>(pendDst + ((p * Q + h) << 9)), pend[p * Q + h]);
            }
        }
    }
    __device__ __forceinline__ void fetch_route(const unsigned char *tile, int lane, int tNext) {
        route = *reinterpret_cast<const uint32_t *>(tile + ((lane & ~7) | ((tNext + 1) & 7)) * kStageLine + 128);
    }
    /* step t: read piece lane%8 of the lines that completed in this step (owner = lane (t+1)%8 of this lane's 8-group), valid
     * if the owner's column t + 1 - skew is one of its column-block ends (routing word fetched during the previous step);
     * they go to chunk t of the wave's stream, at this lane's 16 bytes */
    __device__ __forceinline__ void fetch(const unsigned char *tile, int16_t *waveBase, int lane, int t) {
        const int owner = (lane & ~7) | ((t + 1) & 7);
        const int jg = t + 1 - (int)(route & 0xFFu); /* owner's column: a multiple of 8 */
        const int n8 = (int)((route >> 8) & 0xFFFFFu);
        pendN = (jg >= 8 && jg <= n8) ? (int)(route >> 28) : 0;
        pendDst = waveBase + (size_t)t * kStepElems + (lane << 3);
#pragma unroll
        for (int p = 0; p < PLANES; p++)
#pragma unroll
            for (int h = 0; h < Q; h++)
#if DPX_EXP_QUAD == 2
                pend[p * Q + h].x += (uint32_t)owner;
#else
                pend[p * Q + h] = *reinterpret_cast<const u32x4 *>(tile + ((p * Q + h) * 64 + owner) * kStageLine + (((lane + owner) & 7) << 4));
#endif
    }
};

template <int R, bool LOCAL, bool STORE>
__global__ void __launch_bounds__(DPX_FILL_THREADS) k_linear_lanes(const dpx_fill_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int Q = R / 8;
    using Stage = LineStage<Q, 1>;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int w = blockIdx.x * (int)a.wavesPerBlock + wv;
    if (w >= a.numPairs) return; /* wave-uniform; numPairs = number of wave descriptors */
    const LaneSlot sl = find_slot(a.waves + w, lane);
    const bool has = sl.has;
    const int p = sl.p, l = sl.l;
    const dpx_pair_dev pr = a.pairs[p];
    const int n = has ? pr.n : 0, m = has ? pr.m : 0;
    const int gap = a.gapOpen, matchG = a.match - gap, mismatchG = a.mismatch - gap;
    const unsigned char *ref = reinterpret_cast<const unsigned char *>(a.seq + pr.refIdx);
    const unsigned char *qry = reinterpret_cast<const unsigned char *>(a.seq + pr.qryIdx);

    unsigned char *tileL = smem + (size_t)wv * a.ldsPerWave;      /* [line stage | lane scratch][staged references] */
    unsigned char *scratch = tileL;
    unsigned char *refl = tileL + (STORE ? Stage::kBytes : kLaneScratch) + sl.refOff;
    const unsigned char *refs = stage_bytes(refl, ref, n, l, max(sl.num, 1));

    const int row0 = l * R;
    const int nrows = min(max(m - row0, 0), R);
    LinState<R, LOCAL> st; /* Hl = H + gap, dtop = H[row0][j-1] + gap (lin_cells_g) */
    load_query_rows<R>(st.qc, qry, row0, nrows);
#pragma unroll
    for (int r = 0; r < R; r++) {
        st.Hl[r] = (LOCAL ? 0 : (row0 + 1 + r) * gap) + gap;
        st.key[r] = 0u;
    }
    st.dtop = (LOCAL ? 0 : row0 * gap) + gap;

    const int skew = l + sl.d; /* this lane runs column j = t - skew + 1 in step t */
    const int n8 = (n + 7) & ~7;
    const int LB = (int)dpx_tile8_row_blocks(m);
    /* Routing.  A lane's line (8 columns x 8 rows, 128 B) is complete in the steps t = skew + 7, skew + 15, ... <= n8 + skew - 1, and
     * skew = lane (mod 8): in step t the lines of the lanes (t+1) mod 8 of every 8-lane group are complete, whatever pairs they
     * belong to.  Every lane publishes (first step | last step << 16) and the number of its row blocks that hold rows once, in the
     * 16 spare bytes of its LDS line; every lane then keeps the words of the eight lanes of its group in registers -- the loop reads
     * no routing from LDS (round 2 fetched one word per step) and decides with two compares. */
    uint32_t rt[8], nv[8];
    if constexpr (STORE) {
        const int nValid = has ? min(max(LB - l * Q, 0), Q) : 0;
        uint32_t *mine = reinterpret_cast<uint32_t *>(tileL + lane * kStageLine + 128);
        mine[0] = nValid > 0 ? ((uint32_t)(skew + 7) | ((uint32_t)(n8 + skew - 1) << 16)) : 0x00007FFFu; /* (never valid: first > last) */
        mine[1] = (uint32_t)nValid;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint32_t *o = reinterpret_cast<const uint32_t *>(tileL + ((lane & ~7) | k) * kStageLine + 128);
            rt[k] = o[0];
            nv[k] = o[1];
        }
    }
    /* the wave's stream of chunks (dpx_layout.h): every pair of the wave carries the same base; lane 0 always belongs to slot 0 */
    int16_t *waveBase = a.mat + (size_t)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(pr.matOff >> 32)) << 32) |
                                         (unsigned)__builtin_amdgcn_readfirstlane((int)(pr.matOff & 0xFFFFFFFFull)));
    const int steps = __builtin_amdgcn_readfirstlane(wave_max_i32(has ? (STORE ? n8 : n) + skew : 0)); /* uniform: the loop runs on the scalar unit */
    const unsigned char *rp = refs - skew; /* rp[t] = reference character of column j = t - skew + 1 */
    const unsigned nEff = nrows > 0 ? (unsigned)n : 0u; /* the lane is on a cell iff (unsigned)(t - skew) < nEff */
    const int rpLast = n + skew;                        /* rp[rpLast] = refs[n]: inside the 31 bytes of slack of stage_bytes */
    unsigned char *putPtr = tileL + lane * kStageLine;             /* + sub-tile * 64 lines + (t & 7) * 16 */
    const unsigned char *fetchPtr[8];                              /* piece lane % 8 of the line of lane k of this lane's group, rotated by its owner */
#pragma unroll
    for (int k = 0; k < 8; k++) fetchPtr[k] = tileL + ((lane & ~7) | k) * kStageLine + (((lane + k) & 7) << 4);
    u32x4 pend[Q];
    int pendN = 0;
    int16_t *pendDst = nullptr;
    int bordG = (2 - skew) * gap; /* NW, first lane of a slot: H[0][j] + gap = (j + 1) * gap, j = t - skew + 1 */
    int rcN = rp[0];
    auto flush = [&]() __attribute__((always_inline)) { /* write out the lines read one step ago */
#if DPX_EXP_QUAD == 1 /* ablation build (tools/ab_quad.sh): no global stores */
        if (pendN == 77)
#endif
#pragma unroll
        for (int hq = 0; hq < Q; hq++)
            if (hq < pendN) stream_store(reinterpret_cast<u32x4 *>(pendDst + (hq << 9)), pend[hq]);
    };
    auto lane_step = [&](const int t, auto kTag) __attribute__((always_inline)) {
        constexpr int K = decltype(kTag)::value; /* t & 7 */
        const int tms = t - skew;
        const int rc = rcN;
        rcN = rp[min(t + 1, rpLast)]; /* (never past the slot's staged reference: a shorter pair's lane idles to the end of the wave) */
        const int sh = wave_shr1(st.Hl[R - 1], 0);
        const int upinG = (l == 0) ? (LOCAL ? gap : bordG) : sh; /* a slot's first lane: row-0 border of its column (+ gap) */
        if constexpr (!LOCAL) bordG += gap;
        if ((unsigned)tms < nEff) {
            int h[R];
            lin_cells_g<R, LOCAL>(st, upinG, rc, 0xFFFEu - (unsigned)tms, matchG, mismatchG, gap, h);
            if constexpr (STORE) {
#pragma unroll
                for (int hq = 0; hq < Q; hq++) {
                    u32x4 v = {pack_lo16(h[8 * hq + 0], h[8 * hq + 1]), pack_lo16(h[8 * hq + 2], h[8 * hq + 3]),
                               pack_lo16(h[8 * hq + 4], h[8 * hq + 5]), pack_lo16(h[8 * hq + 6], h[8 * hq + 7])};
#if DPX_EXP_QUAD != 2
                    *reinterpret_cast<u32x4 *>(putPtr + hq * 64 * kStageLine + (K << 4)) = v;
#else
                    pend[hq].y += v.x;
#endif
                }
            }
        }
        if constexpr (STORE) {
            flush();
            constexpr int O = (K + 1) & 7; /* the owners of the lines that are complete now */
            const uint32_t r = rt[O];
            const bool valid = (uint32_t)t >= (r & 0xFFFFu) && (uint32_t)t <= (r >> 16);
            pendN = valid ? (int)nv[O] : 0;
#if DPX_EXP_QUAD == 3 /* ablation build: every store instruction full (invalid lines written too): bytes + 50 %, same instruction count */
            pendN = Q;
#endif
            pendDst = waveBase + (size_t)t * Stage::kStepElems + (lane << 3);
#pragma unroll
            for (int hq = 0; hq < Q; hq++)
#if DPX_EXP_QUAD == 2 /* ablation build: stores without the LDS round trip */
                pend[hq].x += (uint32_t)t;
#else
                pend[hq] = *reinterpret_cast<const u32x4 *>(fetchPtr[O] + hq * 64 * kStageLine);
#endif
        }
    };
    {
        int t = 0;
        for (; t + 8 <= steps; t += 8) { /* eight steps per trip: every LDS address of the line stage is a register + an immediate */
            lane_step(t + 0, std::integral_constant<int, 0>{}); lane_step(t + 1, std::integral_constant<int, 1>{});
            lane_step(t + 2, std::integral_constant<int, 2>{}); lane_step(t + 3, std::integral_constant<int, 3>{});
            lane_step(t + 4, std::integral_constant<int, 4>{}); lane_step(t + 5, std::integral_constant<int, 5>{});
            lane_step(t + 6, std::integral_constant<int, 6>{}); lane_step(t + 7, std::integral_constant<int, 7>{});
        }
        if (t + 0 < steps) lane_step(t + 0, std::integral_constant<int, 0>{});
        if (t + 1 < steps) lane_step(t + 1, std::integral_constant<int, 1>{});
        if (t + 2 < steps) lane_step(t + 2, std::integral_constant<int, 2>{});
        if (t + 3 < steps) lane_step(t + 3, std::integral_constant<int, 3>{});
        if (t + 4 < steps) lane_step(t + 4, std::integral_constant<int, 4>{});
        if (t + 5 < steps) lane_step(t + 5, std::integral_constant<int, 5>{});
        if (t + 6 < steps) lane_step(t + 6, std::integral_constant<int, 6>{});
    }
    if constexpr (STORE) flush();
    if constexpr (LOCAL) {
        /* first strict maximum in row-major order over the slot's lanes (rows ascend with the lane): the slot's first lane
         * scans its lanes' (score, row, column) in the lane scratch */
        int bestv = 0, bestrow = 0, bestcol = 0;
        fold_row_keys<R>(st.key, row0, nrows, bestv, bestrow, bestcol);
        int *mine = reinterpret_cast<int *>(scratch + lane * 16);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); /* (the line stage this aliases has been read to the end) */
        __builtin_amdgcn_wave_barrier();
        mine[0] = bestv; mine[1] = bestrow; mine[2] = bestcol;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); /* the other lanes' entries are read below: keep the order */
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (has && l == 0) {
            for (int k = 1; k < sl.num; k++) {
                const int *o = reinterpret_cast<const int *>(scratch + (lane + k) * 16);
                if (o[0] > bestv) { bestv = o[0]; bestrow = o[1]; bestcol = o[2]; }
            }
            a.score[p] = bestv; a.endRow[p] = bestv > 0 ? bestrow : 0; a.endCol[p] = bestv > 0 ? bestcol : 0;
        }
    } else {
        const int lm = (m - 1) / R, rm = (m - 1) % R; /* owner of row m: its registers hold column n after its last step */
        if (has && l == lm) {
            int v = st.Hl[0];
#pragma unroll
            for (int r = 1; r < R; r++) v = (r == rm) ? st.Hl[r] : v;
            a.score[p] = v - gap; a.endRow[p] = m; a.endCol[p] = n; /* (the state is H + gap) */
        }
    }
}

/* =====================================================================================================
 * Split kernel for SMALL batches (BASELINE configs[1]: 1000 pairs of 512 x 512 -- one wave per pair leaves the chip with
 * one wave per SIMD, and a lone wave issues a vector instruction only every 4 cycles).  One workgroup per pair, one WAVE
 * PER STRIPE: wave w fills rows [w*64R, (w+1)*64R) with R = 4 (or 2), all stripes at the same time, wave w+1 running
 * ~90 columns behind wave w and taking its "row above" from the LDS edge row wave w's lane 63 writes -- the stripe
 * hand-off of cuda/LNW/LinearNeedlemanWunschV12.cu:110-113,141-143 (warpEdgeScore), made concurrent.  Progress is
 * published through LDS every 8 columns (release) and checked every 16 (acquire).  1000 pairs become 2000-4000 waves
 * with half (a quarter) of the dependent chain per step.  Stores stay 16 bytes per lane: G = 8/R steps are collected in
 * registers (dpx_layout.h, split layout); every stripe owns its chunks, so ramp chunks are written whole.
 * ===================================================================================================== */
#define DPX_SPLIT_MAX_WAVES 16
template <int R, bool LOCAL>
__global__ void __launch_bounds__(64 * DPX_SPLIT_MAX_WAVES) k_linear_split(const dpx_fill_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int G = 8 / R; /* steps per 16-byte store */
    static_assert(R == 2 || R == 4 || R == 8, "rows per lane");
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int p = blockIdx.x;
    if (a.order) p = a.order[p];
    const dpx_pair_dev pr = a.pairs[p];
    const int n = pr.n, m = pr.m; /* host guarantees m > 0, n > 0 */
    const int gap = a.gapOpen, matchG = a.match - gap, mismatchG = a.mismatch - gap; /* the state is H + gap (lin_cells_g) */
    const int W = dpx_tiled_stripes(m, R);
    const unsigned char *ref = reinterpret_cast<const unsigned char *>(a.seq + pr.refIdx);
    const unsigned char *qry = reinterpret_cast<const unsigned char *>(a.seq + pr.qryIdx);
    /* LDS: [control: progress[16], done, pad | per-wave results 16 x 16 B][staged reference][edge rows, one per stripe boundary] */
    int *ctrl = reinterpret_cast<int *>(smem);
    int *result = ctrl + 32;
    if (threadIdx.x < 32) ctrl[threadIdx.x] = 0;
    const unsigned char *refl = stage_bytes(smem + a.ldsRefOff + 64, ref, n, (int)threadIdx.x, (int)blockDim.x) - 64; /* refl[64 + (j-1)] */
    __syncthreads(); /* every wave of the workgroup is still here; surplus waves leave afterwards */
    if (w >= W) return;
    int16_t *edgeMine = reinterpret_cast<int16_t *>(smem + a.ldsQryOff) + (size_t)w * a.ldsBufStride;       /* bottom row of this stripe */
    const int16_t *edgePrev = edgeMine - a.ldsBufStride;                                                        /* ... of the stripe above */

    const int row0 = w * 64 * R + lane * R;
    const int nrows = min(max(m - row0, 0), R);
    LinState<R, LOCAL> st;
    load_query_rows<R>(st.qc, qry, row0, nrows);
#pragma unroll
    for (int r = 0; r < R; r++) {
        st.Hl[r] = (LOCAL ? 0 : (row0 + 1 + r) * gap) + gap;
        st.key[r] = 0u;
    }
    st.dtop = (LOCAL ? 0 : row0 * gap) + gap;
    const bool hasNext = w + 1 < W;
    const int rowsHere = min(m - w * 64 * R, 64 * R);
    const int storeLanes = min(64, (((rowsHere + R - 1) / R) + 7) & ~7); /* row-owning lanes, rounded up to whole 128-byte lines */
    const uint32_t SS = dpx_split_stripe_steps(n, R); /* n + 63 rounded up to whole 16-step blocks */
    const size_t cs = pr.chunkStride;
    int16_t *tile = a.mat + pr.matOff + ((size_t)w * (SS / G)) * cs + (size_t)lane * 8;
    const unsigned char *rp = refl + 64 - lane; /* rp[t] = reference character of column j = t - lane + 1 */
    auto wait_for = [&](const int need) {       /* wave-uniform: the stripe above has published `need` columns of its bottom row */
        while (__hip_atomic_load(&ctrl[w - 1], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < need) __builtin_amdgcn_s_sleep(1);
    };
    /* lane 63 writes the stripe's bottom row; the other lanes write the same instruction's worth into a 32-byte dump, so the
     * edge write costs one ds_write_b16 per step and no exec juggling */
    int16_t *dump = reinterpret_cast<int16_t *>(smem + 384) + 16 * 0;
    uint32_t acc[4];
    int hv[R]; /* the plain scores of the lane's last column (outside the ramps every lane has one every step) */
#pragma unroll
    for (int r = 0; r < R; r++) hv[r] = st.Hl[r] - gap;
    /* one block of 16 steps; MASKED: the skew ramps, where a lane may be before column 1 or past column n */
    auto block16 = [&](const int tb, auto maskedTag) {
        constexpr bool MASKED = decltype(maskedTag)::value;
        if (w > 0) wait_for(min(tb + 17, n));
        int16_t *ew = (hasNext && lane == 63) ? edgeMine + (tb - 62) : dump; /* ew[g] = edgeMine[j] of step tb + g */
        const unsigned char *rpb = rp + tb;
        const int16_t *epb = edgePrev + tb;
        int rcN = rpb[0];
        int e0N = ((w == 0) ? (LOCAL ? 0 : (tb + 1) * gap) : (int)epb[1]) + gap; /* "up" of lane 0, + gap like every state value */
#pragma unroll
        for (int g = 0; g < 16; g++) {
            const int t = tb + g;
            const int rc = rcN, e0 = e0N;
            rcN = rpb[g + 1];
            e0N = ((w == 0) ? (LOCAL ? 0 : (t + 2) * gap) : (int)epb[g + 2]) + gap; /* (entries past n are never used) */
            const int upin = wave_shr1(st.Hl[R - 1], e0);
            const int j = t - lane + 1;
            const unsigned negj = 0xFFFFu - (unsigned)j;
            if constexpr (MASKED) {
                if (j >= 1 && j <= n) {
                    lin_cells_g<R, LOCAL>(st, upin, rc, negj, matchG, mismatchG, gap, hv);
                    if (hasNext && lane == 63) edgeMine[j] = (int16_t)hv[R - 1];
                }
            } else {
                lin_cells_g<R, LOCAL>(st, upin, rc, negj, matchG, mismatchG, gap, hv);
                ew[g] = (int16_t)hv[R - 1];
            }
            if constexpr (R == 8) {
                acc[0] = pack_lo16(hv[0], hv[1]); acc[1] = pack_lo16(hv[2], hv[3]);
                acc[2] = pack_lo16(hv[4], hv[5]); acc[3] = pack_lo16(hv[6], hv[7]);
            } else if constexpr (R == 4) {
                acc[2 * (g % G)] = pack_lo16(hv[0], hv[1]); acc[2 * (g % G) + 1] = pack_lo16(hv[2], hv[3]);
            } else {
                acc[g % G] = pack_lo16(hv[0], hv[1]);
            }
            if ((g % G) == G - 1 && t - (G - 1) < n + 63) { /* whole lines, also on the skew ramps (see lin_step); nothing past the last step */
                /* (no ramp_stores() here: this kernel runs small batches, which are bound by the latency of a step, not by bytes --
                 * line-rounded ramp masks measured 8 % SLOWER on 1000 x 512 x 512, tools/ab_ramp.sh) */
                const bool doStore = lane < storeLanes;
                if (doStore) {
                    u32x4 v = {acc[0], acc[1], acc[2], acc[3]};
                    stream_store(reinterpret_cast<u32x4 *>(tile + (size_t)(t / G) * cs), v);
                }
            }
            /* publish the bottom row's progress every 8 columns (lane 63 ran column t - 62 in this step) */
            if ((g & 7) == 7 && hasNext && t >= 63) {
                if (lane == 63) __hip_atomic_store(&ctrl[w], min(t - 62, n), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
    };
    {
        int tb = 0;
        const int steps = (int)SS;
        for (; tb < steps && tb < 64; tb += 16) block16(tb, std::true_type{});
        for (; tb + 16 <= n; tb += 16) block16(tb, std::false_type{}); /* every lane inside [1, n] for all 16 steps */
        for (; tb < steps; tb += 16) block16(tb, std::true_type{});
    }
    if (hasNext && lane == 63) __hip_atomic_store(&ctrl[w], n, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);

    /* results: every wave leaves its candidate in LDS; the wave that arrives last combines them */
    int bestv = 0, bestrow = 0, bestcol = 0;
    if constexpr (LOCAL) {
        fold_row_keys<R>(st.key, row0, nrows, bestv, bestrow, bestcol);
        const unsigned long long mine = ((unsigned long long)(unsigned)bestv << 32) | (unsigned)(0x7FFFFFFF - bestrow);
        const unsigned long long top = wave_max_u64(mine);
        if (mine == top && (bestv > 0 ? true : lane == 0)) { result[4 * w] = bestv; result[4 * w + 1] = bestrow; result[4 * w + 2] = bestcol; }
    } else {
        const int lm = (m - 1 - w * 64 * R) / R, rm = (m - 1) % R; /* owner of row m (in the last stripe) */
        if (w == W - 1 && lane == lm) {
            int v = st.Hl[0];
#pragma unroll
            for (int r = 1; r < R; r++) v = (r == rm) ? st.Hl[r] : v;
            a.score[p] = v - gap; a.endRow[p] = m; a.endCol[p] = n; /* (the state is H + gap) */
        }
    }
    if constexpr (LOCAL) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        int arrived = 0;
        if (lane == 0) arrived = __hip_atomic_fetch_add(&ctrl[16], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
        arrived = __builtin_amdgcn_readfirstlane(arrived);
        if (arrived == W - 1 && lane == 0) { /* first strict maximum in row-major order: max score, then the first stripe holding it */
            int bv = 0, br = 0, bc = 0;
            for (int k = 0; k < W; k++) {
                const int v = __hip_atomic_load(&result[4 * k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (v > bv) { bv = v; br = result[4 * k + 1]; bc = result[4 * k + 2]; }
            }
            a.score[p] = bv; a.endRow[p] = bv > 0 ? br : 0; a.endCol[p] = bv > 0 ? bc : 0;
        }
    }
}

/* =====================================================================================================
 * "+Opt": packed two-pairs-per-wave linear fill (the reference's V18/V19 idea, cuda/LNW/LinearNeedlemanWunschV18.cu:
 * 112-341 and the unfinished cuda/LinearSmithWatermanOpt.cu: one warp computes two pairs with __vibmax_s16x2).
 * Every VGPR holds pair A in its high half and pair B in its low half (V19.cu:16-24); the cell update runs on the
 * VOP3P packed-int16 pipe: v_xor (chars), v_pk_min_u16 (0/1 "differs"), v_pk_mad_i16 (s = differs*(mismatch-match)+match),
 * v_pk_max_i16 / v_pk_add_i16.  One DPP move carries both pairs to the next lane.  Both pairs must have the same
 * (m, n); the host couples equal-shaped pairs and sends leftovers to k_linear_fill.  Matrices are written in the
 * same per-pair wavefront-tiled layout, so export and traceback do not care which kernel filled a pair.
 * SW start cell: tracked exactly in the loop, per half: a packed running row maximum and the column at which it was
 * first reached (v_pk_max_u16 / v_pk_sub_u16 / v_pk_min_u16 / v_pk_sub_u16 / v_bfi_b32, see PkState).
 * ===================================================================================================== */
template <int R>
struct PkState {
    uint32_t Hl[R];   /* packed H[row][j-1] */
    uint32_t qc[R];   /* packed query characters (16-bit lanes) */
    uint32_t rmax[R]; /* SW: per-row running maximum of pair A's key (H << 16 | 0xFFFF - column): max score, then smallest column */
    uint32_t rcol[R]; /* SW: the same for pair B */
    uint32_t dtop;
    uint32_t keyA, keyB; /* SW, TAGS: ONE key per pair and lane, (H * R + (R-1 - row in lane)) << 16 | 0xFFFF - column: max score, then
                            smallest row, then smallest column -- the row-major "first strict maximum" of c++/LinearSmithWaterman.cpp:145-157 */
};

/* per half: H * R + tag on the VOP3P pipe (v_pk_mad_u16 with two inline constants: no register for either) */
template <int R, int TAG>
__device__ __forceinline__ uint32_t pk_row_tag(uint32_t h) {
    static_assert(TAG >= 0 && TAG < R && R <= 16, "inline constants");
    uint32_t r;
    asm("v_pk_mad_u16 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(r) : "v"(h), "n"(R), "n"(TAG));
    return r;
}
/* row r of the lane (a constant once the row loop is unrolled: the switch folds away) carries tag R-1 - r */
template <int R>
__device__ __forceinline__ uint32_t pk_row_tag_of(uint32_t h, const int r) {
#define DPX_TAG_CASE(k) case k: if constexpr (k < R) return pk_row_tag<R, (k < R ? R - 1 - k : 0)>(h); else return 0u;
    switch (r) {
        DPX_TAG_CASE(0) DPX_TAG_CASE(1) DPX_TAG_CASE(2) DPX_TAG_CASE(3) DPX_TAG_CASE(4) DPX_TAG_CASE(5) DPX_TAG_CASE(6) DPX_TAG_CASE(7)
        DPX_TAG_CASE(8) DPX_TAG_CASE(9) DPX_TAG_CASE(10) DPX_TAG_CASE(11) DPX_TAG_CASE(12) DPX_TAG_CASE(13) DPX_TAG_CASE(14) DPX_TAG_CASE(15)
    default: return 0u;
    }
#undef DPX_TAG_CASE
}

template <int R>
__device__ __forceinline__ void store_tile_pk(int16_t *dstA, int16_t *dstB, const uint32_t (&v)[R]) {
    /* pair A = high halves, pair B = low halves; R/2 dwords each */
    if constexpr (R == 2) {
        *reinterpret_cast<uint32_t *>(dstA) = pk_hi16(v[0], v[1]);
        *reinterpret_cast<uint32_t *>(dstB) = pack_lo16((int)v[0], (int)v[1]);
    } else if constexpr (R == 4) {
        uint2 a, b;
        a.x = pk_hi16(v[0], v[1]); a.y = pk_hi16(v[2], v[3]);
        b.x = pack_lo16((int)v[0], (int)v[1]); b.y = pack_lo16((int)v[2], (int)v[3]);
        *reinterpret_cast<uint2 *>(dstA) = a;
        *reinterpret_cast<uint2 *>(dstB) = b;
    } else {
#pragma unroll
        for (int q = 0; q < R / 8; q++) {
            uint4 a, b;
            a.x = pk_hi16(v[8 * q + 0], v[8 * q + 1]); a.y = pk_hi16(v[8 * q + 2], v[8 * q + 3]);
            a.z = pk_hi16(v[8 * q + 4], v[8 * q + 5]); a.w = pk_hi16(v[8 * q + 6], v[8 * q + 7]);
            b.x = pack_lo16((int)v[8 * q + 0], (int)v[8 * q + 1]); b.y = pack_lo16((int)v[8 * q + 2], (int)v[8 * q + 3]);
            b.z = pack_lo16((int)v[8 * q + 4], (int)v[8 * q + 5]); b.w = pack_lo16((int)v[8 * q + 6], (int)v[8 * q + 7]);
            *reinterpret_cast<uint4 *>(dstA + q * 512) = a; /* sub-tile q */
            *reinterpret_cast<uint4 *>(dstB + q * 512) = b;
        }
    }
}

template <int R, bool LOCAL, bool MASKED, bool WHOLE, bool TAGS = false, bool PARTIAL = false>
__device__ __forceinline__ void pk_step(PkState<R> &st, const int t, const int lane, const int n, const bool laneHasRows, const int nrows,
                                        const uint32_t matchP, const uint32_t negDeltaP, const uint32_t gapP, const uint32_t e0,
                                        const uint32_t rcP, uint32_t *edge, const bool writeEdge, int16_t *tileA, int16_t *tileB,
                                        const int storeLanes, const int rampLines) {
    const int j = t - lane + 1;
    const uint32_t upin = (uint32_t)wave_shr1((int)st.Hl[R - 1], (int)e0);
    bool active = true;
    if constexpr (MASKED) active = laneHasRows && (j >= 1) && (j <= n);
    if (active) {
        uint32_t u = upin, d = st.dtop;
        const uint32_t onesP = 0x00010001u;
        const uint32_t negj = 0xFFFFu - (uint32_t)j;
        uint32_t colMax = 0u; /* TAGS: per half, max over the lane's rows of this column of (H * R + R-1 - r) */
#pragma unroll
        for (int r = 0; r < R; r++) {
            const uint32_t left = st.Hl[r];
            const uint32_t differs = dpx::pk_min_u16_raw(st.qc[r] ^ rcP, onesP);                 /* 0 / 1 per half */
            const s16x2 sc = as_s16x2(dpx::pk_mad_i16_raw(differs, negDeltaP, matchP));         /* match or mismatch per half */
            s16x2 h;
            if constexpr (LOCAL && TAGS) { /* (rowTags batches have gap <= 0: gapP holds |gap| here) */
                h = dpx::pk_max(pk_gap_sat(u, left, gapP), (s16x2)(as_s16x2(d) + sc));
            } else {
                const s16x2 g = dpx::pk_max(as_s16x2(u), as_s16x2(left)) + as_s16x2(gapP);
                h = dpx::pk_max(g, (s16x2)(as_s16x2(d) + sc));
                if constexpr (LOCAL) h = dpx::pk_max(h, as_s16x2(0u));
            }
            d = left;
            u = as_u32(h);
            st.Hl[r] = u;
            if constexpr (LOCAL && TAGS) {
                /* the lane's rows are consecutive, so "max score, then first row" inside the lane is one packed maximum over
                 * (H * R + R-1 - r): v_pk_mad_u16 + v_pk_max_u16 for both pairs (the host guarantees H * R + R-1 <= 65535) */
                uint32_t tg = pk_row_tag_of<R>(u, r);
                if constexpr (PARTIAL) tg = (r < nrows) ? tg : 0u; /* rows past the query's end hold no cells */
                colMax = r == 0 ? tg : dpx::pk_max_u16_raw(colMax, tg);
            } else if constexpr (LOCAL) {
                /* first strict maximum of the row, per pair: the int32 kernels' (score, column) key, one per half -- v_and_or_b32 /
                 * v_lshl_or_b32 build it, v_max_u32 (v_max3_u32 across two unrolled steps) folds it: 3-4 ops per two cells where the
                 * packed running-maximum + column select of round 1 took 5 */
                st.rmax[r] = max(st.rmax[r], (u & 0xFFFF0000u) | negj);
                st.rcol[r] = max(st.rcol[r], (u << 16) | negj);
            }
        }
        if constexpr (LOCAL && TAGS) { /* ... and the column: once per step and pair, not once per row */
            st.keyA = max(st.keyA, (colMax & 0xFFFF0000u) | negj);
            st.keyB = max(st.keyB, (colMax << 16) | negj);
        }
        st.dtop = upin;
        if (writeEdge && lane == 63) edge[j] = st.Hl[R - 1];
        if constexpr (MASKED && !WHOLE) store_tile_pk<R>(tileA, tileB, st.Hl);
    }
    if constexpr (!MASKED || WHOLE) {
        bool doStore = lane < storeLanes; /* whole lines (see lin_step) */
        if constexpr (MASKED) doStore = doStore && ramp_stores<R>(lane, t, n, rampLines);
        if (doStore) store_tile_pk<R>(tileA, tileB, st.Hl);
    }
}

#ifndef DPX_PK_MIN_BLOCKS
#define DPX_PK_MIN_BLOCKS 1
#endif
template <int R, bool LOCAL, bool TAGS>
__global__ void __launch_bounds__(DPX_FILL_THREADS, DPX_PK_MIN_BLOCKS) k_linear_fill_pk(const dpx_fill_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = blockIdx.x * (int)a.wavesPerBlock + wv; /* couple index */
    if (c >= a.numPairs) return;
    const int pA = a.order[2 * c], pB = a.order[2 * c + 1];
    const dpx_pair_dev prA = a.pairs[pA], prB = a.pairs[pB];
    const int n = prA.n, m = prA.m; /* host guarantees prB.n == n, prB.m == m, both > 0 */
    const unsigned char *refA = reinterpret_cast<const unsigned char *>(a.seq + prA.refIdx);
    const unsigned char *refB = reinterpret_cast<const unsigned char *>(a.seq + prB.refIdx);
    const unsigned char *qryA = reinterpret_cast<const unsigned char *>(a.seq + prA.qryIdx);
    const unsigned char *qryB = reinterpret_cast<const unsigned char *>(a.seq + prB.qryIdx);
    const int gap = a.gapOpen;
    const uint32_t matchP = ((uint32_t)(uint16_t)a.match << 16) | (uint16_t)a.match;
    const uint32_t negDeltaP = ((uint32_t)(uint16_t)(a.mismatch - a.match) << 16) | (uint16_t)(a.mismatch - a.match);
    const int gapK = (LOCAL && TAGS) ? -gap : gap; /* row-tag batches (gap <= 0): the cell update subtracts |gap| with saturation (pk_gap_sat) */
    const uint32_t gapP = ((uint32_t)(uint16_t)gapK << 16) | (uint16_t)gapK;

    unsigned char *my = smem + (size_t)wv * a.ldsPerWave;
    uint32_t *edge = reinterpret_cast<uint32_t *>(my);                    /* packed edge[j], j = 0..n+1 */
    uint16_t *refl = reinterpret_cast<uint16_t *>(my + a.ldsRefOff);      /* refl[64 + (j-1)] = A char << 8 | B char */
    for (int x = 4 * lane; x < n; x += 256) { /* four columns per lane and trip: 2 + 2 aligned dword loads, one 8-byte LDS store */
        const uint32_t a4 = load4(refA + x), b4 = load4(refB + x);
        uint2 w;
        w.x = __builtin_amdgcn_perm(a4, b4, 0x05010400u); /* {B0, A0, B1, A1}: entry j = A char << 8 | B char */
        w.y = __builtin_amdgcn_perm(a4, b4, 0x07030602u);
        *reinterpret_cast<uint2 *>(refl + 64 + x) = w;    /* refl + 64 is 8-byte aligned (ldsRefOff is a multiple of 16) */
    }
    for (int x = lane; x <= n + 1; x += 64) {
        const uint16_t b = (uint16_t)(LOCAL ? 0 : x * gap);
        edge[x] = ((uint32_t)b << 16) | b;
    }
    int16_t *HpA = a.mat + prA.matOff, *HpB = a.mat + prB.matOff;
    const int W = n + 63;
    const int S = dpx_tiled_stripes(m, R);
    int bestA = 0, browA = 0, bcolA = 0, bestB = 0, browB = 0, bcolB = 0;
    PkState<R> st;

    for (int k = 0; k < S; k++) {
        const int base = k * 64 * R;
        const int row0 = base + lane * R;
        const int nrows = min(max(m - row0, 0), R);
        const bool laneHasRows = nrows > 0;
        const bool hasNext = (k + 1 < S);
        int qa[R], qb[R];
        load_query_rows<R>(qa, qryA, row0, nrows);
        load_query_rows<R>(qb, qryB, row0, nrows);
#pragma unroll
        for (int r = 0; r < R; r++) {
            st.qc[r] = ((uint32_t)qa[r] << 16) | (uint32_t)qb[r]; /* rows past the end: 0x0100 in both halves */
            const uint16_t b = (uint16_t)(LOCAL ? 0 : (row0 + 1 + r) * gap);
            st.Hl[r] = ((uint32_t)b << 16) | b;
            st.rmax[r] = 0u;
            st.rcol[r] = 0u;
        }
        st.keyA = st.keyB = 0u;
        { const uint16_t b = (uint16_t)(LOCAL ? 0 : row0 * gap); st.dtop = ((uint32_t)b << 16) | b; }
        const size_t csA = prA.chunkStride, csB = prB.chunkStride;
        int16_t *tileA = HpA + (size_t)k * (size_t)n * csA + (size_t)lane * (R < 8 ? R : 8);
        int16_t *tileB = HpB + (size_t)k * (size_t)n * csB + (size_t)lane * (R < 8 ? R : 8);
        const uint16_t *rp = refl + 64 - lane;
        uint32_t rcN = rp[0];
        uint32_t e0N = edge[1];
#define DPX_PK_STEP(MASKED_, WHOLE_, HASROWS_, PARTIAL_)                                                                        \
        {                                                                                                             \
            const uint32_t rc16 = rcN, e0 = e0N;                                                                      \
            rcN = rp[t + 1];                                                                                          \
            e0N = edge[min(t + 2, n + 1)];                                                                            \
            const uint32_t rcP = __builtin_amdgcn_perm(0u, rc16, 0x0c010c00u); /* {A char, B char} -> 16-bit lanes */  \
            pk_step<R, LOCAL, MASKED_, WHOLE_, TAGS, PARTIAL_>(st, t, lane, n, HASROWS_, nrows, matchP, negDeltaP, gapP, e0, rcP, edge, hasNext, \
                                       tileA + (size_t)t * csA, tileB + (size_t)t * csB, storeLanes, a.rampLines);   \
        }
        const bool fast = (base + 64 * R <= m) && (n >= 64);
        const int storeLanes = (S == 1) ? store_lanes<R>(m) : 64;
        if (S == 1) {
            if (fast) {
                int t = 0;
                for (; t < 63; t++) DPX_PK_STEP(true, true, true, false)
                for (; t + 1 < n;) { DPX_PK_STEP(false, true, true, false) t++; DPX_PK_STEP(false, true, true, false) t++; } /* two steps per trip: the keys of both fold with v_max3_u32 */
                for (; t < n; t++) DPX_PK_STEP(false, true, true, false)
                for (; t < W; t++) DPX_PK_STEP(true, true, true, false)
            } else {
                for (int t = 0; t < W; t++) DPX_PK_STEP(true, true, laneHasRows, true)
            }
        } else if (fast) { /* stripes share their ramp chunks: masked stores on the ramps */
            int t = 0;
            for (; t < 63; t++) DPX_PK_STEP(true, false, true, false)
            for (; t < n; t++) DPX_PK_STEP(false, false, true, false)
            for (; t < W; t++) DPX_PK_STEP(true, false, true, false)
        } else {
            for (int t = 0; t < W; t++) DPX_PK_STEP(true, false, laneHasRows, true)
        }
#undef DPX_PK_STEP
        if constexpr (LOCAL && TAGS) { /* (stripes ascend: a strict '>' keeps the first row holding the maximum) */
            constexpr int TB = R == 16 ? 4 : R == 8 ? 3 : R == 4 ? 2 : 1;
            const int hA = (int)(st.keyA >> (16 + TB)), hB = (int)(st.keyB >> (16 + TB));
            if (hA > bestA) { bestA = hA; browA = row0 + R - (int)((st.keyA >> 16) & (R - 1)); bcolA = 0xFFFF - (int)(st.keyA & 0xFFFFu); }
            if (hB > bestB) { bestB = hB; browB = row0 + R - (int)((st.keyB >> 16) & (R - 1)); bcolB = 0xFFFF - (int)(st.keyB & 0xFFFFu); }
        } else if constexpr (LOCAL) {
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int hA = (int)(st.rmax[r] >> 16), hB = (int)(st.rcol[r] >> 16);
                if (r < nrows && hA > bestA) { bestA = hA; browA = row0 + 1 + r; bcolA = 0xFFFF - (int)(st.rmax[r] & 0xFFFFu); }
                if (r < nrows && hB > bestB) { bestB = hB; browB = row0 + 1 + r; bcolB = 0xFFFF - (int)(st.rcol[r] & 0xFFFFu); }
            }
        }
    }

    if constexpr (LOCAL) {
        /* max score, then first row (c++/LinearSmithWaterman.cpp:145-157) ... */
        const unsigned long long mineA = ((unsigned long long)(unsigned)bestA << 32) | (unsigned)(0x7FFFFFFF - browA);
        const unsigned long long mineB = ((unsigned long long)(unsigned)bestB << 32) | (unsigned)(0x7FFFFFFF - browB);
        const unsigned long long topA = wave_max_u64(mineA), topB = wave_max_u64(mineB);
        /* ... and the lane that owns that row already holds the row's first column */
        if ((int)(topA >> 32) == 0) { if (lane == 0) { a.score[pA] = 0; a.endRow[pA] = 0; a.endCol[pA] = 0; } }
        else if (mineA == topA) { a.score[pA] = bestA; a.endRow[pA] = browA; a.endCol[pA] = bcolA; }
        if ((int)(topB >> 32) == 0) { if (lane == 0) { a.score[pB] = 0; a.endRow[pB] = 0; a.endCol[pB] = 0; } }
        else if (mineB == topB) { a.score[pB] = bestB; a.endRow[pB] = browB; a.endCol[pB] = bcolB; }
    } else {
        const int lastBase = (S - 1) * 64 * R;
        const int lm = (m - 1 - lastBase) / R, rm = (m - 1 - lastBase) % R;
        if (lane == lm) {
            uint32_t v = st.Hl[0];
#pragma unroll
            for (int r = 1; r < R; r++) v = (r == rm) ? st.Hl[r] : v;
            a.score[pA] = (int)(int16_t)(v >> 16); a.endRow[pA] = m; a.endCol[pA] = n;
            a.score[pB] = (int)(int16_t)(v & 0xFFFFu); a.endRow[pB] = m; a.endCol[pB] = n;
        }
    }
}

/* =====================================================================================================
 * Packed lane kernel for short and medium queries (round 3): k_linear_lanes' schedule and tile layout with the packed-int16
 * arithmetic of k_linear_fill_pk -- but the two halves of a register do not hold two PAIRS (which would need equal shapes), they
 * hold two ROW BLOCKS OF THE SAME PAIR: a lane owns 16 consecutive rows, rows 0-7 in the high halves and rows 8-15 in the low
 * halves, and the low half runs ONE COLUMN BEHIND the high half.  A physical lane is two virtual lanes of the wavefront (2l and
 * 2l+1): the low half takes its "row above" from the lane's own high half of the previous step, the high half from the previous
 * lane's low half (one DPP move + one v_perm_b32), the diagonal is last step's "row above" as everywhere.  Any mix of shapes
 * packs as before (a pair of m rows takes ceil(m/16) lanes); the cell update costs 7 (NW) / 8 (SW) VOP3P instructions per TWO
 * cells instead of 5-6 per cell, and the per-step bookkeeping is shared by 16 rows: the int32 kernel needs 117 vector
 * instructions per step and 16 rows (2 x 58.5), this one 80.
 *   - Column 0 of the low half (its first step) needs no mask: its state starts at a large negative value, so that
 *     max(up+gap, left+gap, diag+s) = up+gap = the column-0 border (SW: 0) -- the host checks that the value cannot wrap.
 *   - The high half's extra step at column n+1 (while the low half finishes column n) runs only in lanes that own more than
 *     8 rows; its results are garbage that nothing reads (SW: masked out of the start-cell key).
 *   - SW start cell: one (H * 8 + 7 - r, column) key per half (pk_row_tag); rows past the query's end are not masked -- the host
 *     uses this kernel for SW only if gap <= 0 and mismatch <= 0, where such a row can never exceed the real rows above it.
 *   - Matrices: the SAME tile layout as k_linear_lanes<16> (dpx_layout.h, lanes == 16, rows == 16).  A line's address is a
 *     function of (row block, column block) only; this kernel just completes the lines in another order: the line of lane
 *     lambda, block h, that k_linear_lanes<16> writes to chunk T of the wave's stream is complete here in step T + delta + h
 *     (delta = this schedule's skew minus that one's), so two 8-line stores per step go to per-owner chunks instead of one
 *     contiguous 2 KiB.  Export and traceback do not know which kernel filled a pair.
 * ===================================================================================================== */
template <bool LOCAL>
__global__ void __launch_bounds__(DPX_FILL_THREADS) k_linear_lanes_pk(const dpx_fill_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int kStageBytes = 2 * 64 * kStageLine; /* [block][lane] lines */
    constexpr int kStepElems = 1024;                 /* int16 elements of one chunk of the wave's stream (two 1-KiB halves) */
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int w = blockIdx.x * (int)a.wavesPerBlock + wv;
    if (w >= a.numPairs) return;
    const LaneSlot sl = find_slot(a.waves + w, lane);
    const bool has = sl.has;
    const int p = sl.p, l = sl.l;
    const dpx_pair_dev pr = a.pairs[p];
    const int n = has ? pr.n : 0, m = has ? pr.m : 0;
    const int gap = a.gapOpen;
    const uint32_t matchP = ((uint32_t)(uint16_t)a.match << 16) | (uint16_t)a.match;
    const uint32_t negDeltaP = ((uint32_t)(uint16_t)(a.mismatch - a.match) << 16) | (uint16_t)(a.mismatch - a.match);
    const int gapK = LOCAL ? -gap : gap; /* SW (gap <= 0, checked by the host): |gap| for the saturating gap term (pk_gap_sat) */
    const uint32_t gapP = ((uint32_t)(uint16_t)gapK << 16) | (uint16_t)gapK;
    const unsigned char *ref = reinterpret_cast<const unsigned char *>(a.seq + pr.refIdx);
    const unsigned char *qry = reinterpret_cast<const unsigned char *>(a.seq + pr.qryIdx);

    unsigned char *tileL = smem + (size_t)wv * a.ldsPerWave; /* [line stage][staged references] */
    unsigned char *scratch = tileL;
    unsigned char *refl = tileL + kStageBytes + sl.refOff;
    const unsigned char *refs = stage_bytes(refl, ref, n, l, max(sl.num, 1));

    const int row0 = l * 16;
    const int nrows = min(max(m - row0, 0), 16);
    /* the smallest value that one more weight cannot wrap: "minus infinity" left of column 0 in the low halves */
    const int wmin = min(min(a.match, a.mismatch), min(gap, 0));
    const uint32_t negInf = (uint16_t)(-32768 - wmin);
    uint32_t Hl[8], qc[8], dtop, keyHi = 0u, keyLo = 0u;
    {
        int qa[16];
        load_query_rows<16>(qa, qry, row0, nrows);
#pragma unroll
        for (int r = 0; r < 8; r++) {
            qc[r] = ((uint32_t)qa[r] << 16) | (uint32_t)qa[8 + r]; /* rows past the end: 0x0100, matches no byte */
            const uint16_t b = (uint16_t)(LOCAL ? 0 : (row0 + 1 + r) * gap);
            Hl[r] = ((uint32_t)b << 16) | negInf; /* high half: column 0 of its rows; low half: not started */
        }
        const uint16_t b = (uint16_t)(LOCAL ? 0 : row0 * gap);
        dtop = ((uint32_t)b << 16) | negInf;
    }
    const int first = lane - l;
    const int dOld = first & 7, dNew = (2 * first) & 7;
    const int skew = 2 * l + dNew; /* the HIGH half runs column j = t - skew + 1 in step t, the low half column j - 1 */
    const int n8 = (n + 7) & ~7;
    const int LB = (int)dpx_tile8_row_blocks(m);
    const int nBlocks = has ? min(max(LB - 2 * l, 0), 2) : 0; /* row blocks of this lane that hold rows */
    /* routing, once: [first | last << 16] completing step of the high block, the same of the low block (one step later), and
     * delta = how many steps later than in k_linear_lanes<16>'s schedule this lane's lines are complete */
    {
        uint32_t *mine = reinterpret_cast<uint32_t *>(tileL + lane * kStageLine + 128);
        mine[0] = nBlocks >= 1 ? ((uint32_t)(skew + 7) | ((uint32_t)(n8 + skew - 1) << 16)) : 0x00007FFFu; /* (never valid: first > last) */
        mine[1] = nBlocks >= 2 ? ((uint32_t)(skew + 8) | ((uint32_t)(n8 + skew) << 16)) : 0x00007FFFu;
        mine[2] = (uint32_t)(skew - (l + dOld));
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    uint32_t rtHi[8], rtLo[8];
    int dl[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint32_t *o = reinterpret_cast<const uint32_t *>(tileL + ((lane & ~7) | k) * kStageLine + 128);
        rtHi[k] = o[0]; rtLo[k] = o[1]; dl[k] = (int)o[2];
    }
    int16_t *waveBase = a.mat + (size_t)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(pr.matOff >> 32)) << 32) |
                                         (unsigned)__builtin_amdgcn_readfirstlane((int)(pr.matOff & 0xFFFFFFFFull)));
    const int lastStep = has ? (nBlocks >= 2 ? n8 + skew : n8 + skew - 1) : -1; /* the step in which this lane's last line is complete */
    const int steps = __builtin_amdgcn_readfirstlane(wave_max_i32(lastStep)) + 1;
    const unsigned char *rp = refs - skew; /* rp[t] = reference character of the high half's column */
    const unsigned nEff = nrows > 8 ? (unsigned)n + 1u : (nrows > 0 ? (unsigned)n : 0u); /* on a cell iff (unsigned)(t - skew) < nEff */
    const int rpLast = n + skew; /* rp[rpLast] = refs[n]: inside the slack of stage_bytes (never read past the slot's staged reference) */
    unsigned char *putPtr = tileL + lane * kStageLine;
    const unsigned char *fetchPtr[8]; /* piece lane % 8 of the high-block line of lane k of this lane's group (low block: + 64 lines) */
#pragma unroll
    for (int k = 0; k < 8; k++) fetchPtr[k] = tileL + ((lane & ~7) | k) * kStageLine + (((lane + 2 * k) & 7) << 4);
    const int laneElems = ((lane >> 3) << 6) + ((lane & 7) << 3); /* this lane's 16 bytes inside a 1-KiB half chunk */
    u32x4 pendA, pendB;
    bool okA = false, okB = false;
    int16_t *dstA = nullptr, *dstB = nullptr;
    uint32_t bord = (uint16_t)(-skew * gap); /* NW, first lane of a slot: H[0][j] of the high half's column, j = t - skew + 1 (16 bits; + gap before use) */
    uint32_t rcCur = rp[0], rcPrev = 0u;
    auto flush = [&]() __attribute__((always_inline)) {
        if (okA) stream_store(reinterpret_cast<u32x4 *>(dstA), pendA);
        if (okB) stream_store(reinterpret_cast<u32x4 *>(dstB), pendB);
    };
    auto lane_step = [&](const int t, auto kTag) __attribute__((always_inline)) {
        constexpr int K = decltype(kTag)::value; /* t & 7 */
        const int tms = t - skew;
        const uint32_t rcP = (rcCur << 16) | rcPrev; /* {character of column j, of column j-1} */
        rcPrev = rcCur;
        rcCur = rp[min(t + 1, rpLast)];
        const uint32_t sh = (uint32_t)wave_shr1((int)Hl[7], 0);
        uint32_t upin = __builtin_amdgcn_perm(sh, Hl[7], 0x05040302u); /* {previous lane's low half, this lane's high half} */
        if constexpr (!LOCAL) bord = (uint32_t)(uint16_t)(bord + (uint32_t)gap);
        if (l == 0) upin = (LOCAL ? 0u : (bord << 16)) | (upin & 0xFFFFu); /* a slot's first lane: the row-0 border */
        if ((unsigned)tms < nEff) {
            uint32_t u = upin, colMax = 0u;
            const uint32_t onesP = 0x00010001u;
            uint32_t dsum[8]; /* diagonal terms first, then every row in place (no register rotation across the masked region, see lin_cells) */
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const uint32_t differs = dpx::pk_min_u16_raw(qc[r] ^ rcP, onesP);
                const uint32_t sc = dpx::pk_mad_i16_raw(differs, negDeltaP, matchP);
                dsum[r] = as_u32((s16x2)(as_s16x2(r == 0 ? dtop : Hl[r - 1]) + as_s16x2(sc)));
            }
#pragma unroll
            for (int r = 0; r < 8; r++) {
                s16x2 h;
                if constexpr (LOCAL) h = dpx::pk_max(pk_gap_sat(u, Hl[r], gapP), as_s16x2(dsum[r])); /* gap <= 0 (host): gapP = |gap|, no max(H, 0) needed */
                else h = dpx::pk_max(dpx::pk_max(as_s16x2(u), as_s16x2(Hl[r])) + as_s16x2(gapP), as_s16x2(dsum[r]));
                u = as_u32(h);
                Hl[r] = u;
                if constexpr (LOCAL) {
                    const uint32_t tg = pk_row_tag_of<8>(u, r);
                    colMax = r == 0 ? tg : dpx::pk_max_u16_raw(colMax, tg);
                }
            }
            dtop = upin;
            if constexpr (LOCAL) {
                const uint32_t negj = 0xFFFEu - (uint32_t)tms;                 /* 0xFFFF - j of the high half */
                if (tms < n) keyHi = max(keyHi, (colMax & 0xFFFF0000u) | negj); /* (column n+1 does not exist) */
                keyLo = max(keyLo, (colMax << 16) | (negj + 1u));              /* the low half is on column j - 1 (column 0 scores 0) */
            }
            /* park both blocks' 16 bytes in their lines: the high block's column in slot t % 8, the low block's in slot (t-1) % 8 */
            u32x4 vh = {pk_hi16(Hl[0], Hl[1]), pk_hi16(Hl[2], Hl[3]), pk_hi16(Hl[4], Hl[5]), pk_hi16(Hl[6], Hl[7])};
            u32x4 vl = {pack_lo16((int)Hl[0], (int)Hl[1]), pack_lo16((int)Hl[2], (int)Hl[3]), pack_lo16((int)Hl[4], (int)Hl[5]), pack_lo16((int)Hl[6], (int)Hl[7])};
            *reinterpret_cast<u32x4 *>(putPtr + (K << 4)) = vh;
            *reinterpret_cast<u32x4 *>(putPtr + 64 * kStageLine + (((K + 7) & 7) << 4)) = vl;
        }
        flush();
        /* lines that are complete now: odd steps the HIGH blocks of the lanes (t+1)/2 mod 4 (and + 4) of every group, even steps the
         * LOW blocks of the lanes t/2 mod 4 (and + 4) */
        constexpr int H = (K & 1) ? 0 : 1;
        constexpr int OA = (K & 1) ? (((K + 1) >> 1) & 3) : (K >> 1), OB = OA + 4;
        const uint32_t ra = H ? rtLo[OA] : rtHi[OA], rb = H ? rtLo[OB] : rtHi[OB];
        okA = (uint32_t)t >= (ra & 0xFFFFu) && (uint32_t)t <= (ra >> 16);
        okB = (uint32_t)t >= (rb & 0xFFFFu) && (uint32_t)t <= (rb >> 16);
        dstA = waveBase + (ptrdiff_t)(t - dl[OA] - H) * kStepElems + (H * 512 + laneElems);
        dstB = waveBase + (ptrdiff_t)(t - dl[OB] - H) * kStepElems + (H * 512 + laneElems);
        pendA = *reinterpret_cast<const u32x4 *>(fetchPtr[OA] + H * 64 * kStageLine);
        pendB = *reinterpret_cast<const u32x4 *>(fetchPtr[OB] + H * 64 * kStageLine);
    };
    {
        int t = 0;
        for (; t + 8 <= steps; t += 8) {
            lane_step(t + 0, std::integral_constant<int, 0>{}); lane_step(t + 1, std::integral_constant<int, 1>{});
            lane_step(t + 2, std::integral_constant<int, 2>{}); lane_step(t + 3, std::integral_constant<int, 3>{});
            lane_step(t + 4, std::integral_constant<int, 4>{}); lane_step(t + 5, std::integral_constant<int, 5>{});
            lane_step(t + 6, std::integral_constant<int, 6>{}); lane_step(t + 7, std::integral_constant<int, 7>{});
        }
        if (t + 0 < steps) lane_step(t + 0, std::integral_constant<int, 0>{});
        if (t + 1 < steps) lane_step(t + 1, std::integral_constant<int, 1>{});
        if (t + 2 < steps) lane_step(t + 2, std::integral_constant<int, 2>{});
        if (t + 3 < steps) lane_step(t + 3, std::integral_constant<int, 3>{});
        if (t + 4 < steps) lane_step(t + 4, std::integral_constant<int, 4>{});
        if (t + 5 < steps) lane_step(t + 5, std::integral_constant<int, 5>{});
        if (t + 6 < steps) lane_step(t + 6, std::integral_constant<int, 6>{});
    }
    flush();
    if constexpr (LOCAL) {
        /* the lane's candidate: the high block's rows come first in row-major order, so the low block must be strictly better */
        int bestv = (int)(keyHi >> 19), bestrow = row0 + 8 - (int)((keyHi >> 16) & 7), bestcol = 0xFFFF - (int)(keyHi & 0xFFFFu);
        const int vLo = (int)(keyLo >> 19);
        if (vLo > bestv) { bestv = vLo; bestrow = row0 + 16 - (int)((keyLo >> 16) & 7); bestcol = 0xFFFF - (int)(keyLo & 0xFFFFu); }
        int *mine = reinterpret_cast<int *>(scratch + lane * 16);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); /* (the line stage this aliases has been read to the end) */
        __builtin_amdgcn_wave_barrier();
        mine[0] = bestv; mine[1] = bestrow; mine[2] = bestcol;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (has && l == 0) {
            for (int k = 1; k < sl.num; k++) {
                const int *o = reinterpret_cast<const int *>(scratch + (lane + k) * 16);
                if (o[0] > bestv) { bestv = o[0]; bestrow = o[1]; bestcol = o[2]; }
            }
            a.score[p] = bestv; a.endRow[p] = bestv > 0 ? bestrow : 0; a.endCol[p] = bestv > 0 ? bestcol : 0;
        }
    } else {
        const int lm = (m - 1) / 16, rr = (m - 1) % 16; /* owner of row m: its registers hold column n after its last step */
        if (has && l == lm) {
            uint32_t v = Hl[0];
#pragma unroll
            for (int r = 1; r < 8; r++) v = (r == (rr & 7)) ? Hl[r] : v;
            a.score[p] = (rr < 8) ? (int)(int16_t)(v >> 16) : (int)(int16_t)(v & 0xFFFFu);
            a.endRow[p] = m; a.endCol[p] = n;
        }
    }
}

} // namespace

/* ---- host-callable launchers (used by dpx_capi.cpp); dpx_device.hpp has launch_fill, launch_lds and the dispatchers ---- */

hipError_t dpx_launch_fill(const dpx_fill_args &a, int algo, int R, bool store, size_t ldsBytes, hipStream_t stream) {
    if (a.numPairs <= 0) return hipSuccess;
    if (algo == DPX_K_BSW) return dpx_launch_bsw_fill(a, R, store, ldsBytes, stream); /* here R carries the cells-per-lane count C = dpx_band_cpl(band) */
    if (algo == DPX_K_ANW || algo == DPX_K_ASW || algo == DPX_K_ASG) return dpx_launch_affine_fill(a, algo, R, store, ldsBytes, stream);
    if (algo != DPX_K_LNW && algo != DPX_K_LSW) return hipErrorInvalidValue;
    return dispatch_int<2, 4, 8, 16>(R, [&](auto r) {
        return dispatch_bool(algo == DPX_K_LSW, [&](auto local) {
            return dispatch_bool(store, [&](auto st) {
                return launch_fill(k_linear_fill<decltype(r)::value, decltype(local)::value, decltype(st)::value>, a, a, ldsBytes, stream);
            });
        });
    });
}

/* lane-packed kernels (short / medium queries): a.waves = one descriptor per wave, a.numPairs = number of waves.
 * ldsBytes is per workgroup: (dpx_lanes_stage_bytes() + reference area) x waves per workgroup (4 for the linear kernels,
 * 1 for the affine one). */
hipError_t dpx_launch_fill_lanes(const dpx_fill_args &a, int algo, int R, bool store, size_t ldsBytes, hipStream_t stream) {
    if (a.numPairs <= 0) return hipSuccess;
    if (algo == DPX_K_ANW || algo == DPX_K_ASW || algo == DPX_K_ASG) return dpx_launch_affine_lanes(a, algo, R, store, ldsBytes, stream);
    const int wpb = (int)a.wavesPerBlock;
    const dim3 grid((unsigned)((a.numPairs + wpb - 1) / wpb));
    return dispatch_int<8, 16>(R, [&](auto r) {
        return dispatch_bool(algo == DPX_K_LSW, [&](auto local) {
            return dispatch_bool(store, [&](auto st) {
                return launch_lds(k_linear_lanes<decltype(r)::value, decltype(local)::value, decltype(st)::value>, grid, dim3(64 * wpb), ldsBytes, stream, a);
            });
        });
    });
}

/* packed lane kernel (16 rows per lane, two row blocks of one pair in the two halves): a.waves / a.numPairs as dpx_launch_fill_lanes */
hipError_t dpx_launch_fill_lanes_packed(const dpx_fill_args &a, int algo, size_t ldsBytes, hipStream_t stream) {
    if (a.numPairs <= 0) return hipSuccess;
    const int wpb = (int)a.wavesPerBlock;
    const dim3 grid((unsigned)((a.numPairs + wpb - 1) / wpb));
    return dispatch_bool(algo == DPX_K_LSW, [&](auto local) {
        return launch_lds(k_linear_lanes_pk<decltype(local)::value>, grid, dim3(64 * wpb), ldsBytes, stream, a);
    });
}

/* split kernel (small batches): one workgroup of `waves` waves per pair, a.numPairs workgroups */
hipError_t dpx_launch_fill_split(const dpx_fill_args &a, int algo, int R, int waves, size_t ldsBytes, hipStream_t stream) {
    if (a.numPairs <= 0) return hipSuccess;
    if (waves < 1 || waves > DPX_SPLIT_MAX_WAVES) return hipErrorInvalidValue;
    return dispatch_int<2, 4>(R, [&](auto r) { /* (8 rows per lane would spill under the 1024-thread launch bound) */
        return dispatch_bool(algo == DPX_K_LSW, [&](auto local) {
            return launch_lds(k_linear_split<decltype(r)::value, decltype(local)::value>, dim3((unsigned)a.numPairs), dim3(64 * waves), ldsBytes, stream, a);
        });
    });
}

/* packed two-pairs-per-wave linear fill: a.order = couples (2 ints each), a.numPairs = number of couples */
hipError_t dpx_launch_fill_packed(const dpx_fill_args &a, int algo, int R, size_t ldsBytes, hipStream_t stream) {
    if (a.numPairs <= 0) return hipSuccess;
    return dispatch_int<2, 4, 8, 16>(R, [&](auto r) {
        constexpr int kR = decltype(r)::value;
        if (algo != DPX_K_LSW) return launch_fill(k_linear_fill_pk<kR, false, false>, a, a, ldsBytes, stream);
        return a.rowTags ? launch_fill(k_linear_fill_pk<kR, true, true>, a, a, ldsBytes, stream)
                         : launch_fill(k_linear_fill_pk<kR, true, false>, a, a, ldsBytes, stream);
    });
}

