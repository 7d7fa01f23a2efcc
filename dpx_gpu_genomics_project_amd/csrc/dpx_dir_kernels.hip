/*
 * dpx_dir_kernels.hip -- fill, traceback and export of direction-matrix batches (DPX_KEEP_DIRECTIONS, layout in dpx_dir.h).
 *
 * The reference's evolved kernels keep no score matrix: from cuda/LNW/LinearNeedlemanWunschV6.cu on they write one direction per
 * cell and the score, and the host back-trackers read exactly that (c++/backtrack.h).  Here a batch of that kind stores one 4-bit
 * code per cell and computes in int32, so pairs whose scores do not fit int16 run too, with a quarter of the matrix bytes of an
 * int16 H batch (a twelfth of ANW's H, I and D).
 *
 * Fill: one 64-lane wave per pair on k_linear_fill's striped schedule (lane l owns R rows of a 64*R-row stripe, one column of skew
 * per lane, `up` of the top row through one DPP wave_shr:1, the stripe's bottom row to an int32 edge row for the next stripe).  The
 * codes follow the reference's tie order exactly: LNW (c++/LinearNeedlemanWunsch.cpp:105-128) and ANW's H (AffineNeedlemanWunsch.cpp:
 * 216-236) take the diagonal, then `up` on up >= diagonal, then `left` on left >= max(up, diagonal) -- the __vibmax predicates; LSW
 * (LinearSmithWaterman.cpp:100-109) records none when the best candidate is negative, else up, then left, then the diagonal on
 * equality with H; ANW's gap cells open when the open term is >= the extension (:185-213).  The reference bytes and the edge rows
 * live in LDS, or -- references too long for it -- in a per-wave area of the batch's own allocation (GLOBAL).
 * No MFMA, no atomics.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "dpx_device.hpp"
#include "dpx_dir.h"
#include "dpx_dir_dev.hpp"
#include "dpx_prims.hpp"

namespace {

using dpx::wave_shr1;
using dpx_dir_dev::dir_put;
using dpx_dir_dev::dir_store;
using dpx_dev::stage_bytes;
using dpx_dev::u32x4;
using dpx_dev::wave_max_u64;
using dpx_table::table_stage_rows;

/* =====================================================================================================
 * LNW (LOCAL = false) / LSW (LOCAL = true).
 * ===================================================================================================== */
template <int R, bool LOCAL, bool GLOBAL>
__global__ void __launch_bounds__(DPX_FILL_THREADS) k_linear_dir(const dpx_dir_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int G = 32 / R;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int slot = blockIdx.x * (int)a.wavesPerBlock + wv; /* in this launch (the scratch area's index) */
    if (a.firstSlot + slot >= a.numPairs) return;
    const int p = a.order ? a.order[a.firstSlot + slot] : a.firstSlot + slot;
    const dpx_pair_dev pr = a.pairs[p];
    const int n = pr.n, m = pr.m;
    const int gap = a.gapOpen, match = a.match, mismatch = a.mismatch;

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
    unsigned char *my;
    if constexpr (GLOBAL) my = a.scratch + (size_t)slot * a.ldsPerWave;
    else my = smem + (size_t)wv * a.ldsPerWave;
    int32_t *edge = reinterpret_cast<int32_t *>(my); /* edge[j], j = 0..n+1: H of the row above the current stripe */
    const unsigned char *refl = stage_bytes(my + a.ldsRefOff + 64, ref, n, lane, 64) - 64; /* refl[64 + (j-1)] */
    for (int x = lane; x <= n + 1; x += 64) edge[x] = LOCAL ? 0 : x * gap; /* row-0 border (LinearNeedlemanWunsch.cpp:38-41) */
    if constexpr (GLOBAL) __threadfence_block();

    const int S = dpx_tiled_stripes(m, R);
    const int Wp = (int)dpx_dir_stripe_steps(n, R);
    const size_t cs = (size_t)pr.chunkStride * 2u;
    unsigned char *cbase = a.codes + (size_t)pr.matOff * 2u + (size_t)lane * 16u;

    int bestv = 0, bestrow = 0, bestcol = 0;
    int Hl[R], qc[R], bv[R], bc[R];
    for (int k = 0; k < S; k++) {
        const int row0 = k * 64 * R + lane * R;
        const int nrows = min(max(m - row0, 0), R);
        const bool hasRows = nrows > 0, hasNext = k + 1 < S;
#pragma unroll
        for (int r = 0; r < R; r++) {
            qc[r] = r < nrows ? (int)qry[row0 + r] : 0x100;
            Hl[r] = LOCAL ? 0 : (row0 + 1 + r) * gap; /* column-0 border */
            bv[r] = 0;
            bc[r] = 0;
        }
        int dtop = LOCAL ? 0 : row0 * gap;
        const unsigned char *rp = refl + 64 - lane; /* rp[t] = reference character of column t - lane + 1 */
        int rcN = rp[0];
        int e0N = edge[1];
        unsigned char *dst = cbase + (size_t)k * (size_t)(Wp / G) * cs;
        for (int t0 = 0; t0 < Wp; t0 += G) {
            uint32_t acc[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int q = 0; q < G; q++) {
                const int t = t0 + q;
                const int rc = rcN, e0 = e0N;
                rcN = rp[t + 1];
                e0N = edge[min(t + 2, n + 1)];
                const int upin = wave_shr1(Hl[R - 1], e0); /* all lanes: a finished lane still feeds its neighbour */
                const int j = t - lane + 1;
                uint32_t w[2] = {0u, 0u};
                if (hasRows && j >= 1 && j <= n) {
                    int u = upin, d = dtop;
#pragma unroll
                    for (int r = 0; r < R; r++) {
                        const int s = (qc[r] == rc) ? match : mismatch;
                        const int corner = d + s, up = u + gap, left = Hl[r] + gap;
                        int h;
                        uint32_t code;
                        if constexpr (LOCAL) { /* LinearSmithWaterman.cpp:100-109 */
                            const int tb = max(max(up, left), corner);
                            h = max(tb, 0);
                            code = tb < 0 ? 0u : (up == tb ? 2u : (left == tb ? 3u : 1u));
                            code |= (h == 0) ? 4u : 0u;
                            if (h > bv[r]) { bv[r] = h; bc[r] = j; } /* first strict maximum of the row */
                        } else { /* LinearNeedlemanWunsch.cpp:105-128: __vibmax(del, mm), then __vibmax(ins, .) */
                            const int v = max(up, corner);
                            h = max(left, v);
                            code = left >= v ? 3u : (up >= corner ? 2u : 1u);
                        }
                        w[(r * 4) >> 5] |= code << ((r * 4) & 31);
                        d = Hl[r];
                        u = h;
                        Hl[r] = h;
                    }
                    dtop = upin;
                    if (hasNext && lane == 63) edge[j] = Hl[R - 1];
                }
                dir_put<R>(acc, q, w[0], w[1]);
            }
            dir_store(dst + (size_t)(t0 / G) * cs, acc); /* every lane, ramps included: whole KiB per store */
        }
        if constexpr (GLOBAL) __threadfence_block(); /* the next stripe's lane 0 reads what lane 63 wrote */
        if constexpr (LOCAL) {
#pragma unroll
            for (int r = 0; r < R; r++)
                if (r < nrows && bv[r] > bestv) { bestv = bv[r]; bestrow = row0 + 1 + r; bestcol = bc[r]; }
        }
    }

    if constexpr (LOCAL) {
        /* first strict maximum in row-major order (LinearSmithWaterman.cpp:145-157): max score, then smallest row; a row's first
         * column is what its lane kept */
        const unsigned long long mine = ((unsigned long long)(unsigned)bestv << 32) | (unsigned)(0x7FFFFFFF - bestrow);
        const unsigned long long top = wave_max_u64(mine);
        if ((int)(top >> 32) == 0) {
            if (lane == 0) { a.score[p] = 0; a.endRow[p] = 0; a.endCol[p] = 0; }
        } else if (mine == top) {
            a.score[p] = bestv;
            a.endRow[p] = bestrow;
            a.endCol[p] = bestcol;
        }
    } else {
        const int lastBase = (S - 1) * 64 * R;
        const int lm = (m - 1 - lastBase) / R, rm = (m - 1 - lastBase) % R;
        if (lane == lm) {
            int v = Hl[0];
#pragma unroll
            for (int r = 1; r < R; r++) v = (r == rm) ? Hl[r] : v;
            a.score[p] = v; /* H[m][n] (LinearNeedlemanWunsch.cpp:176) */
            a.endRow[p] = m;
            a.endCol[p] = n;
        }
    }
}

/* =====================================================================================================
 * ANW (Gotoh, AffineNeedlemanWunsch.cpp:167-240): three int32 chains, one code per cell (H move, I / D extension bits).
 * Virtual borders D[0][j] = I[i][0] = DPX_NEG give the reference's i == 1 / j == 1 cases ("open").
 * ===================================================================================================== */
template <int R, bool GLOBAL>
__global__ void __launch_bounds__(DPX_FILL_THREADS) k_affine_dir(const dpx_dir_args a) {
    constexpr bool LOCAL = false, SEMI = false, TABLE = false;
    constexpr dpx_table_ref tref = {nullptr, nullptr};
#include "dpx_affine_dir.inc"
}

/* ASW (affine-gap Smith-Waterman, include/dpx_align.h): the same fill with the zero floor; code move 0 where H == 0, bits 2 / 3 as ANW */
template <int R, bool GLOBAL>
__global__ void __launch_bounds__(DPX_FILL_THREADS) k_asw_dir(const dpx_dir_args a) {
    constexpr bool LOCAL = true, SEMI = false, TABLE = false;
    constexpr dpx_table_ref tref = {nullptr, nullptr};
#include "dpx_affine_dir.inc"
}

/* ASG (affine-gap semi-global alignment, include/dpx_align.h): ANW's fill and codes under a zero row-0 border; the end cell is the first
 * maximum of row m, its column-0 border included */
template <int R, bool GLOBAL>
__global__ void __launch_bounds__(DPX_FILL_THREADS) k_asg_dir(const dpx_dir_args a) {
    constexpr bool LOCAL = false, SEMI = true, TABLE = false;
    constexpr dpx_table_ref tref = {nullptr, nullptr};
#include "dpx_affine_dir.inc"
}

/* ---- the walk over the codes: one WAVE per pair, runs of path steps decided by all 64 lanes at once ----
 * Which way the path leaves a cell is in that cell's code alone, so in every trip lane l fetches the code of the l-th cell of the three lines
 * the path can follow from the walker's cell (i, j) -- the diagonal (i-l, j-l), the column (i-l, j), the row (i, j-l) -- and the two bases
 * of its diagonal cell, all independent loads: one memory round trip per trip.  A ballot then gives how many steps the path really follows
 * the line the walker's own code picks (LNW: left / up / diagonal, borders included; LSW: until a cell with H = 0 or a border; ANW: the
 * SCORING state's choice, and in the two gap states the run of "extends" bits, c++/backtrack.cpp:214-356), and the lanes of that run
 * write their own three characters.  Alignments worth computing are mostly long diagonal runs: ~1 trip per 64 diagonal steps or per gap. */
__device__ __forceinline__ int dir_code(const unsigned char *base, const uint64_t cs, const int n, const int R, const int i, const int j) {
    int sh;
    const uint64_t off = dpx_dir_byte(i, j, n, R, cs, &sh);
    return (base[off] >> sh) & 0xF;
}

__device__ __forceinline__ int dir_run(const bool cont) { /* leading lanes (from lane 0) whose condition holds */
    const unsigned long long mask = __ballot(cont);
    return ~mask == 0ull ? 64 : __builtin_ctzll(~mask);
}

__global__ void __launch_bounds__(64) k_traceback_dir(const dpx_dir_args a, int numPairs, int algo, int R, const uint64_t *tbOff, char *tb,
                                                      int32_t *tbLen) {
    const int p = blockIdx.x, lane = threadIdx.x;
    if (p >= numPairs) return;
    const dpx_pair_dev pr = a.pairs[p];
    const int n = pr.n, m = pr.m;
    const int cap = (m + n + 1 + 3) & ~3;
    char *lr = tb + tbOff[p], *lx = lr + cap, *lq = lx + cap;
    const unsigned char *qry = reinterpret_cast<const unsigned char *>(a.seq + pr.qryIdx);
    const unsigned char *ref = reinterpret_cast<const unsigned char *>(a.seq + pr.refIdx);
    const unsigned char *base = a.codes + (size_t)pr.matOff * 2u;
    const uint64_t cs = (uint64_t)pr.chunkStride * 2u;
    int pos = cap; /* lines grow from the back; the character of run step l goes to pos - 1 - l */
    int i = a.endRow[p], j = a.endCol[p];
    auto put = [&](const int at, const int rc, const int xc, const int qc) { lr[at] = (char)rc; lx[at] = (char)xc; lq[at] = (char)qc; };
    auto tail_up = [&](const int cnt) { /* cnt column-0 / remaining steps up from row i */
        for (int x = lane; x < cnt; x += 64) put(pos - 1 - x, '_', ' ', qry[i - 1 - x]);
        pos -= cnt; i -= cnt;
    };
    auto tail_left = [&](const int cnt) {
        for (int x = lane; x < cnt; x += 64) put(pos - 1 - x, ref[j - 1 - x], ' ', '_');
        pos -= cnt; j -= cnt;
    };
    int cur = 0; /* ANW: 0 SCORING, 1 INSERTION, 2 DELETION */
    const bool affine = algo == DPX_K_ANW || algo == DPX_K_ASW || algo == DPX_K_ASG; /* three states; ASW also stops where H == 0 (move 0) */
    bool done = (algo == DPX_K_LSW || algo == DPX_K_ASW) ? !(a.score[p] > 0 && i > 0 && j > 0) : false; /* score 0: no path (LinearSmithWaterman.cpp:253-257) */
    while (!done) {
        if (algo == DPX_K_LNW && (i == 0 || j == 0)) { /* borders: row 0 is QUERY_INSERTION, column 0 QUERY_DELETION */
            tail_left(j);
            tail_up(i);
            break;
        }
        if (i == 0 || j == 0) break; /* LSW: borders hold 0; ANW: the loop condition of :258 */
        const bool inD = i - lane >= 1 && j - lane >= 1, inU = i - lane >= 1, inL = j - lane >= 1;
        const int cD = inD ? dir_code(base, cs, n, R, i - lane, j - lane) : -1;
        const int cU = inU ? dir_code(base, cs, n, R, i - lane, j) : -1;
        const int cL = inL ? dir_code(base, cs, n, R, i, j - lane) : -1;
        const int qd = inD ? (int)qry[i - lane - 1] : 0, rd = inD ? (int)ref[j - lane - 1] : 0;
        const int c0 = __shfl(cD, 0, 64); /* the walker's own cell */
        if (algo == DPX_K_LSW && (c0 & 4)) break; /* arrived on H == 0 (:222) -- the start cell has H > 0 */
        const int mv = c0 & 3;
        int kind = mv == 3 ? 3 : mv == 2 ? 2 : 1; /* LNW / ANW: anything but up / left is the diagonal */
        if ((algo == DPX_K_LSW || (algo == DPX_K_ASW && cur == 0)) && mv == 0) break;
        if (affine && cur != 0) kind = cur == 1 ? 3 : 2;
        if (affine && kind != 1) { /* a gap: step l is taken while the cells before it extend (bit 2 for I, bit 3 for D) */
            const int c = kind == 3 ? cL : cU, bit = kind == 3 ? 4 : 8;
            const int k = dir_run(c >= 0 && (c & bit));
            const int steps = k == 64 ? 64 : k + 1; /* (an extension never reaches row / column 0: the virtual borders open) */
            cur = k == 64 ? (kind == 3 ? 1 : 2) : 0;
            if (lane < steps) {
                if (kind == 3) put(pos - 1 - lane, ref[j - 1 - lane], ' ', '_');
                else put(pos - 1 - lane, '_', ' ', qry[i - 1 - lane]);
            }
            pos -= steps;
            if (kind == 3) j -= steps; else i -= steps;
            continue;
        }
        /* linear moves, and ANW's diagonal: step l leaves cell l of the line; for LSW every cell after the first must also have H > 0 */
        const int c = kind == 1 ? cD : kind == 2 ? cU : cL;
        bool ok = c >= 0;
        if (algo == DPX_K_LSW) ok = ok && (c & 3) == kind && (lane == 0 || !(c & 4));
        else if (algo == DPX_K_ASW) ok = ok && (c & 3) == 1; /* (a cell with H == 0 ends the run: move 0) */
        else if (kind == 1) ok = ok && (c & 3) != 2 && (c & 3) != 3;
        else ok = ok && (c & 3) == kind;
        const int steps = dir_run(ok); /* >= 1: lane 0 is the walker's cell */
        if (lane < steps) {
            if (kind == 1) put(pos - 1 - lane, rd, qd == rd ? '*' : '|', qd);
            else if (kind == 2) put(pos - 1 - lane, '_', ' ', qry[i - 1 - lane]);
            else put(pos - 1 - lane, ref[j - 1 - lane], ' ', '_');
        }
        pos -= steps;
        if (kind != 3) i -= steps;
        if (kind != 2) j -= steps;
    }
    if (algo == DPX_K_ANW || algo == DPX_K_ASG) { /* :348-360; ASG: column 0 drains the query, the reference before the alignment is free */
        tail_up(i);
        if (algo == DPX_K_ANW) tail_left(j);
    }
    if (lane == 0) tbLen[p] = cap - pos;
}

/* One pair's direction matrix as the oracle's fills write it (c++/backtrack.h enums: directionMain NONE 0, MATCH 1, MISMATCH 2,
 * QUERY_INSERTION 3, QUERY_DELETION 4; directionIndel NONE 0, GAP_OPEN 1, GAP_EXTEND 2), borders in closed form. */
__global__ void __launch_bounds__(256) k_export_dir(const unsigned char *codes, const dpx_pair_dev pr, const char *seq, int algo, int R, int which,
                                                    uint8_t *out) {
    const int n = pr.n, m = pr.m;
    const uint64_t total = (uint64_t)(m + 1) * (uint64_t)(n + 1);
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int i = (int)(idx / (uint64_t)(n + 1)), j = (int)(idx % (uint64_t)(n + 1));
    uint8_t v;
    if (i == 0 || j == 0) {
        if (which != 0 || algo == DPX_K_LSW || algo == DPX_K_ASW || (i == 0 && (j == 0 || algo == DPX_K_ASG))) v = 0; /* (SW borders, ASG's row 0: H = 0, NONE) */
        else v = (j == 0) ? 4 : 3; /* column 0: QUERY_DELETION, row 0: QUERY_INSERTION */
    } else {
        int sh;
        const uint64_t off = dpx_dir_byte(i, j, n, R, (uint64_t)pr.chunkStride * 2u, &sh);
        const int c = (codes[(size_t)pr.matOff * 2u + off] >> sh) & 0xF;
        if (which == 1) v = (c & 4) ? 2 : 1;
        else if (which == 2) v = (c & 8) ? 2 : 1;
        else {
            const int mv = c & 3;
            v = mv == 0 ? 0 : mv == 2 ? 4 : mv == 3 ? 3 : (seq[pr.qryIdx + i - 1] == seq[pr.refIdx + j - 1] ? 1 : 2);
        }
    }
    out[idx] = v;
}

template <class K>
hipError_t dir_launch(K kernel, const dpx_dir_args &a, hipStream_t s) {
    const unsigned wpb = a.wavesPerBlock ? a.wavesPerBlock : 1u;
    if (!a.scratch) return dpx_dev::launch_lds(kernel, dim3(((unsigned)a.numPairs + wpb - 1) / wpb), dim3(64u * wpb), (size_t)a.ldsPerWave * wpb, s, a);
    dpx_dir_args c = a; /* global edge rows (no LDS): DPX_DIR_SCRATCH_SLOTS waves per launch, each launch reusing the scratch */
    for (c.firstSlot = 0; c.firstSlot < a.numPairs; c.firstSlot += DPX_DIR_SCRATCH_SLOTS) {
        const unsigned waves = (unsigned)std::min(a.numPairs - c.firstSlot, DPX_DIR_SCRATCH_SLOTS);
        hipLaunchKernelGGL(kernel, dim3((waves + wpb - 1) / wpb), dim3(64u * wpb), 0, s, c);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <int R>
hipError_t launch_linear_dir_R(const dpx_dir_args &a, bool local, hipStream_t s) {
    if (a.scratch) return local ? dir_launch(k_linear_dir<R, true, true>, a, s) : dir_launch(k_linear_dir<R, false, true>, a, s);
    return local ? dir_launch(k_linear_dir<R, true, false>, a, s) : dir_launch(k_linear_dir<R, false, false>, a, s);
}

template <int R>
hipError_t launch_affine_dir_R(const dpx_dir_args &a, hipStream_t s) {
    return a.scratch ? dir_launch(k_affine_dir<R, true>, a, s) : dir_launch(k_affine_dir<R, false>, a, s);
}

template <int R>
hipError_t launch_asw_dir_R(const dpx_dir_args &a, hipStream_t s) {
    return a.scratch ? dir_launch(k_asw_dir<R, true>, a, s) : dir_launch(k_asw_dir<R, false>, a, s);
}

template <int R>
hipError_t launch_asg_dir_R(const dpx_dir_args &a, hipStream_t s) {
    return a.scratch ? dir_launch(k_asg_dir<R, true>, a, s) : dir_launch(k_asg_dir<R, false>, a, s);
}

} // namespace

hipError_t dpx_launch_fill_dir(const dpx_dir_args &a, int algo, int R, hipStream_t stream) {
    if (a.numPairs <= 0) return hipSuccess;
    if (algo == DPX_K_ANW) {
        switch (R) {
        case 2: return launch_affine_dir_R<2>(a, stream);
        case 4: return launch_affine_dir_R<4>(a, stream);
        case 8: return launch_affine_dir_R<8>(a, stream);
        default: return hipErrorInvalidValue;
        }
    }
    if (algo == DPX_K_ASW) {
        switch (R) {
        case 2: return launch_asw_dir_R<2>(a, stream);
        case 4: return launch_asw_dir_R<4>(a, stream);
        case 8: return launch_asw_dir_R<8>(a, stream);
        default: return hipErrorInvalidValue;
        }
    }
    if (algo == DPX_K_ASG) {
        switch (R) {
        case 2: return launch_asg_dir_R<2>(a, stream);
        case 4: return launch_asg_dir_R<4>(a, stream);
        case 8: return launch_asg_dir_R<8>(a, stream);
        default: return hipErrorInvalidValue;
        }
    }
    if (algo != DPX_K_LNW && algo != DPX_K_LSW) return hipErrorInvalidValue;
    const bool local = algo == DPX_K_LSW;
    switch (R) {
    case 2: return launch_linear_dir_R<2>(a, local, stream);
    case 4: return launch_linear_dir_R<4>(a, local, stream);
    case 8: return launch_linear_dir_R<8>(a, local, stream);
    case 16: /* (LNW only: LSW's per-row best cells would take the wave past 128 VGPRs, its batches stay at <= 8 rows per lane) */
        if (local) return hipErrorInvalidValue;
        return a.scratch ? dir_launch(k_linear_dir<16, false, true>, a, stream) : dir_launch(k_linear_dir<16, false, false>, a, stream);
    default: return hipErrorInvalidValue;
    }
}

hipError_t dpx_launch_traceback_dir(const dpx_dir_args &a, int numPairs, int algo, int R, const uint64_t *tbOff, char *tb, int32_t *tbLen,
                                    hipStream_t stream) {
    if (numPairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_traceback_dir, dim3((unsigned)numPairs), dim3(64), 0, stream, a, numPairs, algo, R, tbOff, tb, tbLen);
    return hipGetLastError();
}

hipError_t dpx_launch_export_dir(const uint8_t *codes, const dpx_pair_dev &pr, const char *seq, int algo, int R, int which, uint8_t *out,
                                 hipStream_t stream) {
    const uint64_t total = (uint64_t)(pr.m + 1) * (uint64_t)(pr.n + 1);
    if (!total) return hipSuccess;
    hipLaunchKernelGGL(k_export_dir, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, codes, pr, seq, algo, R, which, out);
    return hipGetLastError();
}
