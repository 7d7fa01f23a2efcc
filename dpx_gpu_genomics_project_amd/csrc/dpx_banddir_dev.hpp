/*
 * dpx_banddir_dev.hpp -- device code shared by the band-direction units: dpx_banddir_kernels.hip (4-bit codes), dpx_bdx_kernels.hip
 * (the same under a table and / or BAXT's extension mode), dpx_bd2_kernels.hip (two-piece gaps, 8-bit codes), dpx_bdl_kernels.hip
 * (BSW / BASW: the local forms of walk and export, LOCAL below) and dpx_lb2_kernels.hip (BASW under two gap pieces: LOCAL over the
 * 8-bit codes).
 *
 * Shared as templates (outside the fills' hot loops): window_push, the launch helper of the fills, the two codecs over dpx_banddir.h /
 * dpx_banddir2.h, the walk (banddir_walk) and the export loop (banddir_export).  Shared as text: the fills' frame, dpx_banddir_fill.inc,
 * included inside each fill kernel, and the scan after a step, DPX_BANDDIR_SCAN_AFTER below.  NOT shared, on purpose: bdir_step, bdx_step,
 * bd2_step, lb2_step and bdl_step (the last is dpx_bdl_dev.hpp's, one text for the two local units, dpx_bdl_kernels.hip and dpx_bdlt_kernels.hip).
 * How the same operations are grouped into functions moves the compiler's schedule of these fills (profiles/band_sharing_ab.md); text
 * included inside the kernel does not (profiles/banddir_sharing_ab.md).
 */
#ifndef DPX_BANDDIR_DEV_HPP
#define DPX_BANDDIR_DEV_HPP

#include "dpx_band_affine.hpp"
#include "dpx_banddir2.h"

namespace dpx_band {

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

/* launches a fill with its own argument block; the block shape comes from f (a direction batch sizes its LDS per wave, not as a
 * four-wave request) */
template <class K, class Args>
hipError_t launch_banddir_fill(K kernel, const Args &args, const dpx_fill_args &f, hipStream_t s) {
    const unsigned wpb = f.wavesPerBlock ? f.wavesPerBlock : 1u;
    const size_t lds = (size_t)f.ldsPerWave * wpb;
    if (lds > 160u * 1024u) return hipErrorInvalidValue;
    if (lds > 64u * 1024u) { /* opt in to more than the default 64 KiB of dynamic LDS */
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const unsigned grid = ((unsigned)f.numPairs + wpb - 1) / wpb;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64u * wpb), lds, s, args);
    return hipGetLastError();
}

/* ---- the two codecs: what walk and export need to know about a stored code.  A move is 1 (diagonal) or the number of a gap plane; odd
 * planes run along the row (I: left), even ones along the column (D: up).  code_at reads cell (i, j)'s code from `bytes`, laid out with
 * chunk stride cs, the byte index taken & wrap (the walk's ring; ~0 for a pair's own chunks).  decode gives the exported value of one
 * code for selector `which`, -1 for a diagonal move of the H plane (MATCH or MISMATCH by the two bases). ---- */
struct NibbleCodec { /* dpx_banddir.h: moves 1-3 in bits 0-1, I extends = 4, D extends = 8 */
    static constexpr int kMoveMask = 3;
    static __device__ __forceinline__ int log2_group(const int B) { return 5 - dpx_log2(dpx_band_cpl(B)); }
    static __device__ __forceinline__ int chunks(const int m, const int n, const int B) { return (int)dpx_banddir_chunks(m, n, B); }
    static __device__ __forceinline__ int code_at(const unsigned char *bytes, const uint64_t wrap, const int i, const int j, const int B, const uint64_t cs) {
        int sh;
        const uint64_t off = dpx_banddir_byte(i, j, B, cs, &sh);
        return ((int)bytes[off & wrap] >> sh) & 0xF;
    }
    static __device__ __forceinline__ int move(const int c) { return max(c & 3, 1); } /* (a move of 0 is taken as diagonal) */
    static __device__ __forceinline__ bool is_move(const int) { return true; }         /* (so every stored value is a move) */
    static __device__ __forceinline__ int extend_bit(const int plane) { return 16 >> (plane - 1); } /* plane 3 (I): 4, plane 2 (D): 8 */
    static __device__ __forceinline__ bool is_i(const int which) { return which == 1; }
    static __device__ __forceinline__ bool is_d(const int which) { return which == 2; }
    static __device__ __forceinline__ int decode(const int c, const int which) {
        if (which == 1) return (c & 4) ? 2 : 1;
        if (which == 2) return (c & 8) ? 2 : 1;
        const int mv = c & 3;
        return mv == 2 ? 4 : mv == 3 ? 3 : -1;
    }
};
struct ByteCodec { /* dpx_banddir2.h: moves 1-5 in bits 0-2, I1 / D1 / I2 / D2 extend = 8 / 16 / 32 / 64 */
    static constexpr int kMoveMask = 7;
    static __device__ __forceinline__ int log2_group(const int B) { return 4 - dpx_log2(dpx_band_cpl(B)); }
    static __device__ __forceinline__ int chunks(const int m, const int n, const int B) { return (int)dpx_banddir2_chunks(m, n, B); }
    static __device__ __forceinline__ int code_at(const unsigned char *bytes, const uint64_t wrap, const int i, const int j, const int B, const uint64_t cs) {
        return (int)bytes[dpx_banddir2_byte(i, j, B, cs) & wrap];
    }
    static __device__ __forceinline__ int move(const int c) { return c & 7; }
    static __device__ __forceinline__ bool is_move(const int mv) { return mv >= 1 && mv <= 5; }
    static __device__ __forceinline__ int extend_bit(const int plane) { return plane == 3 ? 8 : plane == 2 ? 16 : plane == 5 ? 32 : 64; }
    static __device__ __forceinline__ bool is_i(const int which) { return which == 1 || which == 3; }
    static __device__ __forceinline__ bool is_d(const int which) { return which == 2 || which == 4; }
    static __device__ __forceinline__ int decode(const int c, const int which) {
        const int mv = c & 7;
        if (which == 1) return (c & 8) ? 2 : 1;
        if (which == 2) return (c & 16) ? 2 : 1;
        if (which == 3) return (c & 32) ? 2 : 1;
        if (which == 4) return (c & 64) ? 2 : 1;
        if (which == 5) return (mv == 2 || mv == 3) ? 1 : (mv == 4 || mv == 5) ? 2 : 0;
        return (mv == 2 || mv == 4) ? 4 : (mv == 3 || mv == 5) ? 3 : -1;
    }
};

/* -----------------------------------------------------------------------------------------------------
 * Traceback: one WAVE per pair, k_traceback_dir's run scheme (dpx_dir_kernels.hip) over an LDS ring of code chunks.  The walk moves to
 * strictly smaller anti-diagonals and one chunk holds Gd whole anti-diagonals of the band, so the chunks a path needs are known in
 * advance: the ring holds kRing consecutive chunks as two halves, the walker stands in the upper half, and when it has left it the wave
 * drops that half and streams the next lower one in (every lane its own 16 bytes of each chunk: whole-KiB loads, all in flight at once).
 * A step of the walk: every lane reads the code of one cell of the line the path would follow next from LDS (the walker's diagonal in
 * SCORING, its row in an I plane, its column in a D plane) and a ballot gives the number of cells the path really follows; a cell below
 * the ring ends the run early, and the next trip slides the ring.  In SCORING the cell's move names the plane; in a gap state the walk
 * follows that plane's own extend bit.  Then ANW's two tails.  `ring` is the kernel's own kRingBytes of LDS.
 * LOCAL (k_bdl_traceback, BSW / BASW; k_lb2_traceback, BASW under two gap pieces): the walk stops in SCORING on the first cell whose H
 * is 0 -- BSW (`linear`): bit 2 of its code, BASW: move 0 under the codec's move mask; a cell without a code (border, outside the band)
 * has H = 0 too -- and there are no tails.  BSW has no gap states: a gap move is a single step and the next cell is read in SCORING.
 * ----------------------------------------------------------------------------------------------------- */
constexpr int kRing = 16; /* chunks in LDS */
constexpr int kRingBytes = kRing * (int)DPX_BANDDIR_CHUNK_BYTES;

template <class Codec, bool LOCAL = false>
__device__ __forceinline__ void banddir_walk(unsigned char *ring, const dpx_fill_args &a, const int numPairs, const uint64_t *tbOff, char *tb,
                                             int32_t *tbLen, [[maybe_unused]] const bool linear = false) {
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
    const int sg = Codec::log2_group(B); /* Gd = 2^sg */
    const int numChunks = Codec::chunks(m, n, B);
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
        return Codec::code_at(ring, (uint64_t)(kRingBytes - 1), ci, cj, B, DPX_BANDDIR_CHUNK_BYTES);
    };
    auto run_of = [&](const bool cont) -> int { /* leading lanes (from lane 0) whose condition holds */
        const unsigned long long mask = __ballot(cont);
        return ~mask == 0ull ? 64 : __builtin_ctzll(~mask);
    };
    auto put = [&](const int at, const int rc, const int xc, const int qc) { lr[at] = (char)rc; lx[at] = (char)xc; lq[at] = (char)qc; };
    int cur = 0; /* 0 SCORING, else the move number of the gap plane the walk stands in */
    while (i != 0 && j != 0) {
        const int hw = ((i + j - 2) >> sg) / kHalf; /* the walker's half */
        if (!have || hw < hTop) {
            __syncthreads(); /* the reads of the last trip are done before the ring changes */
            if (!have) { hTop = hw; load_half(hw); load_half(hw - 1); have = true; }
            else while (hTop > hw) { hTop--; load_half(hTop - 1); }
            __syncthreads();
        }
        const int c0 = code(i, j); /* the walker's own cell: the same byte for every lane */
        if (c0 < 0) break;         /* (global: cannot happen, the walker stands on a stored cell of the ring's upper half; LOCAL: a border cell or one outside the band, H = 0) */
        if constexpr (LOCAL) { /* H == 0 ends the walk where it stands in SCORING: BSW's bit 2, BASW's move 0 */
            if (cur == 0 && (linear ? (c0 & 4) != 0 : (c0 & Codec::kMoveMask) == 0)) break;
        }
        const int kind = cur != 0 ? cur : Codec::move(c0);
        if (!Codec::is_move(kind)) break; /* (cannot happen: a stored cell has a move) */
        if constexpr (LOCAL) {
            if (kind != 1 && linear) { /* BSW: a gap move is one step, the next cell says its own move (there is no extend bit) */
                const bool left = kind == 3;
                if (lane == 0) {
                    if (left) put(pos - 1, ref[j - 1], ' ', '_');
                    else put(pos - 1, '_', ' ', qry[i - 1]);
                }
                pos--;
                if (left) j--; else i--;
                continue;
            }
        }
        if (kind != 1) { /* a gap: step l is taken while the cells before it extend in this plane; the cell that opens ends it */
            const bool left = (kind & 1) != 0; /* an I plane: along the row */
            const int bit = Codec::extend_bit(kind);
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
        /* (LOCAL: a run ends on the first cell that is zero or not diagonal; BSW's zero cells carry a move, so bit 2 counts) */
        const int runMask = (LOCAL && linear) ? 7 : Codec::kMoveMask;
        const int steps = run_of(c >= 0 && (lane == 0 || (c & runMask) == 1));
        if (steps == 0) break; /* (cannot happen) */
        if (lane < steps) {
            const int qd = (int)qry[i - lane - 1], rd = (int)ref[j - lane - 1];
            put(pos - 1 - lane, rd, qd == rd ? '*' : '|', qd);
        }
        pos -= steps;
        i -= steps;
        j -= steps;
    }
    if constexpr (!LOCAL) { /* ANW's tails: the rest of column 0 as deletions, then the rest of row 0 as insertions (at most one of the two is left) */
        for (int x = lane; x < i; x += 64) put(pos - 1 - x, '_', ' ', qry[i - 1 - x]);
        pos -= max(i, 0);
        for (int x = lane; x < j; x += 64) put(pos - 1 - x, ref[j - 1 - x], ' ', '_');
        pos -= max(j, 0);
    }
    if (lane == 0) tbLen[p] = cap - pos;
}

/* One pair's plane `which` as the oracles write it (c++/backtrack.h enums: directionMain NONE 0, MATCH 1, MISMATCH 2, QUERY_INSERTION 3,
 * QUERY_DELETION 4; directionIndel NONE 0, GAP_OPEN 1, GAP_EXTEND 2): 0 outside the band; the in-band border cells of H as ANW exports
 * them; I on the band's lower edge and D on its upper edge are GAP_OPEN by the geometry (-inf >= -inf); else the codec's decode.
 * LOCAL (BSW / BASW): every plane is 0 on the borders, and the edge planes are decoded like every other cell (the neighbour outside the
 * band read H = 0, D = -inf, so the stored bit says GAP_OPEN). */
template <class Codec, bool LOCAL = false>
__device__ __forceinline__ void banddir_export(const unsigned char *codes, const dpx_pair_dev &pr, const char *seq, const int band, const int which,
                                               uint8_t *out) {
    const int n = pr.n, m = pr.m;
    const uint64_t total = (uint64_t)(m + 1) * (uint64_t)(n + 1);
    const bool iPlane = Codec::is_i(which), dPlane = Codec::is_d(which);
    for (uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * blockDim.x) {
        const int i = (int)(idx / (uint64_t)(n + 1)), j = (int)(idx % (uint64_t)(n + 1));
        uint8_t v = 0;
        if (in_band(i, j, band)) {
            if (LOCAL && (i == 0 || j == 0)) {
                v = 0;
            } else if (i == 0 || j == 0) {
                v = (which != 0 || (i | j) == 0) ? 0 : (j == 0 ? 4 : 3); /* column 0: QUERY_DELETION, row 0: QUERY_INSERTION */
            } else if (!LOCAL && ((iPlane && i - j == band - 1) || (dPlane && j - i == band - 1))) {
                v = 1;
            } else {
                const int d = Codec::decode(Codec::code_at(codes + (size_t)pr.matOff * 2u, ~0ull, i, j, band, (uint64_t)pr.chunkStride * 2u), which);
                v = d >= 0 ? d : (seq[pr.qryIdx + i - 1] == seq[pr.refIdx + j - 1] ? 1 : 2);
            }
        }
        out[idx] = v;
    }
}

/* ---- the scan after a step of a fill in extension mode, text over the names of dpx_banddir_fill.inc ----
 * Scalar registers.  At C = 8 the step alone takes most of the 102 scalar registers (every cell of a border step makes several compare
 * masks), and the scan's state is scalar too.  As a scalar pair behind a wave-uniform branch with one v_readlane, the row-m pick-up
 * made the C = 8 fills without the drop test 198 VGPRs wide; branch-free and per lane it costs two VGPRs.  How the owning register is
 * selected then decides between scalar spills to VGPR lanes only and a scratch frame, so DPX_BANDDIR_SCAN_AFTER has two forms of one
 * function of the same values, chosen by the kernel's constexpr kPickUniform.  What each form compiled to in k_bdx_fill at C = 8
 * (private_segment_fixed_size in bytes; every other instantiation had none under any form; <C, PB, EXT, TABLE, SCAN>):
 *   (a) the per-lane register index m - i0 - lane * C compared with c, no geometry test -- k_bdx_fill when SCAN == 1, k_bd2_fill always:
 *       no scratch there; k_bdx_fill with SCAN == 2: <8, 1, 1, 0, 2> 20 bytes, <8, 0, 1, 1, 2> 36 bytes
 *   (b) the wave-uniform index (m - i0) % C compared with c, a lane compare, and the geometry test of DPX_BAND_SCAN_AFTER, which (a)
 *       shows to be redundant -- k_bdx_fill when SCAN == 2: no scratch there; with SCAN == 1: <8, 1, 1, 1, 1> and <8, 1, 1, 0, 1> 36 bytes
 *   (b) without the geometry test, with SCAN == 2: <8, 1, 1, 1, 2> 36 bytes
 * The frame is never accessed in any of these (the scalar spills go to VGPR lanes), but a kernel with one is launched with scratch.
 * Below C = 8 either form is safe to use for both modes; at C = 8 a change to this text, or a compiler update, has to be checked against
 * tests/test_bdx_kernels_isa.py, which holds all 48 instantiations to zero scratch.
 *
 * After step A_, whose H values stand in st.prevH and whose first slot is row i0: the row-m pick-up into the owning lane's (qeScore,
 * qeCol) -- no branch and no readlane, so that the body of two steps stays straight-line code -- then (SCAN == 2) the anti-diagonal's
 * maximum, its holder with the smallest row and the drop test, which sets lastDiag and stop.  A macro over the kernel's own names, as
 * DPX_BAND_SCAN_AFTER is (as a function taking the state by reference that text cost registers). */
#define DPX_BANDDIR_SCAN_AFTER(A_)                                                                                        \
    if constexpr (SCAN > 0) {                                                                                             \
        const int a_ = (A_) + 2;                                                                                          \
        { /* row m on this step is slot m - i0: register (m - i0) % C of lane (m - i0) / C.  A slot holds a cell of the       */ \
          /* matrix (a border cell included) exactly when its H is not DPX_NEG, so no geometry is tested: a lane that does    */ \
          /* not own the slot, or an empty slot, offers DPX_NEG, which is below every qeScore.                               */ \
            int pick_ = DPX_NEG;                                                                                          \
            if constexpr (kPickUniform) {                                                                                 \
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

} // namespace dpx_band
#endif
