/*
 * dpx_basw_kernels.hip -- banded affine-gap Smith-Waterman (DPX_ALGO_BASW) for gfx950: fill, matrix export and traceback.
 *
 * The recurrence is ASW's Gotoh recurrence (dpx_affine_fill.inc) restricted to the band |i-j| <= B-1; every neighbour that is a
 * border cell or lies outside the band reads H = 0, I = D = -infinity (DPX_NEG), so the first in-band cell of a row or column always
 * opens its gap.  The schedule is k_banded_fill's (dpx_bsw_kernels.hip): the wave walks anti-diagonals a = i+j, slot s = (i-j+B-1)>>1,
 * lane l owns the C = ceil(B/64) slots [l*C, l*C+C), all 64 lanes work on every step.  With p = (a+B-1)&1
 *       p=1: up = prev[s], left = prev[s+1]        p=0: up = prev[s-1], left = prev[s]
 * D needs H and D of the up neighbour, I needs H and I of the left neighbour, H needs the diagonal (prev2H[s]).  Only ONE of the two
 * neighbours crosses the lane boundary on a step, so a step moves two values with DPP: H and I (wave_shl:1) on a p=1 step, H and D
 * (wave_shr:1) on a p=0 step.  The lane that has no neighbour receives H = 0, I / D = DPX_NEG.
 * A slot outside the band or the matrix hands H = 0 and I = D = DPX_NEG to the next step (masking I / D to 0 would let a gap be
 * "extended" out of nothing whenever gapOpen < 0).
 *
 * Stores: three planes in the band layout of dpx_layout.h (dpx_band_plane_index): chunk = [plane H, I, D][lane][8] int16, every lane
 * writes 16 contiguous bytes per plane and store.  In-band I / D values are >= gapOpen + gapExtend (an open from H >= 0), so they fit
 * int16 whenever the host's range check passed; slots that hold no cell are written but never read.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "dpx_device.hpp"
#include "dpx_kernels.h"
#include "dpx_layout.h"
#include "dpx_prims.hpp"

namespace {

using dpx::pack_lo16;
using dpx::wave_shl1;
using dpx::wave_shr1;

using namespace dpx_dev; /* stage_bytes, store8, wave_max_u64, CharWin, launch_fill, dispatch_fill */

template <int C>
struct BaswState {
    int prevH[C], prev2H[C]; /* H on anti-diagonals a-1 and a-2 */
    int prevI[C], prevD[C];  /* I and D on anti-diagonal a-1 */
    int qch[C], rch[C];      /* query / reference character of each slot's cell */
    unsigned key[C];         /* running max of (H << 16 | 0xFFFF - A): max score, then earliest step */
    int lim;                 /* B-1 - lane*C: slot c is inside the band on a step of parity p when c + p <= lim */
};

/* INTERIOR: every in-band slot of this anti-diagonal lies inside the matrix, so validity is one compare against the per-lane
 * constant `lim` instead of two against the step's slot window */
template <int C, bool P1, bool INTERIOR>
__device__ __forceinline__ void basw_step(BaswState<C> &st, const int A, int &i0, int &j0, const int lane, const int m, const int n,
                                          const int B, const int match, const int mismatch, const int oe, const int e,
                                          const unsigned char *qL, const unsigned char *rL, int *outH, int *outI, int *outD) {
    const int p = P1 ? 1 : 0;
    if constexpr (P1) i0++; else j0++;
    const int smin = INTERIOR ? 0 : max(max(1 - i0, j0 - n), 0);
    const int smax = INTERIOR ? 0 : min(min(m - i0, j0 - 1), B - 1 - p);
    int upH[C], upD[C], leftH[C], leftI[C];
    if constexpr (P1) {
        const int newq = INTERIOR ? qL[i0 + 64 * C - 2] : qL[min(max(i0 + 64 * C - 2, 0), m - 1)];
        const int tq = wave_shl1(st.qch[0], newq);
#pragma unroll
        for (int c = 0; c < C - 1; c++) st.qch[c] = st.qch[c + 1];
        st.qch[C - 1] = tq;
        const int nbH = wave_shl1(st.prevH[0], 0);
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
        const int nbH = wave_shr1(st.prevH[C - 1], 0);
        const int nbD = wave_shr1(st.prevD[C - 1], DPX_NEG);
#pragma unroll
        for (int c = 0; c < C; c++) {
            leftH[c] = st.prevH[c];
            leftI[c] = st.prevI[c];
            upH[c] = (c > 0) ? st.prevH[c - 1] : nbH;
            upD[c] = (c > 0) ? st.prevD[c - 1] : nbD;
        }
    }
    const unsigned negA = 0xFFFFu - (unsigned)A;
#pragma unroll
    for (int c = 0; c < C; c++) {
        const int sc = (st.qch[c] == st.rch[c]) ? match : mismatch;
        int d = max(upH[c] + oe, upD[c] + e);
        int ii = max(leftH[c] + oe, leftI[c] + e);
        int h = max(max(max(d, ii), st.prev2H[c] + sc), 0);
        bool valid;
        if constexpr (INTERIOR) {
            valid = (c + p) <= st.lim;
        } else {
            const int s = lane * C + c;
            valid = (s >= smin) && (s <= smax);
        }
        h = valid ? h : 0;
        d = valid ? d : DPX_NEG;
        ii = valid ? ii : DPX_NEG;
        st.key[c] = max(st.key[c], ((unsigned)h << 16) | negA);
        st.prev2H[c] = st.prevH[c];
        st.prevH[c] = h;
        st.prevI[c] = ii;
        st.prevD[c] = d;
        outH[c] = h;
        outI[c] = ii;
        outD[c] = d;
    }
}

template <int C, bool PB, bool STORE>
__global__ void __launch_bounds__(DPX_FILL_THREADS) k_basw_fill(const dpx_fill_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int G = (C >= 8) ? 1 : 8 / C; /* steps per 16-byte store */
    constexpr int GG = (G < 2) ? 2 : G;     /* steps per loop iteration (parity pattern repeats every 2) */
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int p = blockIdx.x * (int)a.wavesPerBlock + wv;
    if (p >= a.numPairs) return;
    if (a.order) p = a.order[p];
    const dpx_pair_dev pr = a.pairs[p];
    const int n = pr.n, m = pr.m, B = a.band;
    const int match = a.match, mismatch = a.mismatch, e = a.gapExtend, oe = a.gapOpen + a.gapExtend;
    if (m <= 0 || n <= 0) {
        if (lane == 0) { a.score[p] = 0; a.endRow[p] = 0; a.endCol[p] = 0; }
        return;
    }
    const unsigned char *ref = reinterpret_cast<const unsigned char *>(a.seq + pr.refIdx);
    const unsigned char *qry = reinterpret_cast<const unsigned char *>(a.seq + pr.qryIdx);
    unsigned char *my = smem + (size_t)wv * a.ldsPerWave;
    const unsigned char *qL = stage_bytes(my, qry, m, lane, 64);
    const unsigned char *rL = stage_bytes(my + a.ldsRefOff, ref, n, lane, 64);

    BaswState<C> st;
    st.lim = B - 1 - lane * C;
    { /* character windows of the virtual anti-diagonal a = 1 (the first real step then slides one of them) */
        const int p1 = B & 1;
        const int vi0 = (1 + p1 - (B - 1)) >> 1;
        const int vj0 = 1 - vi0;
#pragma unroll
        for (int c = 0; c < C; c++) {
            const int s = lane * C + c;
            st.qch[c] = qL[min(max(vi0 + s - 1, 0), m - 1)];
            st.rch[c] = rL[min(max(vj0 - s - 1, 0), n - 1)];
            st.prevH[c] = 0;
            st.prev2H[c] = 0;
            st.prevI[c] = DPX_NEG;
            st.prevD[c] = DPX_NEG;
            st.key[c] = 0u;
        }
    }
    /* is every in-band slot of anti-diagonal A inside the matrix?  (true for one contiguous range of A) */
    auto interior = [&](const int A) -> bool {
        const int aa = A + 2, pp = (aa + B - 1) & 1;
        const int ii0 = (aa + pp - (B - 1)) >> 1, jj0 = aa - ii0, top = B - 1 - pp;
        return ii0 >= 1 && ii0 + top <= m && jj0 - top >= 1 && jj0 <= n;
    };
    const int NS = m + n - 1;               /* anti-diagonals a = 2 .. m+n */
    const int numGroups = (NS + G - 1) / G; /* == dpx_band_chunks(m, n, B): no store goes past the pair's last chunk */
    int16_t *Hp = a.mat + pr.matOff + (size_t)lane * 8u;
    const size_t cs = pr.chunkStride;
    int accH[8], accI[8], accD[8];
    int i0 = (1 + (B & 1) - (B - 1)) >> 1;
    int j0 = 1 - i0;
#define DPX_BASW_STORE(grp_)                                                                                              \
    {                                                                                                                     \
        int16_t *at_ = Hp + (size_t)(grp_) * cs;                                                                          \
        store8(at_, accH);                                                                                                \
        store8(at_ + DPX_BAND_PLANE_ELEMS, accI);                                                                         \
        store8(at_ + 2 * DPX_BAND_PLANE_ELEMS, accD);                                                                     \
    }
#define DPX_BASW_BODY(INTERIOR_)                                                                                          \
    _Pragma("unroll") for (int g = 0; g < GG; g += 2) {                                                                  \
        basw_step<C, PB, INTERIOR_>(st, A0 + g, i0, j0, lane, m, n, B, match, mismatch, oe, e, qL, rL, &accH[(g % G) * C], \
                                    &accI[(g % G) * C], &accD[(g % G) * C]);                                              \
        if constexpr (STORE && G == 1) {                                                                                  \
            if (INTERIOR_ || A0 + g < numGroups) DPX_BASW_STORE(A0 + g)                                                   \
        }                                                                                                                 \
        basw_step<C, !PB, INTERIOR_>(st, A0 + g + 1, i0, j0, lane, m, n, B, match, mismatch, oe, e, qL, rL,               \
                                     &accH[((g + 1) % G) * C], &accI[((g + 1) % G) * C], &accD[((g + 1) % G) * C]);       \
        if constexpr (STORE) {                                                                                            \
            if (((g + 1) % G) == G - 1) {                                                                                 \
                const int grp = (A0 + g + 1) / G;                                                                         \
                if (INTERIOR_ || grp < numGroups) DPX_BASW_STORE(grp)                                                     \
            }                                                                                                             \
        }                                                                                                                 \
    }
    /* parity of step A is (A + B + 1) & 1; A0 is even, so even steps have parity PB and odd steps !PB.
     * Three phases: head (some slots outside the matrix), interior, tail. */
    int A0 = 0;
    for (; A0 < NS && !(interior(A0) && interior(A0 + GG - 1)); A0 += GG) { DPX_BASW_BODY(false) }
    for (; A0 + GG <= NS && interior(A0 + GG - 1); A0 += GG) { DPX_BASW_BODY(true) }
    for (; A0 < NS; A0 += GG) { DPX_BASW_BODY(false) }
#undef DPX_BASW_BODY
#undef DPX_BASW_STORE
    /* candidates: every slot's first maximum (within a slot cells arrive in row-major order); across slots max score, min row, min col */
    unsigned long long mine = 0ull;
#pragma unroll
    for (int c = 0; c < C; c++) {
        const int hv = (int)(st.key[c] >> 16);
        if (hv > 0) {
            const int A = 0xFFFF - (int)(st.key[c] & 0xFFFFu);
            const int aa = A + 2;
            const int pp = (aa + B - 1) & 1;
            const int u = 2 * (lane * C + c) + pp;
            const int i = (aa + u - (B - 1)) >> 1;
            const int j = aa - i;
            const unsigned long long k = ((unsigned long long)(unsigned)hv << 40) | ((unsigned long long)(0xFFFFFu - (unsigned)i) << 20) |
                                         (unsigned long long)(0xFFFFFu - (unsigned)j);
            mine = k > mine ? k : mine;
        }
    }
    const unsigned long long top = wave_max_u64(mine);
    if (lane == 0) {
        const int hv = (int)(top >> 40);
        a.score[p] = hv;
        a.endRow[p] = hv > 0 ? (int)(0xFFFFFu - (unsigned)((top >> 20) & 0xFFFFFu)) : 0;
        a.endCol[p] = hv > 0 ? (int)(0xFFFFFu - (unsigned)(top & 0xFFFFFu)) : 0;
    }
}

/* ---- one pair's plane as the row-major (m+1) x (n+1) matrix: borders and cells outside the band are 0 in every plane ---- */
/* (dpx_band::cell_in_band is this test written over in_band(); with it k_basw_export and both walks compile to other instructions) */
__device__ __forceinline__ bool basw_in_band(const int i, const int j, const int band) {
    const int dlt = i - j;
    return i >= 1 && j >= 1 && dlt <= band - 1 && -dlt <= band - 1;
}

__global__ void k_basw_export(const int16_t *mat, dpx_pair_dev pr, int plane, int band, int16_t *out) {
    const int n = pr.n, m = pr.m;
    const size_t total = (size_t)(m + 1) * (size_t)(n + 1);
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int i = (int)(idx / (size_t)(n + 1));
        const int j = (int)(idx % (size_t)(n + 1));
        out[idx] = basw_in_band(i, j, band) ? mat[pr.matOff + dpx_band_plane_index(i, j, band, plane, pr.chunkStride)] : (int16_t)0;
    }
}

/* ---- traceback: one lane per pair, ASW's three-state walk (dpx_traceback_kernels.hip: tb_walk_lane) over the band layout.  The stored I / D
 * of a border or out-of-band neighbour are 0, not -infinity: such a neighbour is "always GAP_OPEN", as row 1 / column 1 are in ASW. ---- */
struct BaswView {
    const int16_t *mat;
    uint64_t off;
    uint32_t cs;
    int band;
    __device__ __forceinline__ int get(int i, int j, int plane) const {
        return basw_in_band(i, j, band) ? (int)mat[off + dpx_band_plane_index(i, j, band, plane, cs)] : 0;
    }
};

__global__ void k_basw_traceback(const dpx_fill_args a, int numPairs, const int32_t *endRow, const int32_t *endCol, const uint64_t *tbOff,
                                 char *tb, int32_t *tbLen) {
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
    const int match = a.match, mismatch = a.mismatch, o = a.gapOpen, e = a.gapExtend;
    const BaswView v{a.mat, pr.matOff, pr.chunkStride, band};
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
    int cur = 0; /* 0 SCORING, 1 INSERTION, 2 DELETION */
    while (i != 0 && j != 0) {
        if (cur == 0) {
            if (v.get(i, j, 0) <= 0) break; /* (also: a gap opened out of a cell outside the band, which reads H = 0) */
            const bool eq = qw.get(i - 1) == rw.get(j - 1);
            const int mm = v.get(i - 1, j - 1, 0) + (eq ? match : mismatch);
            const int D = v.get(i, j, 2), I = v.get(i, j, 1);
            const int vmax = max(D, mm);
            if (I >= vmax) cur = 1;
            else if (D >= mm) cur = 2;
            else { EMIT(rw.get(j - 1), eq ? '*' : '|', qw.get(i - 1)); i--; j--; }
        } else if (cur == 1) {
            const bool open = !basw_in_band(i, j - 1, band) || (v.get(i, j - 1, 0) + o + e >= v.get(i, j - 1, 1) + e);
            if (open) cur = 0;
            EMIT(rw.get(j - 1), ' ', '_'); j--;
        } else {
            const bool open = !basw_in_band(i - 1, j, band) || (v.get(i - 1, j, 0) + o + e >= v.get(i - 1, j, 2) + e);
            if (open) cur = 0;
            EMIT('_', ' ', qw.get(i - 1)); i--;
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

/* -----------------------------------------------------------------------------------------------------
 * Wave-cooperative traceback: k_traceback_wave's scheme (dpx_traceback_kernels.hip) for the three band-layout planes.  One WAVE owns a pair; lane c
 * fetches column cLo + c of a window of 48 rows x 64 columns of H, I and D around the walker into LDS (one 112-byte line per column and
 * plane; cells outside the band, the matrix or on the borders are 0) -- only the three 8-row groups around the walker's diagonal unless the
 * walk left the last window sideways -- and the walk takes RUNS: every lane decides one cell of the line the path would follow next (the
 * walker's diagonal in SCORING, its row in INSERTION, its column in DELETION) and a ballot gives the number of steps the path really
 * follows.  The band layout has no 16-byte column pieces (the rows of a column lie on consecutive anti-diagonals): 2-byte loads through
 * dpx_band_plane_index, as the linear-gap banded walk does.  A neighbour outside the band reads I = D = 0 in the window, not -infinity:
 * the two gap states treat it as "the gap was opened here" without comparing through it.
 * ----------------------------------------------------------------------------------------------------- */
struct BaswWin {
    static constexpr int G = 6;             /* row groups of a window */
    static constexpr int GL = 3;            /* row groups of a banded (diagonal-following) window column */
    static constexpr int WR = 8 * G;        /* rows R0+1 .. R0+WR; columns cLo .. cLo+63, one per lane */
    static constexpr int CS = WR + 8;       /* int16 elements between two columns in LDS */
    static constexpr int kBytes = 3 * 64 * CS * 2;
};

__global__ void __launch_bounds__(64) k_basw_traceback_wave(const dpx_fill_args a, int numPairs, const int32_t *endRow, const int32_t *endCol,
                                                            const uint64_t *tbOff, char *tb, int32_t *tbLen) {
    constexpr int G = BaswWin::G, GL = BaswWin::GL, WR = BaswWin::WR, CS = BaswWin::CS;
    extern __shared__ __attribute__((aligned(16))) unsigned char smemTb[];
    int16_t *win = reinterpret_cast<int16_t *>(smemTb); /* win[(plane * 64 + (jj - cLo)) * CS + (ii - R0 - 1)] = plane[ii][jj] */
    const int p = blockIdx.x;
    const int lane = threadIdx.x;
    if (p >= numPairs) return;
    const dpx_pair_dev pr = a.pairs[p];
    const int n = pr.n, m = pr.m, B = a.band;
    const unsigned char *ref = reinterpret_cast<const unsigned char *>(a.seq + pr.refIdx);
    const unsigned char *qry = reinterpret_cast<const unsigned char *>(a.seq + pr.qryIdx);
    const int16_t *base = a.mat + pr.matOff;
    const uint32_t cs = pr.chunkStride;
    const int cap = (m + n + 1 + 3) & ~3;
    char *lr = tb + tbOff[p], *lx = lr + cap, *lq = lx + cap;
    int pos = cap;
    const int match = a.match, mismatch = a.mismatch, g = a.gapOpen, ext = a.gapExtend;
    int i = __builtin_amdgcn_readfirstlane(endRow[p]), j = __builtin_amdgcn_readfirstlane(endCol[p]);
    int R0 = 1 << 28, cLo = 1 << 28;
    int diag0 = 0;         /* i - j of the cell the window was anchored on */
    bool banded = false;   /* ... and whether only the groups around that diagonal were fetched */
    bool wantFull = false; /* the walk left the last window sideways (a long gap): fetch whole columns next time */
    uint32_t chR = 0u, chQ = 0u; /* reference character of this lane's column; query character of window row `lane` */
    auto stored = [&](const int ii, const int jj) -> bool { return ii <= m && jj <= n && basw_in_band(ii, jj, B); };
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
    /* what issue() loaded becomes the window in LDS, cells without storage masked to 0 */
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
                    d[e >> 1] |= (stored(ii2, jc) ? raw[(pl * CNT + gi) * 8 + e] : 0u) << ((e & 1) * 16);
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
    using std::integral_constant;
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
        using I0 = integral_constant<int, 0>;
        using I1 = integral_constant<int, 1>;
        using I2 = integral_constant<int, 2>;
        using I3 = integral_constant<int, 3>;
        if (banded) { /* the usual window: three row groups of all three planes at once (72 two-byte loads in flight) */
            uint32_t raw[3 * GL * 8];
            issue(I0{}, I3{}, integral_constant<int, GL>{}, raw, gBase, gFirst, jc);
            commit(I0{}, I3{}, integral_constant<int, GL>{}, raw, gBase, gFirst, jc);
        } else { /* whole columns (after a long gap; rare): plane by plane, 48 loads in flight, to keep the kernel's registers down */
            uint32_t raw[G * 8];
            issue(I0{}, I1{}, integral_constant<int, G>{}, raw, gBase, gFirst, jc);
            commit(I0{}, I1{}, integral_constant<int, G>{}, raw, gBase, gFirst, jc);
            issue(I1{}, I1{}, integral_constant<int, G>{}, raw, gBase, gFirst, jc);
            commit(I1{}, I1{}, integral_constant<int, G>{}, raw, gBase, gFirst, jc);
            issue(I2{}, I1{}, integral_constant<int, G>{}, raw, gBase, gFirst, jc);
            commit(I2{}, I1{}, integral_constant<int, G>{}, raw, gBase, gFirst, jc);
        }
        chQ = okQ ? rq : 0u;
        chR = okR ? rr : 0u;
        asm volatile("" : "+v"(chQ), "+v"(chR)); /* the two characters are waited for here, not in every trip of the walk */
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
    auto cell = [&](const int pl, const int col, const int row) -> int { return (int)win[(pl * 64 + col) * CS + row]; };
    /* number of lanes that continue a run which starts at lane `from` and goes DOWN the lanes while `on` holds (lane 0 is never on) */
    auto run_down = [&](const bool on, const int from) -> int {
        const unsigned long long inv = ~__builtin_amdgcn_ballot_w64(on) << (63 - from);
        return inv ? __builtin_clzll(inv) : 64;
    };
    /* SCORING decision of window cell (rq, cq) (>= 1 each): 0 diagonal, 1 to INSERTION, 2 to DELETION, 3 stop (H = 0) */
    auto decide_cell = [&](const int rq, const int cq, const uint32_t rc, int &qcOut) -> uint32_t {
        const int qc = __builtin_amdgcn_ds_bpermute(rq << 2, (int)chQ);
        qcOut = qc;
        const int ii = R0 + 1 + rq, jc = cLo + cq;
        const int dg = cell(0, cq - 1, rq - 1), I = cell(1, cq, rq), D = cell(2, cq, rq);
        const int mm = dg + ((uint32_t)qc == rc ? match : mismatch);
        uint32_t d = I >= max(D, mm) ? 1u : (D >= mm ? 2u : 0u);
        if (cell(0, cq, rq) <= 0) d = 3u; /* H = 0 (also every cell outside the band): the local alignment starts here */
        if (ii <= 0 || jc <= 0) d = 3u;
        return d;
    };
    /* (r, c) = the walker's window cell; lane l decides the cell of the walker's diagonal in its own column */
    auto decide_diag = [&](const int r, const int c, int &qcOut) -> uint32_t {
        const int rr = r - (c - lane);
        const bool usable = lane <= c && lane >= 1 && rr >= 1;
        const uint32_t d = decide_cell(usable ? rr : 1, usable ? lane : 1, chR, qcOut);
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
        const int qc = __builtin_amdgcn_ds_bpermute(max(r - lane, 0) << 2, (int)chQ);
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
                    else break; /* H = 0 */
                }
                continue;
            }
            cur = __builtin_amdgcn_readlane((int)d, c); /* 1: to INSERTION, 2: to DELETION */
            if (cur == 3) break;                         /* H is 0 here */
        } else if (cur == 1) {
            /* INSERTION: steps to the left along row i until (and including) the cell where the gap was opened; lane l decides the cell in
             * column l.  The left neighbour outside the band (or column 0): opened. */
            const int cq = max(lane, 1), jc = cLo + cq;
            const bool opened = !basw_in_band(i, jc - 1, B) || cell(0, cq - 1, r) + g + ext >= cell(1, cq - 1, r) + ext;
            const bool usable = lane <= c && lane >= 1 && jc >= 1 && (!banded || (i - j) - diag0 + (c - lane) <= 6);
            const int cont = run_down(usable && !opened, c); /* cells the gap passes through */
            const bool stops = c - cont >= 1 && cLo + c - cont >= 1 && (!banded || (i - j) - diag0 + cont <= 6); /* ... then a usable cell that opened it (else: the window's edge) */
            const int len = cont + (stops ? 1 : 0);
            emit_left(c, len); j -= len;
            if (stops) cur = 0;
        } else {
            /* DELETION: steps up along column j; lane k decides the cell k rows above the walker.  The upper neighbour outside the band (or
             * row 0): opened. */
            const int rq = max(r - lane, 1), ii = R0 + 1 + rq;
            const bool opened = !basw_in_band(ii - 1, j, B) || cell(0, c, rq - 1) + g + ext >= cell(2, c, rq - 1) + ext;
            const bool usable = r - lane >= 1 && ii >= 1 && (!banded || (i - j) - diag0 - lane >= -7);
            const unsigned long long m64 = __builtin_amdgcn_ballot_w64(!(usable && !opened)); /* first lane that ends the run */
            const int cont = m64 ? __builtin_ctzll(m64) : 64;
            const bool stops = r - cont >= 1 && R0 + 1 + r - cont >= 1 && (!banded || (i - j) - diag0 - cont >= -7);
            const int len = cont + (stops ? 1 : 0);
            emit_up(r, len); i -= len;
            if (stops) cur = 0;
        }
    }
    if (lane == 0) tbLen[p] = cap - pos;
}

} // namespace

hipError_t dpx_launch_basw_fill(const dpx_fill_args &a, int C, bool store, size_t ldsBytes, hipStream_t stream) {
    if (a.numPairs <= 0) return hipSuccess;
    return dispatch_fill(C, a.band, store, [&](auto c, auto pb, auto st) {
        return launch_fill(k_basw_fill<decltype(c)::value, decltype(pb)::value, decltype(st)::value>, a, a, ldsBytes, stream);
    });
}

hipError_t dpx_launch_basw_export(const int16_t *mat, const dpx_pair_dev &pr, int plane, int band, int16_t *out, hipStream_t stream) {
    const size_t total = (size_t)(pr.m + 1) * (size_t)(pr.n + 1);
    unsigned blocks = (unsigned)((total + 255) / 256);
    if (blocks > 4096u) blocks = 4096u;
    hipLaunchKernelGGL(k_basw_export, dim3(blocks), dim3(256), 0, stream, mat, pr, plane, band, out);
    return hipGetLastError();
}

hipError_t dpx_launch_basw_traceback(const dpx_fill_args &a, int numPairs, int walk, const uint64_t *tbOff, char *tb, int32_t *tbLen,
                                     hipStream_t stream) {
    if (numPairs <= 0) return hipSuccess;
    if (walk == 2) /* one wave per pair with an LDS window */
        hipLaunchKernelGGL(k_basw_traceback_wave, dim3((unsigned)numPairs), dim3(64), (size_t)BaswWin::kBytes, stream, a, numPairs, a.endRow,
                           a.endCol, tbOff, tb, tbLen);
    else
        hipLaunchKernelGGL(k_basw_traceback, dim3((unsigned)((numPairs + 63) / 64)), dim3(64), 0, stream, a, numPairs, a.endRow, a.endCol, tbOff,
                           tb, tbLen);
    return hipGetLastError();
}
