/*
 * dpx_banw_kernels.hip -- banded affine-gap Needleman-Wunsch (DPX_ALGO_BANW) for gfx950: fill, matrix export and traceback.
 *
 * The recurrence is ANW's Gotoh recurrence restricted to the band |i-j| <= B-1, border cells included: H[0][0] = 0, the in-band
 * border cells carry H = gapOpen + k * gapExtend (k <= B-1), and everything outside the band is -infinity (DPX_NEG) in H, I and D.
 * There is no zero floor and no start cell: the score is H[m][n].  The schedule is k_basw_fill's (dpx_basw_kernels.hip): the wave
 * walks anti-diagonals a = i+j, slot s = (i-j+B-1)>>1, lane l owns the C = ceil(B/64) slots [l*C, l*C+C).  With p = (a+B-1)&1
 *       p=1: up = prev[s], left = prev[s+1]        p=0: up = prev[s-1], left = prev[s]
 * and a step moves two values with DPP: H and I (wave_shl:1) on a p=1 step, H and D (wave_shr:1) on a p=0 step.  The lane that has no
 * neighbour receives DPX_NEG for both.  A slot that holds no cell hands H = I = D = DPX_NEG to the next step, except the (at most
 * two) slots of an anti-diagonal a <= B-1 that are the in-band border cells (0, a) and (a, 0): they hand on H = gapOpen + a * gapExtend.
 * Such slots exist only while slot 0 is above row 1, that is in the head phase.
 *
 * Stores: three planes in the band layout of dpx_layout.h (dpx_band_plane_index), every lane writes 16 contiguous bytes per plane and
 * store.  I of a cell on the band's lower edge (i - j = B-1) and D of a cell on its upper edge (j - i = B-1) are -infinity; what the
 * fill stores there (the low half of DPX_NEG + a weight) is NEVER READ: the export and both walks know these cells from the geometry
 * alone and substitute -infinity, so the fill pays nothing for them.  Every other in-band value is finite and fits int16 whenever the
 * host's range check passed; slots that hold no cell are written but never read.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "dpx_kernels.h"
#include "dpx_layout.h"
#include "dpx_prims.hpp"

namespace {

using dpx::pack_lo16;
using dpx::wave_shl1;
using dpx::wave_shr1;

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

/* a string copied into LDS with aligned 16-byte loads; it lands `src & 15` bytes into the buffer (as in dpx_kernels.hip) */
__device__ __forceinline__ unsigned char *stage_bytes(unsigned char *dst16, const unsigned char *src, const int n, const int l, const int G) {
    const unsigned a = (unsigned)(reinterpret_cast<uintptr_t>(src) & 15u);
    const u32x4 *from = reinterpret_cast<const u32x4 *>(src - a);
    u32x4 *to = reinterpret_cast<u32x4 *>(dst16);
    const int blocks = n > 0 ? (int)((a + (unsigned)n + 15u) >> 4) : 0;
    for (int k = l; k < blocks; k += G) to[k] = from[k];
    return dst16 + a;
}

/* eight int32 values -> eight int16, one 16-byte store */
__device__ __forceinline__ void store8(int16_t *dst, const int (&v)[8]) {
    u32x4 w = {pack_lo16(v[0], v[1]), pack_lo16(v[2], v[3]), pack_lo16(v[4], v[5]), pack_lo16(v[6], v[7])};
    *reinterpret_cast<u32x4 *>(dst) = w;
}

template <int C>
struct BanwState {
    int prevH[C], prev2H[C]; /* H on anti-diagonals a-1 and a-2 */
    int prevI[C], prevD[C];  /* I and D on anti-diagonal a-1 */
    int qch[C], rch[C];      /* query / reference character of each slot's cell */
    int lim;                 /* B-1 - lane*C: slot c is inside the band on a step of parity p when c + p <= lim */
    int fin;                 /* H[m][n], picked up on the last anti-diagonal by the lane that owns its slot */
};

/* INTERIOR: every in-band slot of this anti-diagonal lies inside the matrix, so validity is one compare against the per-lane
 * constant `lim` instead of two against the step's slot window; no border slot and not the last anti-diagonal (the caller sees to both) */
template <int C, bool P1, bool INTERIOR>
__device__ __forceinline__ void banw_step(BanwState<C> &st, const int A, int &i0, int &j0, const int lane, const int m, const int n,
                                          const int B, const int match, const int mismatch, const int o, const int oe, const int e,
                                          const int cEnd, const unsigned char *qL, const unsigned char *rL, int *outH, int *outI,
                                          int *outD) {
    const int p = P1 ? 1 : 0;
    if constexpr (P1) i0++; else j0++;
    const int smin = INTERIOR ? 0 : max(max(1 - i0, j0 - n), 0);
    const int smax = INTERIOR ? 0 : min(min(m - i0, j0 - 1), B - 1 - p);
    /* the in-band border cells of this anti-diagonal: (0, a) in slot -i0 and (a, 0) in slot j0, both H = o + a * e, while a <= B-1 */
    const int a = A + 2;
    const int bord = (INTERIOR || a > B - 1) ? DPX_NEG : o + a * e;
    const int sTop = (INTERIOR || a > n) ? -1 : -i0, sLeft = (INTERIOR || a > m) ? -1 : j0;
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
            const int s = lane * C + c;
            const bool valid = (s >= smin) && (s <= smax);
            h = valid ? h : ((s == sTop || s == sLeft) ? bord : DPX_NEG);
            d = valid ? d : DPX_NEG;
            ii = valid ? ii : DPX_NEG;
            st.fin = (last && c == cEnd) ? h : st.fin;
        }
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
__global__ void __launch_bounds__(DPX_FILL_THREADS) k_banw_fill(const dpx_fill_args a) {
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
    const int match = a.match, mismatch = a.mismatch, o = a.gapOpen, e = a.gapExtend, oe = a.gapOpen + a.gapExtend;
    if (m <= 0 || n <= 0) { /* an empty sequence: the end cell is a border cell (in band: the host admits only |m - n| <= B-1) */
        if (lane == 0) { a.score[p] = (m > 0 || n > 0) ? o + max(m, n) * e : 0; a.endRow[p] = max(m, 0); a.endCol[p] = max(n, 0); }
        return;
    }
    const unsigned char *ref = reinterpret_cast<const unsigned char *>(a.seq + pr.refIdx);
    const unsigned char *qry = reinterpret_cast<const unsigned char *>(a.seq + pr.qryIdx);
    unsigned char *my = smem + (size_t)wv * a.ldsPerWave;
    const unsigned char *qL = stage_bytes(my, qry, m, lane, 64);
    const unsigned char *rL = stage_bytes(my + a.ldsRefOff, ref, n, lane, 64);

    BanwState<C> st;
    st.lim = B - 1 - lane * C;
    st.fin = DPX_NEG;
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
    }
    /* the lane and register that own the end cell (m, n) on the last anti-diagonal */
    const int sEnd = (m - n + B - 1) >> 1;
    const int cEnd = (lane == sEnd / C) ? (sEnd % C) : -1;
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
#define DPX_BANW_STORE(grp_)                                                                                              \
    {                                                                                                                     \
        int16_t *at_ = Hp + (size_t)(grp_) * cs;                                                                          \
        store8(at_, accH);                                                                                                \
        store8(at_ + DPX_BAND_PLANE_ELEMS, accI);                                                                         \
        store8(at_ + 2 * DPX_BAND_PLANE_ELEMS, accD);                                                                     \
    }
#define DPX_BANW_BODY(INTERIOR_)                                                                                          \
    _Pragma("unroll") for (int g = 0; g < GG; g += 2) {                                                                  \
        banw_step<C, PB, INTERIOR_>(st, A0 + g, i0, j0, lane, m, n, B, match, mismatch, o, oe, e, cEnd, qL, rL,           \
                                    &accH[(g % G) * C], &accI[(g % G) * C], &accD[(g % G) * C]);                          \
        if constexpr (STORE && G == 1) {                                                                                  \
            if (INTERIOR_ || A0 + g < numGroups) DPX_BANW_STORE(A0 + g)                                                   \
        }                                                                                                                 \
        banw_step<C, !PB, INTERIOR_>(st, A0 + g + 1, i0, j0, lane, m, n, B, match, mismatch, o, oe, e, cEnd, qL, rL,      \
                                     &accH[((g + 1) % G) * C], &accI[((g + 1) % G) * C], &accD[((g + 1) % G) * C]);       \
        if constexpr (STORE) {                                                                                            \
            if (((g + 1) % G) == G - 1) {                                                                                 \
                const int grp = (A0 + g + 1) / G;                                                                         \
                if (INTERIOR_ || grp < numGroups) DPX_BANW_STORE(grp)                                                     \
            }                                                                                                             \
        }                                                                                                                 \
    }
    /* parity of step A is (A + B + 1) & 1; A0 is even, so even steps have parity PB and odd steps !PB.
     * Three phases: head (some slots outside the matrix, border slots), interior, tail.  The interior loop stops short of the last
     * anti-diagonal (A = NS-1), so the end cell is always picked up by the general step. */
    int A0 = 0;
    for (; A0 < NS && !(interior(A0) && interior(A0 + GG - 1)); A0 += GG) { DPX_BANW_BODY(false) }
    for (; A0 + GG < NS && interior(A0 + GG - 1); A0 += GG) { DPX_BANW_BODY(true) }
    for (; A0 < NS; A0 += GG) { DPX_BANW_BODY(false) }
#undef DPX_BANW_BODY
#undef DPX_BANW_STORE
    if (cEnd >= 0) { a.score[p] = st.fin; a.endRow[p] = m; a.endCol[p] = n; }
}

/* ---- geometry shared by the export and the walks.  A cell (i, j), borders included, is in the band when |i - j| <= B-1; the fill stores
 * the in-band cells with i, j >= 1; I on the lower edge and D on the upper edge are -infinity whatever the fill stored there ---- */
__device__ __forceinline__ bool banw_in_band(const int i, const int j, const int band) {
    const int dlt = i - j;
    return dlt <= band - 1 && -dlt <= band - 1;
}
__device__ __forceinline__ bool banw_cell_in_band(const int i, const int j, const int band) { /* ... and has storage */
    return i >= 1 && j >= 1 && banw_in_band(i, j, band);
}
/* H of the in-band border cell (i, j), i == 0 or j == 0 */
__device__ __forceinline__ int banw_border(const int i, const int j, const int o, const int e) { return (i | j) == 0 ? 0 : o + (i + j) * e; }
/* is `plane` of the stored cell (i, j) minus infinity? */
__device__ __forceinline__ bool banw_edge(const int i, const int j, const int band, const int plane) {
    return (plane == 1 && i - j == band - 1) || (plane == 2 && j - i == band - 1);
}

/* one pair's plane as the row-major (m+1) x (n+1) matrix: 0 outside the band; in-band borders carry H = o + k * e and I = D = 0 (as ANW
 * exports them); an in-band I or D that is -infinity exports as -32768 */
__global__ void k_banw_export(const int16_t *mat, dpx_pair_dev pr, int plane, int band, int o, int e, int16_t *out) {
    const int n = pr.n, m = pr.m;
    const size_t total = (size_t)(m + 1) * (size_t)(n + 1);
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int i = (int)(idx / (size_t)(n + 1));
        const int j = (int)(idx % (size_t)(n + 1));
        int v = 0;
        if (banw_in_band(i, j, band)) {
            if (i == 0 || j == 0) v = plane == 0 ? banw_border(i, j, o, e) : 0;
            else if (banw_edge(i, j, band, plane)) v = -32768;
            else v = mat[pr.matOff + dpx_band_plane_index(i, j, band, plane, pr.chunkStride)];
        }
        out[idx] = (int16_t)v;
    }
}

/* ---- traceback: one lane per pair, ANW's three-state walk (dpx_kernels.hip: tb_walk_lane) over the band layout, with ANW's two tails.
 * The walk stands on stored cells only; the neighbours it reads are in band (the diagonal one always; the left / upper one because the
 * gap it came through is finite) or border cells, which open the gap. ---- */
struct BanwView {
    const int16_t *mat;
    uint64_t off;
    uint32_t cs;
    int band, o, e;
    /* a stored cell, or (plane 0) an in-band border cell */
    __device__ __forceinline__ int get(int i, int j, int plane) const {
        if (i == 0 || j == 0) return plane == 0 ? banw_border(i, j, o, e) : DPX_NEG;
        if (banw_edge(i, j, band, plane) || !banw_in_band(i, j, band)) return DPX_NEG;
        return (int)mat[off + dpx_band_plane_index(i, j, band, plane, cs)];
    }
};

/* a byte string read back to front through one register: four characters per aligned dword load */
struct CharWin {
    const unsigned char *s;
    uintptr_t at = 1;
    uint32_t w = 0;
    __device__ __forceinline__ int get(int x) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(s + x), al = a & ~(uintptr_t)3;
        if (al != at) { at = al; w = *reinterpret_cast<const uint32_t *>(al); } /* never leaves the 256-byte aligned arena */
        return (int)((w >> (8 * (int)(a & 3))) & 0xFFu);
    }
};

__global__ void k_banw_traceback(const dpx_fill_args a, int numPairs, const int32_t *endRow, const int32_t *endCol, const uint64_t *tbOff,
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
    const BanwView v{a.mat, pr.matOff, pr.chunkStride, band, o, e};
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
            const bool eq = qw.get(i - 1) == rw.get(j - 1);
            const int mm = v.get(i - 1, j - 1, 0) + (eq ? match : mismatch);
            const int D = v.get(i, j, 2), I = v.get(i, j, 1);
            const int vmax = max(D, mm);
            if (I >= vmax) cur = 1;
            else if (D >= mm) cur = 2;
            else { EMIT(rw.get(j - 1), eq ? '*' : '|', qw.get(i - 1)); i--; j--; }
        } else if (cur == 1) {
            const bool open = (j == 1) || (v.get(i, j - 1, 0) + o + e >= v.get(i, j - 1, 1) + e); /* (a border neighbour opens the gap) */
            if (open) cur = 0;
            EMIT(rw.get(j - 1), ' ', '_'); j--;
        } else {
            const bool open = (i == 1) || (v.get(i - 1, j, 0) + o + e >= v.get(i - 1, j, 2) + e);
            if (open) cur = 0;
            EMIT('_', ' ', qw.get(i - 1)); i--;
        }
    }
    while (i > 0) { EMIT('_', ' ', qw.get(i - 1)); i--; }  /* column-0 border: QUERY_DELETION */
    while (j > 0) { EMIT(rw.get(j - 1), ' ', '_'); j--; }  /* row-0 border: QUERY_INSERTION */
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
 * Wave-cooperative traceback: k_traceback_wave's scheme (dpx_kernels.hip) for the three band-layout planes.  One WAVE owns a pair; lane c
 * fetches column cLo + c of a window of 48 rows x 64 columns of H, I and D around the walker into LDS (one 112-byte line per column and
 * plane; in-band border cells carry their H, every other cell without storage and every edge I / D is -32768, the window's minus
 * infinity, which cell() turns into DPX_NEG) -- only the three 8-row groups around the walker's diagonal unless the
 * walk left the last window sideways -- and the walk takes RUNS: every lane decides one cell of the line the path would follow next (the
 * walker's diagonal in SCORING, its row in INSERTION, its column in DELETION) and a ballot gives the number of steps the path really
 * follows.  The band layout has no 16-byte column pieces (the rows of a column lie on consecutive anti-diagonals): 2-byte loads through
 * dpx_band_plane_index, as the linear-gap banded walk does.  Unlike k_basw_traceback_wave's window, a cell without storage must not read 0:
 * scores are negative here, and a 0 in I or D would win "I >= max(D, mm)".  After the runs come ANW's two tails (the rest of column 0 as
 * deletions, the rest of row 0 as insertions), written by all lanes at once.
 * ----------------------------------------------------------------------------------------------------- */
struct BanwWin {
    static constexpr int G = 6;             /* row groups of a window */
    static constexpr int GL = 3;            /* row groups of a banded (diagonal-following) window column */
    static constexpr int WR = 8 * G;        /* rows R0+1 .. R0+WR; columns cLo .. cLo+63, one per lane */
    static constexpr int CS = WR + 8;       /* int16 elements between two columns in LDS */
    static constexpr int kBytes = 3 * 64 * CS * 2;
};

__global__ void __launch_bounds__(64) k_banw_traceback_wave(const dpx_fill_args a, int numPairs, const int32_t *endRow, const int32_t *endCol,
                                                            const uint64_t *tbOff, char *tb, int32_t *tbLen) {
    constexpr int G = BanwWin::G, GL = BanwWin::GL, WR = BanwWin::WR, CS = BanwWin::CS;
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
    constexpr uint32_t kNegInf16 = 0x8000u; /* -32768: below every finite value the range check admits */
    int i = __builtin_amdgcn_readfirstlane(endRow[p]), j = __builtin_amdgcn_readfirstlane(endCol[p]);
    int R0 = 1 << 28, cLo = 1 << 28;
    int diag0 = 0;         /* i - j of the cell the window was anchored on */
    bool banded = false;   /* ... and whether only the groups around that diagonal were fetched */
    bool wantFull = false; /* the walk left the last window sideways (a long gap): fetch whole columns next time */
    uint32_t chR = 0u, chQ = 0u; /* reference character of this lane's column; query character of window row `lane` */
    auto stored = [&](const int ii, const int jj) -> bool { return ii <= m && jj <= n && banw_cell_in_band(ii, jj, B); };
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
                    if (stored(ii2, jc)) val = banw_edge(ii2, jc, B, PL0 + pl) ? kNegInf16 : raw[(pl * CNT + gi) * 8 + e];
                    else if (PL0 + pl == 0 && (ii2 == 0 || jc == 0) && ii2 >= 0 && jc >= 0 && ii2 <= m && jc <= n && banw_in_band(ii2, jc, B))
                        val = (uint32_t)banw_border(ii2, jc, g, ext) & 0xFFFFu;
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
    auto cell = [&](const int pl, const int col, const int row) -> int {
        const int v = (int)win[(pl * 64 + col) * CS + row];
        return v == -32768 ? DPX_NEG : v;
    };
    /* number of lanes that continue a run which starts at lane `from` and goes DOWN the lanes while `on` holds (lane 0 is never on) */
    auto run_down = [&](const bool on, const int from) -> int {
        const unsigned long long inv = ~__builtin_amdgcn_ballot_w64(on) << (63 - from);
        return inv ? __builtin_clzll(inv) : 64;
    };
    /* SCORING decision of window cell (rq, cq) (>= 1 each): 0 diagonal, 1 to INSERTION, 2 to DELETION, 3 not a cell (row / column <= 0) */
    auto decide_cell = [&](const int rq, const int cq, const uint32_t rc, int &qcOut) -> uint32_t {
        const int qc = __builtin_amdgcn_ds_bpermute(rq << 2, (int)chQ);
        qcOut = qc;
        const int ii = R0 + 1 + rq, jc = cLo + cq;
        const int dg = cell(0, cq - 1, rq - 1), I = cell(1, cq, rq), D = cell(2, cq, rq);
        const int mm = dg + ((uint32_t)qc == rc ? match : mismatch);
        uint32_t d = I >= max(D, mm) ? 1u : (D >= mm ? 2u : 0u);
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
                }
                continue;
            }
            cur = __builtin_amdgcn_readlane((int)d, c); /* 1: to INSERTION, 2: to DELETION */
            if (cur == 3) break;                         /* (cannot happen: the walker stands on a cell) */
        } else if (cur == 1) {
            /* INSERTION: steps to the left along row i until (and including) the cell where the gap was opened; lane l decides the cell in
             * column l.  The left neighbour in column 0: opened; on the band's lower edge: its I is minus infinity, opened. */
            const int cq = max(lane, 1), jc = cLo + cq;
            const bool opened = !banw_cell_in_band(i, jc - 1, B) || cell(0, cq - 1, r) + g + ext >= cell(1, cq - 1, r) + ext;
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
            const bool opened = !banw_cell_in_band(ii - 1, j, B) || cell(0, c, rq - 1) + g + ext >= cell(2, c, rq - 1) + ext;
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

template <class K>
hipError_t launch_banw_kernel(K kernel, const dpx_fill_args &a, dim3 grid, size_t lds, hipStream_t s) {
    if (lds > 64u * 1024u) { /* opt in to more than the default 64 KiB of dynamic LDS */
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const unsigned wpb = a.wavesPerBlock; /* `lds` is the request of a four-wave workgroup */
    hipLaunchKernelGGL(kernel, grid, dim3(64u * wpb), lds / 4u * wpb, s, a);
    return hipGetLastError();
}

template <int C>
hipError_t launch_banw_C(const dpx_fill_args &a, bool store, dim3 grid, size_t lds, hipStream_t s) {
    const bool pb = ((a.band + 1) & 1) != 0; /* parity of step A = 0 */
    if (pb) return store ? launch_banw_kernel(k_banw_fill<C, true, true>, a, grid, lds, s)
                         : launch_banw_kernel(k_banw_fill<C, true, false>, a, grid, lds, s);
    return store ? launch_banw_kernel(k_banw_fill<C, false, true>, a, grid, lds, s)
                 : launch_banw_kernel(k_banw_fill<C, false, false>, a, grid, lds, s);
}

} // namespace

hipError_t dpx_launch_banw_fill(const dpx_fill_args &a, int C, bool store, size_t ldsBytes, hipStream_t stream) {
    if (a.numPairs <= 0) return hipSuccess;
    const int wavesPerBlock = (int)a.wavesPerBlock;
    dim3 grid((unsigned)((a.numPairs + wavesPerBlock - 1) / wavesPerBlock));
    switch (C) {
    case 1: return launch_banw_C<1>(a, store, grid, ldsBytes, stream);
    case 2: return launch_banw_C<2>(a, store, grid, ldsBytes, stream);
    case 4: return launch_banw_C<4>(a, store, grid, ldsBytes, stream);
    case 8: return launch_banw_C<8>(a, store, grid, ldsBytes, stream);
    default: return hipErrorInvalidValue;
    }
}

hipError_t dpx_launch_banw_export(const int16_t *mat, const dpx_pair_dev &pr, int plane, int band, int gapOpen, int gapExtend, int16_t *out,
                                  hipStream_t stream) {
    const size_t total = (size_t)(pr.m + 1) * (size_t)(pr.n + 1);
    unsigned blocks = (unsigned)((total + 255) / 256);
    if (blocks > 4096u) blocks = 4096u;
    hipLaunchKernelGGL(k_banw_export, dim3(blocks), dim3(256), 0, stream, mat, pr, plane, band, gapOpen, gapExtend, out);
    return hipGetLastError();
}

hipError_t dpx_launch_banw_traceback(const dpx_fill_args &a, int numPairs, int walk, const uint64_t *tbOff, char *tb, int32_t *tbLen,
                                     hipStream_t stream) {
    if (numPairs <= 0) return hipSuccess;
    if (walk == 2) /* one wave per pair with an LDS window */
        hipLaunchKernelGGL(k_banw_traceback_wave, dim3((unsigned)numPairs), dim3(64), (size_t)BanwWin::kBytes, stream, a, numPairs, a.endRow,
                           a.endCol, tbOff, tb, tbLen);
    else
        hipLaunchKernelGGL(k_banw_traceback, dim3((unsigned)((numPairs + 63) / 64)), dim3(64), 0, stream, a, numPairs, a.endRow, a.endCol, tbOff,
                           tb, tbLen);
    return hipGetLastError();
}
