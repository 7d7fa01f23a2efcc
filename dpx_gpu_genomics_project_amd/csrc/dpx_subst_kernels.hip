/*
 * dpx_subst_kernels.hip -- substitution-matrix scoring for DPX_ALGO_BANW and DPX_ALGO_BAXT batches (dpx_batch_set_substitution) for
 * gfx950: the fill and both walks.  The export is BANW's (dpx_launch_banw_export reads stored cells and closed-form borders).
 *
 * Everything but the diagonal term is k_banw_fill's / k_baxt_fill's, value for value: band, borders, recurrence, tie order, schedule,
 * three phases, stores and band layout (see dpx_banw_kernels.hip), BANW's end-cell pick-up when EXT is false and k_baxt_fill's per-slot
 * signed key with its 64-bit wave reduction when EXT is true (see dpx_baxt_kernels.hip).  The diagonal term is
 *       H[i-1][j-1] + s(ref[j-1], qry[i-1]),      s(r, q) = scores[codeOf[r] * alphabet + codeOf[q]]
 * in place of the byte compare.  The host hands over the table with a row stride of 32 (1 KiB of int8, row = reference code, column =
 * query code, unused entries 0) and the 256 bytes of codeOf.  Every wave copies both (1280 bytes) into its own slice of LDS (the waves of a workgroup share nothing and return at different points, so there is no barrier to meet at).  A character
 * is translated ONCE, when it enters the sliding window -- a second LDS read that depends on the wave-uniform one the step does anyway --
 * and the window registers hold codes, not bytes: the query code as it is, the reference code as code << 5.  A cell's score is then one
 * address add and one signed-byte LDS read where the plain kernels have a compare and a select.  The text is produced by the walks from
 * the sequence bytes, so nothing downstream sees the codes.
 *
 * The walks are BANW's two (one lane per pair; one wave per pair with an LDS window) with mm = H_diag + s(r, q); the relation character
 * is still the byte compare.  The one-lane walk reads table and map from global memory (1280 bytes, resident in L1 after the first
 * steps); the wave walk keeps the table in LDS behind its window and translates a lane's two characters when it loads a window.
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

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        unsigned long long o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

/* (score, min row, min column) as one unsigned key; score > 0 */
__device__ __forceinline__ unsigned long long end_key(const int hv, const int i, const int j) {
    return ((unsigned long long)(unsigned)hv << 40) | ((unsigned long long)(0xFFFFFu - (unsigned)i) << 20) |
           (unsigned long long)(0xFFFFFu - (unsigned)j);
}

template <int C, bool EXT>
struct SubstState {
    int prevH[C], prev2H[C]; /* H on anti-diagonals a-1 and a-2 */
    int prevI[C], prevD[C];  /* I and D on anti-diagonal a-1 */
    int qcd[C], rcd[C];      /* query code / reference code << 5 of each slot's cell */
    int key[EXT ? C : 1];    /* EXT: running signed max of (H << 16 | 0xFFFF - A): max score, then earliest step */
    int lim;                 /* B-1 - lane*C: slot c is inside the band on a step of parity p when c + p <= lim */
    int fin;                 /* !EXT: H[m][n], picked up on the last anti-diagonal by the lane that owns its slot */
};

/* banw_step / baxt_step with the table lookup.  INTERIOR: every in-band slot of this anti-diagonal lies inside the matrix, so validity
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

template <int C, bool PB, bool STORE, bool EXT>
__global__ void __launch_bounds__(DPX_FILL_THREADS) k_subst_fill(const dpx_subst_args sa) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const dpx_fill_args &a = sa.f;
    constexpr int G = (C >= 8) ? 1 : 8 / C; /* steps per 16-byte store */
    constexpr int GG = (G < 2) ? 2 : G;     /* steps per loop iteration (parity pattern repeats every 2) */
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int p = blockIdx.x * (int)a.wavesPerBlock + wv;
    if (p >= a.numPairs) return;
    if (a.order) p = a.order[p];
    const dpx_pair_dev pr = a.pairs[p];
    const int n = pr.n, m = pr.m, B = a.band;
    const int o = a.gapOpen, e = a.gapExtend, oe = a.gapOpen + a.gapExtend;
    if (m <= 0 || n <= 0) { /* an empty sequence: no diagonal step, so the table plays no part (k_banw_fill's / k_baxt_fill's cases) */
        if (lane == 0) {
            if constexpr (EXT) {
                const int L = min(max(max(m, n), 0), B - 1);
                const int k = e > 0 ? L : min(L, 1);
                const int v = k > 0 ? o + k * e : 0;
                const bool take = v > 0;
                a.score[p] = take ? v : 0;
                a.endRow[p] = (take && m > 0) ? k : 0;
                a.endCol[p] = (take && m <= 0) ? k : 0;
            } else {
                a.score[p] = (m > 0 || n > 0) ? o + max(m, n) * e : 0; a.endRow[p] = max(m, 0); a.endCol[p] = max(n, 0);
            }
        }
        return;
    }
    const unsigned char *ref = reinterpret_cast<const unsigned char *>(a.seq + pr.refIdx);
    const unsigned char *qry = reinterpret_cast<const unsigned char *>(a.seq + pr.qryIdx);
    /* the wave's LDS slice: [staged query][staged reference][table image]; a.ldsPerWave counts all three */
    unsigned char *my = smem + (size_t)wv * a.ldsPerWave;
    const unsigned char *qL = stage_bytes(my, qry, m, lane, 64);
    const unsigned char *rL = stage_bytes(my + a.ldsRefOff, ref, n, lane, 64);
    unsigned char *img = my + (a.ldsPerWave - (uint32_t)DPX_SUBST_IMAGE_BYTES);
    { /* (both arrays are 16-byte aligned: the host keeps them in one device allocation, the map behind the table) */
        reinterpret_cast<u32x4 *>(img)[lane] = reinterpret_cast<const u32x4 *>(sa.table)[lane];
        if (lane < 16) reinterpret_cast<u32x4 *>(img + DPX_SUBST_TABLE_BYTES)[lane] = reinterpret_cast<const u32x4 *>(sa.codeOf)[lane];
    }
    const signed char *tabL = reinterpret_cast<const signed char *>(img);
    const unsigned char *codeL = img + DPX_SUBST_TABLE_BYTES;

    SubstState<C, EXT> st;
    st.lim = B - 1 - lane * C;
    st.fin = DPX_NEG;
    { /* anti-diagonals a = 1 (prev: the border cells (0, 1) and (1, 0), in band when B >= 2) and a = 0 (prev2: H[0][0] = 0, which
       * shares its slot with cell (1, 1)); the code windows are those of a = 1, the first real step then slides one of them */
        const int p1 = B & 1;
        const int vi0 = (1 + p1 - (B - 1)) >> 1;
        const int vj0 = 1 - vi0;
#pragma unroll
        for (int c = 0; c < C; c++) {
            const int s = lane * C + c;
            st.qcd[c] = codeL[qL[min(max(vi0 + s - 1, 0), m - 1)]];
            st.rcd[c] = (int)codeL[rL[min(max(vj0 - s - 1, 0), n - 1)]] << 5;
            const int bi = vi0 + s; /* the slot's cell on a = 1 is (bi, 1 - bi) */
            st.prevH[c] = (B >= 2 && (bi == 0 || bi == 1)) ? oe : DPX_NEG;
            st.prev2H[c] = (s == ((B - 1) >> 1)) ? 0 : DPX_NEG;
            st.prevI[c] = DPX_NEG;
            st.prevD[c] = DPX_NEG;
            if constexpr (EXT) st.key[c] = 0;
        }
    }
    /* !EXT: the lane and register that own the end cell (m, n) on the last anti-diagonal */
    const int sEnd = (m - n + B - 1) >> 1;
    const int cEnd = (!EXT && lane == sEnd / C) ? (sEnd % C) : -1;
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
#define DPX_SUBST_STORE(grp_)                                                                                             \
    {                                                                                                                     \
        int16_t *at_ = Hp + (size_t)(grp_) * cs;                                                                          \
        store8(at_, accH);                                                                                                \
        store8(at_ + DPX_BAND_PLANE_ELEMS, accI);                                                                         \
        store8(at_ + 2 * DPX_BAND_PLANE_ELEMS, accD);                                                                     \
    }
#define DPX_SUBST_BODY(INTERIOR_)                                                                                         \
    _Pragma("unroll") for (int g = 0; g < GG; g += 2) {                                                                  \
        subst_step<C, PB, INTERIOR_, EXT>(st, A0 + g, i0, j0, lane, m, n, B, o, oe, e, cEnd, qL, rL, tabL, codeL,         \
                                          &accH[(g % G) * C], &accI[(g % G) * C], &accD[(g % G) * C]);                    \
        if constexpr (STORE && G == 1) {                                                                                  \
            if (INTERIOR_ || A0 + g < numGroups) DPX_SUBST_STORE(A0 + g)                                                  \
        }                                                                                                                 \
        subst_step<C, !PB, INTERIOR_, EXT>(st, A0 + g + 1, i0, j0, lane, m, n, B, o, oe, e, cEnd, qL, rL, tabL, codeL,    \
                                           &accH[((g + 1) % G) * C], &accI[((g + 1) % G) * C], &accD[((g + 1) % G) * C]); \
        if constexpr (STORE) {                                                                                            \
            if (((g + 1) % G) == G - 1) {                                                                                 \
                const int grp = (A0 + g + 1) / G;                                                                         \
                if (INTERIOR_ || grp < numGroups) DPX_SUBST_STORE(grp)                                                    \
            }                                                                                                             \
        }                                                                                                                 \
    }
    /* parity of step A is (A + B + 1) & 1; A0 is even, so even steps have parity PB and odd steps !PB.
     * Three phases: head (some slots outside the matrix, border slots), interior, tail.  !EXT: the interior loop stops short of the last
     * anti-diagonal (A = NS-1), so the end cell is always picked up by the general step.  EXT: no end cell has to be caught, the
     * interior loop runs up to the last anti-diagonal; steps past NS - 1 (the rest of the last group) hold no cell. */
    int A0 = 0;
    for (; A0 < NS && !(interior(A0) && interior(A0 + GG - 1)); A0 += GG) { DPX_SUBST_BODY(false) }
    for (; A0 + GG < NS + (EXT ? 1 : 0) && interior(A0 + GG - 1); A0 += GG) { DPX_SUBST_BODY(true) }
    for (; A0 < NS; A0 += GG) { DPX_SUBST_BODY(false) }
#undef DPX_SUBST_BODY
#undef DPX_SUBST_STORE
    if constexpr (!EXT) {
        if (cEnd >= 0) { a.score[p] = st.fin; a.endRow[p] = m; a.endCol[p] = n; }
    } else {
        /* candidates: every slot's first maximum (within a slot cells arrive in row-major order); across slots max score, min row, min
         * col.  A border slot decodes to i = 0 or j = 0.  (0, 1) and (1, 0) need no candidate: see the end of k_baxt_fill. */
        unsigned long long mine = 0ull;
#pragma unroll
        for (int c = 0; c < C; c++) {
            const int hv = st.key[c] >> 16;
            if (hv > 0) {
                const int A = 0xFFFF - (st.key[c] & 0xFFFF);
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
        if (lane == 0) {
            const int hv = (int)(top >> 40);
            a.score[p] = hv;
            a.endRow[p] = hv > 0 ? (int)(0xFFFFFu - (unsigned)((top >> 20) & 0xFFFFFu)) : 0;
            a.endCol[p] = hv > 0 ? (int)(0xFFFFFu - (unsigned)(top & 0xFFFFFu)) : 0;
        }
    }
}

/* ---- geometry of the walks (dpx_banw_kernels.hip shares it with its export).  A cell (i, j), borders included, is in the band when |i - j| <= B-1; the fill stores
 * the in-band cells with i, j >= 1; I on the lower edge and D on the upper edge are -infinity whatever the fill stored there ---- */
__device__ __forceinline__ bool sb_in_band(const int i, const int j, const int band) {
    const int dlt = i - j;
    return dlt <= band - 1 && -dlt <= band - 1;
}
__device__ __forceinline__ bool sb_cell_in_band(const int i, const int j, const int band) { /* ... and has storage */
    return i >= 1 && j >= 1 && sb_in_band(i, j, band);
}
/* H of the in-band border cell (i, j), i == 0 or j == 0 */
__device__ __forceinline__ int sb_border(const int i, const int j, const int o, const int e) { return (i | j) == 0 ? 0 : o + (i + j) * e; }
/* is `plane` of the stored cell (i, j) minus infinity? */
__device__ __forceinline__ bool sb_edge(const int i, const int j, const int band, const int plane) {
    return (plane == 1 && i - j == band - 1) || (plane == 2 && j - i == band - 1);
}

/* ---- traceback: one lane per pair, ANW's three-state walk (dpx_kernels.hip: tb_walk_lane) over the band layout, with ANW's two tails.
 * The walk stands on stored cells only; the neighbours it reads are in band (the diagonal one always; the left / upper one because the
 * gap it came through is finite) or border cells, which open the gap. ---- */
struct SubstView {
    const int16_t *mat;
    uint64_t off;
    uint32_t cs;
    int band, o, e;
    /* a stored cell, or (plane 0) an in-band border cell */
    __device__ __forceinline__ int get(int i, int j, int plane) const {
        if (i == 0 || j == 0) return plane == 0 ? sb_border(i, j, o, e) : DPX_NEG;
        if (sb_edge(i, j, band, plane) || !sb_in_band(i, j, band)) return DPX_NEG;
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

__global__ void k_subst_traceback(const dpx_subst_args sa, int numPairs, const int32_t *endRow, const int32_t *endCol,
                                  const uint64_t *tbOff, char *tb, int32_t *tbLen) {
    const dpx_fill_args &a = sa.f;
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
    const signed char *tab = reinterpret_cast<const signed char *>(sa.table);
    const unsigned char *code = sa.codeOf;
    const SubstView v{a.mat, pr.matOff, pr.chunkStride, band, o, e};
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
            const int qc = qw.get(i - 1), rc = rw.get(j - 1);
            const bool eq = qc == rc; /* the relation character stays the byte compare */
            const int mm = v.get(i - 1, j - 1, 0) + (int)tab[((int)code[rc] << 5) + (int)code[qc]];
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
struct SubstWin {
    static constexpr int G = 6;             /* row groups of a window */
    static constexpr int GL = 3;            /* row groups of a banded (diagonal-following) window column */
    static constexpr int WR = 8 * G;        /* rows R0+1 .. R0+WR; columns cLo .. cLo+63, one per lane */
    static constexpr int CS = WR + 8;       /* int16 elements between two columns in LDS */
    static constexpr int kBytes = 3 * 64 * CS * 2;
};

__global__ void __launch_bounds__(64) k_subst_traceback_wave(const dpx_subst_args sa, int numPairs, const int32_t *endRow, const int32_t *endCol,
                                                             const uint64_t *tbOff, char *tb, int32_t *tbLen) {
    const dpx_fill_args &a = sa.f;
    constexpr int G = SubstWin::G, GL = SubstWin::GL, WR = SubstWin::WR, CS = SubstWin::CS;
    extern __shared__ __attribute__((aligned(16))) unsigned char smemTb[];
    int16_t *win = reinterpret_cast<int16_t *>(smemTb); /* win[(plane * 64 + (jj - cLo)) * CS + (ii - R0 - 1)] = plane[ii][jj] */
    const signed char *tabL = reinterpret_cast<const signed char *>(smemTb + SubstWin::kBytes); /* the table, behind the window */
    const unsigned char *code = sa.codeOf;
    const int p = blockIdx.x;
    const int lane = threadIdx.x;
    if (p >= numPairs) return;
    reinterpret_cast<u32x4 *>(smemTb + SubstWin::kBytes)[lane] = reinterpret_cast<const u32x4 *>(sa.table)[lane]; /* 64 x 16 B = the 1-KiB table; load_window's fences order it before the first read */
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
    uint32_t chR = 0u, chQ = 0u; /* reference character of this lane's column; query character of window row `lane` (its code in bits 8..) */
    uint32_t cdR = 0u;           /* code << 5 of chR */
    auto stored = [&](const int ii, const int jj) -> bool { return ii <= m && jj <= n && sb_cell_in_band(ii, jj, B); };
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
                    if (stored(ii2, jc)) val = sb_edge(ii2, jc, B, PL0 + pl) ? kNegInf16 : raw[(pl * CNT + gi) * 8 + e];
                    else if (PL0 + pl == 0 && (ii2 == 0 || jc == 0) && ii2 >= 0 && jc >= 0 && ii2 <= m && jc <= n && sb_in_band(ii2, jc, B))
                        val = (uint32_t)sb_border(ii2, jc, g, ext) & 0xFFFFu;
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
        chR = okR ? rr : 0u;
        cdR = (uint32_t)code[chR] << 5; /* the lane's two characters are translated here, once per window */
        chQ = okQ ? rq : 0u;
        chQ |= (uint32_t)code[chQ] << 8;
        asm volatile("" : "+v"(chQ), "+v"(chR), "+v"(cdR)); /* the two characters are waited for here, not in every trip of the walk */
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
    auto decide_cell = [&](const int rq, const int cq, int &qcOut) -> uint32_t {
        const int qpk = __builtin_amdgcn_ds_bpermute(rq << 2, (int)chQ); /* byte | code << 8 */
        qcOut = qpk & 0xFF;
        const int ii = R0 + 1 + rq, jc = cLo + cq;
        const int dg = cell(0, cq - 1, rq - 1), I = cell(1, cq, rq), D = cell(2, cq, rq);
        const int mm = dg + (int)tabL[(int)cdR + (qpk >> 8)];
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
        const int qc = __builtin_amdgcn_ds_bpermute(max(r - lane, 0) << 2, (int)chQ) & 0xFF;
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
            const bool opened = !sb_cell_in_band(i, jc - 1, B) || cell(0, cq - 1, r) + g + ext >= cell(1, cq - 1, r) + ext;
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
            const bool opened = !sb_cell_in_band(ii - 1, j, B) || cell(0, c, rq - 1) + g + ext >= cell(2, c, rq - 1) + ext;
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
hipError_t launch_subst_kernel(K kernel, const dpx_subst_args &a, dim3 grid, size_t lds, hipStream_t s) {
    if (lds > 64u * 1024u) { /* opt in to more than the default 64 KiB of dynamic LDS */
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const unsigned wpb = a.f.wavesPerBlock; /* `lds` is the request of a four-wave workgroup */
    hipLaunchKernelGGL(kernel, grid, dim3(64u * wpb), lds / 4u * wpb, s, a);
    return hipGetLastError();
}

template <int C, bool EXT>
hipError_t launch_subst_C(const dpx_subst_args &a, bool store, dim3 grid, size_t lds, hipStream_t s) {
    const bool pb = ((a.f.band + 1) & 1) != 0; /* parity of step A = 0 */
    if (pb) return store ? launch_subst_kernel(k_subst_fill<C, true, true, EXT>, a, grid, lds, s)
                         : launch_subst_kernel(k_subst_fill<C, true, false, EXT>, a, grid, lds, s);
    return store ? launch_subst_kernel(k_subst_fill<C, false, true, EXT>, a, grid, lds, s)
                 : launch_subst_kernel(k_subst_fill<C, false, false, EXT>, a, grid, lds, s);
}

template <bool EXT>
hipError_t launch_subst_E(const dpx_subst_args &a, int C, bool store, dim3 grid, size_t lds, hipStream_t s) {
    switch (C) {
    case 1: return launch_subst_C<1, EXT>(a, store, grid, lds, s);
    case 2: return launch_subst_C<2, EXT>(a, store, grid, lds, s);
    case 4: return launch_subst_C<4, EXT>(a, store, grid, lds, s);
    case 8: return launch_subst_C<8, EXT>(a, store, grid, lds, s);
    default: return hipErrorInvalidValue;
    }
}

} // namespace

hipError_t dpx_launch_subst_fill(const dpx_subst_args &a, int C, bool store, bool ext, size_t ldsBytes, hipStream_t stream) {
    if (a.f.numPairs <= 0) return hipSuccess;
    const int wavesPerBlock = (int)a.f.wavesPerBlock;
    dim3 grid((unsigned)((a.f.numPairs + wavesPerBlock - 1) / wavesPerBlock));
    return ext ? launch_subst_E<true>(a, C, store, grid, ldsBytes, stream) : launch_subst_E<false>(a, C, store, grid, ldsBytes, stream);
}

hipError_t dpx_launch_subst_traceback(const dpx_subst_args &a, int numPairs, int walk, const uint64_t *tbOff, char *tb, int32_t *tbLen,
                                      hipStream_t stream) {
    if (numPairs <= 0) return hipSuccess;
    if (walk == 2) /* one wave per pair with an LDS window, the table behind it */
        hipLaunchKernelGGL(k_subst_traceback_wave, dim3((unsigned)numPairs), dim3(64), (size_t)SubstWin::kBytes + DPX_SUBST_TABLE_BYTES, stream, a,
                           numPairs, a.f.endRow, a.f.endCol, tbOff, tb, tbLen);
    else
        hipLaunchKernelGGL(k_subst_traceback, dim3((unsigned)((numPairs + 63) / 64)), dim3(64), 0, stream, a, numPairs, a.f.endRow, a.f.endCol,
                           tbOff, tb, tbLen);
    return hipGetLastError();
}
