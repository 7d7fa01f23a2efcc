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
 * The helpers, the band geometry and both walks (band_walk_lane, band_walk_wave under ByteScorer) are dpx_band_affine.hpp's, which also
 * says why the step is not.
 *
 * Stores: three planes in the band layout of dpx_layout.h (dpx_band_plane_index), every lane writes 16 contiguous bytes per plane and
 * store.  I of a cell on the band's lower edge (i - j = B-1) and D of a cell on its upper edge (j - i = B-1) are -infinity; what the
 * fill stores there (the low half of DPX_NEG + a weight) is NEVER READ: the export and both walks know these cells from the geometry
 * alone and substitute -infinity, so the fill pays nothing for them.  Every other in-band value is finite and fits int16 whenever the
 * host's range check passed; slots that hold no cell are written but never read.
 */
#include "dpx_band_affine.hpp"

namespace {

using namespace dpx_band;

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

/* one pair's plane as the row-major (m+1) x (n+1) matrix: 0 outside the band; in-band borders carry H = o + k * e and I = D = 0 (as ANW
 * exports them); an in-band I or D that is -infinity exports as -32768 */
__global__ void k_banw_export(const int16_t *mat, dpx_pair_dev pr, int plane, int band, int o, int e, int16_t *out) {
    const int n = pr.n, m = pr.m;
    const size_t total = (size_t)(m + 1) * (size_t)(n + 1);
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int i = (int)(idx / (size_t)(n + 1));
        const int j = (int)(idx % (size_t)(n + 1));
        int v = 0;
        if (in_band(i, j, band)) {
            if (i == 0 || j == 0) v = plane == 0 ? border(i, j, o, e) : 0;
            else if (edge(i, j, band, plane)) v = -32768;
            else v = mat[pr.matOff + dpx_band_plane_index(i, j, band, plane, pr.chunkStride)];
        }
        out[idx] = (int16_t)v;
    }
}

__global__ void k_banw_traceback(const dpx_fill_args a, int numPairs, const int32_t *endRow, const int32_t *endCol, const uint64_t *tbOff,
                                 char *tb, int32_t *tbLen) {
    band_walk_lane(a, ByteScorer{a.match, a.mismatch}, numPairs, endRow, endCol, tbOff, tb, tbLen);
}

__global__ void __launch_bounds__(64) k_banw_traceback_wave(const dpx_fill_args a, int numPairs, const int32_t *endRow, const int32_t *endCol,
                                                            const uint64_t *tbOff, char *tb, int32_t *tbLen) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smemTb[];
    band_walk_wave(a, ByteScorer{a.match, a.mismatch}, nullptr, smemTb, numPairs, endRow, endCol, tbOff, tb, tbLen);
}

} // namespace

hipError_t dpx_launch_banw_fill(const dpx_fill_args &a, int C, bool store, size_t ldsBytes, hipStream_t stream) {
    if (a.numPairs <= 0) return hipSuccess;
    return dispatch_fill(C, a.band, store, [&](auto c, auto pb, auto st) {
        return launch_fill(k_banw_fill<decltype(c)::value, decltype(pb)::value, decltype(st)::value>, a, a, ldsBytes, stream);
    });
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
        hipLaunchKernelGGL(k_banw_traceback_wave, dim3((unsigned)numPairs), dim3(64), (size_t)BandWin::kBytes, stream, a, numPairs, a.endRow,
                           a.endCol, tbOff, tb, tbLen);
    else
        hipLaunchKernelGGL(k_banw_traceback, dim3((unsigned)((numPairs + 63) / 64)), dim3(64), 0, stream, a, numPairs, a.endRow, a.endCol, tbOff,
                           tb, tbLen);
    return hipGetLastError();
}
