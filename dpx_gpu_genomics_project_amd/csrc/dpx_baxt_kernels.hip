/*
 * dpx_baxt_kernels.hip -- banded affine-gap extension alignment (DPX_ALGO_BAXT) for gfx950: the fill.  Export and both walks are BANW's
 * (dpx_banw_kernels.hip: dpx_launch_banw_export, dpx_launch_banw_traceback), which read the same stored layout under the same edge and
 * border rules and start from endRow / endCol.
 *
 * The cells are BANW's, value for value: ANW's Gotoh recurrence restricted to the band |i-j| <= B-1, border cells included, H[0][0] = 0,
 * in-band border cells H = gapOpen + k * gapExtend, -infinity (DPX_NEG) outside the band, no zero floor.  What differs is the result: the
 * alignment is anchored at (0, 0) and ends where H peaks -- the score is the maximum of H over ALL in-band cells, the border cells and
 * (0, 0) included (so it is >= 0), and the end cell is the first cell in row-major order that holds it.  There is no admission rule:
 * when |m - n| >= B the corner (m, n) is simply never reached.
 *
 * The step is dpx_band_affine.hpp's slot_key_step, which k_zext_fill runs too.  Schedule, stores and the three phases are k_banw_fill's (anti-diagonals a = i+j, slot s = (i-j+B-1)>>1, lane l owns the C = ceil(B/64)
 * slots [l*C, l*C+C), two values per step by DPP, border slots hand on o + a*e in the head phase, 16-byte stores of three planes in the
 * band layout of dpx_layout.h).  In place of BANW's end-cell pick-up every slot keeps k_basw_fill's running key (score << 16 | 0xFFFF -
 * step): a slot sees the cells of its two diagonals in row order -- border slots too -- so the first maximum of a slot is its first
 * maximum in row-major order, and a 64-bit (score, min row, min column) wave reduction finds the first one over all slots.  The key is
 * taken AFTER the border select, which covers the border cells of anti-diagonals a >= 2; the two border cells of a = 1, (0, 1) and (1, 0),
 * precede the first step and can never hold the maximum (see the end of k_baxt_fill).  (0, 0) is no candidate: it is the "nothing
 * above 0" case.
 *
 * The key is a SIGNED int: (h << 16) | (0xFFFF - A) orders by h, then by the earlier step, under a signed compare for every
 * -32768 <= h <= 32767, which the host's range check guarantees for an in-band cell; a slot without a cell carries DPX_NEG = -2^29, whose
 * low 16 bits are 0, so it enters as score 0.  Only a cell with H > 0 can displace (0, 0), so scores <= 0 need not be told apart, and the
 * signed form saves the max(h, 0) of the unsigned one.
 */
#include "dpx_band_affine.hpp"

namespace {

using namespace dpx_band;

template <int C, bool PB, bool STORE>
__global__ void __launch_bounds__(DPX_FILL_THREADS) k_baxt_fill(const dpx_fill_args a) {
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
    if (m <= 0 || n <= 0) {
        /* an empty sequence: the in-band cells are one border line, H = o + k*e for 1 <= k <= L = min(max(m, n), B-1) and 0 at k = 0.
         * Linear in k: the first maximum is at k = L when e > 0 and at k = 1 otherwise; it counts when it is above the 0 of (0, 0) */
        if (lane == 0) {
            const int L = min(max(max(m, n), 0), B - 1);
            const int k = e > 0 ? L : min(L, 1);
            const int v = k > 0 ? o + k * e : 0;
            const bool take = v > 0;
            a.score[p] = take ? v : 0;
            a.endRow[p] = (take && m > 0) ? k : 0;
            a.endCol[p] = (take && m <= 0) ? k : 0;
        }
        return;
    }
    const unsigned char *ref = reinterpret_cast<const unsigned char *>(a.seq + pr.refIdx);
    const unsigned char *qry = reinterpret_cast<const unsigned char *>(a.seq + pr.qryIdx);
    unsigned char *my = smem + (size_t)wv * a.ldsPerWave;
    const unsigned char *qL = stage_bytes(my, qry, m, lane, 64);
    const unsigned char *rL = stage_bytes(my + a.ldsRefOff, ref, n, lane, 64);

    SlotKeyState<C> st;
    st.lim = B - 1 - lane * C;
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
            st.key[c] = 0;
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
#define DPX_BAXT_STORE(grp_)                                                                                              \
    {                                                                                                                     \
        int16_t *at_ = Hp + (size_t)(grp_) * cs;                                                                          \
        store8(at_, accH);                                                                                                \
        store8(at_ + DPX_BAND_PLANE_ELEMS, accI);                                                                         \
        store8(at_ + 2 * DPX_BAND_PLANE_ELEMS, accD);                                                                     \
    }
#define DPX_BAXT_BODY(INTERIOR_)                                                                                          \
    _Pragma("unroll") for (int g = 0; g < GG; g += 2) {                                                                  \
        slot_key_step<C, PB, INTERIOR_>(st, A0 + g, i0, j0, lane, m, n, B, match, mismatch, o, oe, e, qL, rL,             \
                                    &accH[(g % G) * C], &accI[(g % G) * C], &accD[(g % G) * C]);                          \
        if constexpr (STORE && G == 1) {                                                                                  \
            if (INTERIOR_ || A0 + g < numGroups) DPX_BAXT_STORE(A0 + g)                                                   \
        }                                                                                                                 \
        slot_key_step<C, !PB, INTERIOR_>(st, A0 + g + 1, i0, j0, lane, m, n, B, match, mismatch, o, oe, e, qL, rL,        \
                                     &accH[((g + 1) % G) * C], &accI[((g + 1) % G) * C], &accD[((g + 1) % G) * C]);       \
        if constexpr (STORE) {                                                                                            \
            if (((g + 1) % G) == G - 1) {                                                                                 \
                const int grp = (A0 + g + 1) / G;                                                                         \
                if (INTERIOR_ || grp < numGroups) DPX_BAXT_STORE(grp)                                                     \
            }                                                                                                             \
        }                                                                                                                 \
    }
    /* parity of step A is (A + B + 1) & 1; A0 is even, so even steps have parity PB and odd steps !PB.
     * Three phases: head (some slots outside the matrix, border slots), interior, tail.  No end cell has to be caught, so the interior
     * loop runs up to the last anti-diagonal as k_basw_fill's does.  Steps past NS - 1 (the rest of the last group) hold no cell. */
    int A0 = 0;
    for (; A0 < NS && !(interior(A0) && interior(A0 + GG - 1)); A0 += GG) { DPX_BAXT_BODY(false) }
    for (; A0 + GG <= NS && interior(A0 + GG - 1); A0 += GG) { DPX_BAXT_BODY(true) }
    for (; A0 < NS; A0 += GG) { DPX_BAXT_BODY(false) }
#undef DPX_BAXT_BODY
#undef DPX_BAXT_STORE
    /* candidates: every slot's first maximum (within a slot cells arrive in row-major order); across slots max score, min row, min col.
     * A border slot decodes to i = 0 or j = 0. */
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
    /* The border cells of anti-diagonal 1, (0, 1) and (1, 0), which no step visits, need no candidate: they are in band when B >= 2 and
     * hold o + e, which counts only when it is above 0; but then (1, 1) -- a cell of this matrix, m and n are >= 1 here -- holds
     * H >= D = H[0][1] + o + e = 2 * (o + e) > o + e. */
    const unsigned long long top = wave_max_u64(mine);
    if (lane == 0) {
        const int hv = (int)(top >> 40);
        a.score[p] = hv;
        a.endRow[p] = hv > 0 ? (int)(0xFFFFFu - (unsigned)((top >> 20) & 0xFFFFFu)) : 0;
        a.endCol[p] = hv > 0 ? (int)(0xFFFFFu - (unsigned)(top & 0xFFFFFu)) : 0;
    }
}

} // namespace

hipError_t dpx_launch_baxt_fill(const dpx_fill_args &a, int C, bool store, size_t ldsBytes, hipStream_t stream) {
    if (a.numPairs <= 0) return hipSuccess;
    return dispatch_fill(C, a.band, store, [&](auto c, auto pb, auto st) {
        return launch_fill(k_baxt_fill<decltype(c)::value, decltype(pb)::value, decltype(st)::value>, a, a, ldsBytes, stream);
    });
}
