/*
 * dpx_zext_kernels.hip -- DPX_ALGO_BAXT in extension mode (dpx_batch_set_extension) for gfx950: the fill with z-drop termination, the
 * best score that reaches the end of the query, and the end-bonus choice between the two.  Export and both walks stay BANW's
 * (dpx_banw_kernels.hip); the host masks the exported planes behind the pair's last anti-diagonal.
 *
 * The step is k_baxt_fill's, the same function (dpx_band_affine.hpp: slot_key_step): schedule (anti-diagonals a = i+j, slot s = (i-j+B-1)>>1, lane l owns
 * the C slots [l*C, l*C+C)), staging, the three phases, the 16-byte stores of three planes and the per-slot signed key
 * (H << 16 | 0xFFFF - step) that finds the first row-major maximum.  On step A (anti-diagonal a = A + 2) slot s holds the cell
 * (i0 + s, j0 - s).  Added to the state:
 *
 *   row-m key   The cell of row m on anti-diagonal a is (m, a - m), in slot m - i0; it exists when 0 <= a - m <= n and |2m - a| <= B-1,
 *               both wave-uniform, so the pick-up sits behind a scalar branch that at most 2B-1 steps take: one v_readlane of the
 *               slot's H and a scalar max(H << 16 | 0xFFFF - (a - 1)), the maximum of H[m][.] at the smallest column.  "None" is
 *               INT_MIN, which no cell produces (a - 1 <= 64999 leaves the low half above 0).
 *   ZDROP only  best, bi, bj (wave-uniform).  Per step every lane takes the maximum over its slots of (max(H, -32768) << 16 |
 *               0xFFFF - row), a DPP reduction brings the wave's maximum to lane 63 -- the anti-diagonal's maximum at its smallest
 *               row; in-band cells are >= -32767 by the range check, so -32768 in the top half means "no cell on this anti-diagonal"
 *               -- and one scalar update-or-drop test follows.  Border cells take part (the key is taken after the border select).
 *               Anti-diagonal 1, the border cells (0, 1) and (1, 0) that no step visits, is tested before the loop.
 *
 * On a drop the wave leaves the loop, stores its partial group (the steps of the group it did not run keep the previous group's
 * values, or zeros: they lie behind lastDiag and the host never shows them), writes its results and returns; the waves of a workgroup
 * share no barrier.  Nothing is stored past the pair's last chunk: a dropped pair stores a prefix of what k_baxt_fill stores.
 *
 * The scan's pieces (wave_max_i32, zdrop_test, write_results, the border-line scan of an empty sequence, the after-step and the final
 * reduction) live in dpx_band_affine.hpp: k_zsub_fill (dpx_zsub_kernels.hip) runs the same text under a substitution table.
 */
#include "dpx_band_affine.hpp"

namespace {

using namespace dpx_band;

template <int C, bool PB, bool STORE, bool ZDROP>
__global__ void __launch_bounds__(DPX_FILL_THREADS) k_zext_fill(const dpx_zext_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int G = (C >= 8) ? 1 : 8 / C; /* steps per 16-byte store */
    constexpr int GG = (G < 2) ? 2 : G;     /* steps per loop iteration (parity pattern repeats every 2) */
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int p = blockIdx.x * (int)a.f.wavesPerBlock + wv;
    if (p >= a.f.numPairs) return;
    if (a.f.order) p = a.f.order[p];
    const dpx_pair_dev pr = a.f.pairs[p];
    const int n = pr.n, m = pr.m, B = a.f.band;
    const int match = a.f.match, mismatch = a.f.mismatch, o = a.f.gapOpen, e = a.f.gapExtend, oe = a.f.gapOpen + a.f.gapExtend;
    const int Z = a.scan.zdrop, pen = e < 0 ? -e : 0;
    if (m <= 0 || n <= 0) {
        if (lane == 0) scan_border_line<ZDROP>(a.f, a.scan.endBonus, a.scan.ext, p, m, n, B, [&](const int k) { return o + k * e; }, Z, pen); /* an empty sequence: one border line */
        return;
    }
    const unsigned char *ref = reinterpret_cast<const unsigned char *>(a.f.seq + pr.refIdx);
    const unsigned char *qry = reinterpret_cast<const unsigned char *>(a.f.seq + pr.qryIdx);
    unsigned char *my = smem + (size_t)wv * a.f.ldsPerWave;
    const unsigned char *qL = stage_bytes(my, qry, m, lane, 64);
    const unsigned char *rL = stage_bytes(my + a.f.ldsRefOff, ref, n, lane, 64);

    SlotKeyState<C> st;
    st.lim = B - 1 - lane * C;
    /* (1, 0), the only cell of row m that no step visits: in band when B >= 2, on anti-diagonal 1 */
    int qe = (m == 1 && B >= 2) ? (int)(((unsigned)oe << 16) | 0xFFFFu) : INT_MIN;
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
    int16_t *Hp = a.f.mat + pr.matOff + (size_t)lane * 8u;
    const size_t cs = pr.chunkStride;
    int accH[8] = {}, accI[8] = {}, accD[8] = {}; /* (zeros: a drop inside the first group stores all eight steps of it) */
    int i0 = (1 + (B & 1) - (B - 1)) >> 1;
    int j0 = 1 - i0;
    /* the scan's state; anti-diagonal 1 is non-empty when B >= 2, its maximum o + e sits at its smallest row, (0, 1) */
    int best = 0, bi = 0, bj = 0, lastDiag = m + n;
    bool stop = false;
    if constexpr (ZDROP) {
        if (B >= 2 && zdrop_test(oe, 0, 1, Z, pen, best, bi, bj)) {
            lastDiag = 1;
            stop = true;
        }
    }
#define DPX_ZEXT_STORE(grp_)                                                                                              \
    {                                                                                                                     \
        int16_t *at_ = Hp + (size_t)(grp_) * cs;                                                                          \
        store8(at_, accH);                                                                                                \
        store8(at_ + DPX_BAND_PLANE_ELEMS, accI);                                                                         \
        store8(at_ + 2 * DPX_BAND_PLANE_ELEMS, accD);                                                                     \
    }
    /* after step A_ (i0, j0 are the step's): the row-m pick-up, then the anti-diagonal's maximum and the drop test */
#define DPX_ZEXT_AFTER(A_, h_) DPX_BAND_SCAN_AFTER(A_, h_)
#define DPX_ZEXT_BODY(INTERIOR_)                                                                                          \
    _Pragma("unroll") for (int g = 0; g < GG; g += 2) {                                                                  \
        slot_key_step<C, PB, INTERIOR_>(st, A0 + g, i0, j0, lane, m, n, B, match, mismatch, o, oe, e, qL, rL,             \
                                    &accH[(g % G) * C], &accI[(g % G) * C], &accD[(g % G) * C]);                          \
        DPX_ZEXT_AFTER(A0 + g, &accH[(g % G) * C])                                                                        \
        if constexpr (STORE && G == 1) {                                                                                  \
            if (INTERIOR_ || A0 + g < numGroups) DPX_ZEXT_STORE(A0 + g)                                                   \
        }                                                                                                                 \
        if (stop) break;                                                                                                  \
        slot_key_step<C, !PB, INTERIOR_>(st, A0 + g + 1, i0, j0, lane, m, n, B, match, mismatch, o, oe, e, qL, rL,        \
                                     &accH[((g + 1) % G) * C], &accI[((g + 1) % G) * C], &accD[((g + 1) % G) * C]);       \
        DPX_ZEXT_AFTER(A0 + g + 1, &accH[((g + 1) % G) * C])                                                              \
        if constexpr (STORE) {                                                                                            \
            if (((g + 1) % G) == G - 1) {                                                                                 \
                const int grp = (A0 + g + 1) / G;                                                                         \
                if (INTERIOR_ || grp < numGroups) DPX_ZEXT_STORE(grp)                                                     \
            }                                                                                                             \
        }                                                                                                                 \
        if (stop) break;                                                                                                  \
    }
    /* parity of step A is (A + B + 1) & 1; A0 is even, so even steps have parity PB and odd steps !PB.  Three phases as in k_baxt_fill:
     * head (some slots outside the matrix, border slots), interior, tail; each ends early on a drop. */
    int A0 = 0;
    for (; !stop && A0 < NS && !(interior(A0) && interior(A0 + GG - 1)); A0 += GG) { DPX_ZEXT_BODY(false) }
    for (; !stop && A0 + GG <= NS && interior(A0 + GG - 1); A0 += GG) { DPX_ZEXT_BODY(true) }
    for (; !stop && A0 < NS; A0 += GG) { DPX_ZEXT_BODY(false) }
    if constexpr (ZDROP && STORE && G > 1) {
        /* a drop on a step that does not close its store group: the group goes out as it stands (lastDiag >= 2 here means a step ran) */
        if (stop && lastDiag >= 2 && ((lastDiag - 2) % G) != G - 1) {
            const int grp = (lastDiag - 2) / G;
            if (grp < numGroups) DPX_ZEXT_STORE(grp)
        }
    }
#undef DPX_ZEXT_BODY
#undef DPX_ZEXT_AFTER
#undef DPX_ZEXT_STORE
    scan_finish<C>(a.f, a.scan.endBonus, a.scan.ext, p, st.key, lane, m, B, qe, lastDiag, stop);
}

} // namespace

hipError_t dpx_launch_zext_fill(const dpx_zext_args &a, int C, bool store, size_t ldsBytes, hipStream_t stream) {
    if (a.f.numPairs <= 0) return hipSuccess;
    if (!a.scan.ext) return hipErrorInvalidValue;
    return dispatch_fill(C, a.f.band, store, [&](auto c, auto pb, auto st) {
        constexpr int kC = decltype(c)::value;
        constexpr bool kPB = decltype(pb)::value, kStore = decltype(st)::value;
        return a.scan.zdrop >= 0 ? launch_fill(k_zext_fill<kC, kPB, kStore, true>, a, a.f, ldsBytes, stream)
                            : launch_fill(k_zext_fill<kC, kPB, kStore, false>, a, a.f, ldsBytes, stream);
    });
}
