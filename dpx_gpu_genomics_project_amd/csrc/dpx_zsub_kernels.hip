/*
 * dpx_zsub_kernels.hip -- DPX_ALGO_BAXT in extension mode under a substitution table (dpx_batch_set_extension_table) for gfx950: the fill,
 * k_zsub_fill, and nothing else.  The walks are dpx_subst_kernels.hip's two (a walk from a computed cell only visits earlier
 * anti-diagonals), the export is BANW's, and the host masks the exported planes behind the pair's last anti-diagonal.
 *
 * The kernel is k_subst_fill<..., EXT = true>'s step with k_zext_fill's state and after-step, and every piece is the text those two
 * kernels run (dpx_band_affine.hpp):
 *   subst_step        table and byte map in the wave's LDS slice, characters translated once as they enter the window, one signed-byte LDS
 *                     read per cell, the per-slot signed key (explained in dpx_subst_kernels.hip and dpx_baxt_kernels.hip)
 *   DPX_BAND_SCAN_AFTER the row-m pick-up behind its wave-uniform branch; when ZDROP the per-anti-diagonal DPP maximum and the scalar
 *                     update-or-drop test (explained in dpx_zext_kernels.hip).  best, bi, bj, lastDiag, stop and the row-m key are
 *                     wave-uniform: they cost no vector register
 *   scan_border_line  lane 0's scan for an empty sequence, where the table plays no part
 *   scan_finish       the first row-major maximum over the computed cells and the record (write_results)
 * Prologue, the three phase loops and the stores are k_zext_fill's: anti-diagonal 1 is tested before the loop, each phase ends early
 * on a drop, a drop stores its partial group (the steps of the group that did not run keep the previous group's values, or zeros:
 * they lie behind lastDiag and the host never shows them), and nothing is stored past the pair's last chunk.  The waves of a workgroup
 * share no barrier, so each leaves when its pair is done.
 */
#include "dpx_band_affine.hpp"

namespace {

using namespace dpx_band;

template <int C, bool PB, bool STORE, bool ZDROP>
__global__ void __launch_bounds__(DPX_FILL_THREADS) k_zsub_fill(const dpx_zsub_args za) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const dpx_fill_args &a = za.s.f;
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
    const int Z = za.scan.zdrop, pen = e < 0 ? -e : 0;
    if (m <= 0 || n <= 0) {
        if (lane == 0) scan_border_line<ZDROP>(a, za.scan.endBonus, za.scan.ext, p, m, n, B, [&](const int k) { return o + k * e; }, Z, pen); /* an empty sequence: one border line */
        return;
    }
    const unsigned char *ref = reinterpret_cast<const unsigned char *>(a.seq + pr.refIdx);
    const unsigned char *qry = reinterpret_cast<const unsigned char *>(a.seq + pr.qryIdx);
    /* the wave's LDS slice: [staged query][staged reference][table image]; a.ldsPerWave counts all three */
    unsigned char *my = smem + (size_t)wv * a.ldsPerWave;
    const unsigned char *qL = stage_bytes(my, qry, m, lane, 64);
    const unsigned char *rL = stage_bytes(my + a.ldsRefOff, ref, n, lane, 64);
    unsigned char *img = my + (a.ldsPerWave - (uint32_t)DPX_SUBST_IMAGE_BYTES);
    DPX_TABLE_COPY_ROWS(img, za.s.tab, lane)
    const signed char *tabL = reinterpret_cast<const signed char *>(img);
    const unsigned char *codeL = img + DPX_SUBST_TABLE_BYTES;

    SubstState<C, true> st;
    st.lim = B - 1 - lane * C;
    st.fin = DPX_NEG;
    /* (1, 0), the only cell of row m that no step visits: in band when B >= 2, on anti-diagonal 1 */
    int qe = (m == 1 && B >= 2) ? (int)(((unsigned)oe << 16) | 0xFFFFu) : INT_MIN;
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
#define DPX_ZSUB_STORE(grp_)                                                                                              \
    {                                                                                                                     \
        int16_t *at_ = Hp + (size_t)(grp_) * cs;                                                                          \
        store8(at_, accH);                                                                                                \
        store8(at_ + DPX_BAND_PLANE_ELEMS, accI);                                                                         \
        store8(at_ + 2 * DPX_BAND_PLANE_ELEMS, accD);                                                                     \
    }
#define DPX_ZSUB_BODY(INTERIOR_)                                                                                          \
    _Pragma("unroll") for (int g = 0; g < GG; g += 2) {                                                                  \
        subst_step<C, PB, INTERIOR_, true>(st, A0 + g, i0, j0, lane, m, n, B, o, oe, e, -1, qL, rL, tabL, codeL,          \
                                           &accH[(g % G) * C], &accI[(g % G) * C], &accD[(g % G) * C]);                   \
        DPX_BAND_SCAN_AFTER(A0 + g, &accH[(g % G) * C])                                                                   \
        if constexpr (STORE && G == 1) {                                                                                  \
            if (INTERIOR_ || A0 + g < numGroups) DPX_ZSUB_STORE(A0 + g)                                                   \
        }                                                                                                                 \
        if (stop) break;                                                                                                  \
        subst_step<C, !PB, INTERIOR_, true>(st, A0 + g + 1, i0, j0, lane, m, n, B, o, oe, e, -1, qL, rL, tabL, codeL,     \
                                            &accH[((g + 1) % G) * C], &accI[((g + 1) % G) * C], &accD[((g + 1) % G) * C]); \
        DPX_BAND_SCAN_AFTER(A0 + g + 1, &accH[((g + 1) % G) * C])                                                         \
        if constexpr (STORE) {                                                                                            \
            if (((g + 1) % G) == G - 1) {                                                                                 \
                const int grp = (A0 + g + 1) / G;                                                                         \
                if (INTERIOR_ || grp < numGroups) DPX_ZSUB_STORE(grp)                                                     \
            }                                                                                                             \
        }                                                                                                                 \
        if (stop) break;                                                                                                  \
    }
    /* parity of step A is (A + B + 1) & 1; A0 is even, so even steps have parity PB and odd steps !PB.  Three phases as in k_zext_fill:
     * head (some slots outside the matrix, border slots), interior, tail; each ends early on a drop. */
    int A0 = 0;
    for (; !stop && A0 < NS && !(interior(A0) && interior(A0 + GG - 1)); A0 += GG) { DPX_ZSUB_BODY(false) }
    for (; !stop && A0 + GG <= NS && interior(A0 + GG - 1); A0 += GG) { DPX_ZSUB_BODY(true) }
    for (; !stop && A0 < NS; A0 += GG) { DPX_ZSUB_BODY(false) }
    if constexpr (ZDROP && STORE && G > 1) {
        /* a drop on a step that does not close its store group: the group goes out as it stands (lastDiag >= 2 here means a step ran) */
        if (stop && lastDiag >= 2 && ((lastDiag - 2) % G) != G - 1) {
            const int grp = (lastDiag - 2) / G;
            if (grp < numGroups) DPX_ZSUB_STORE(grp)
        }
    }
#undef DPX_ZSUB_BODY
#undef DPX_ZSUB_STORE
    scan_finish<C>(a, za.scan.endBonus, za.scan.ext, p, st.key, lane, m, B, qe, lastDiag, stop);
}

} // namespace

hipError_t dpx_launch_zsub_fill(const dpx_zsub_args &a, int C, bool store, size_t ldsBytes, hipStream_t stream) {
    if (a.s.f.numPairs <= 0) return hipSuccess;
    if (!a.scan.ext || !a.s.tab.table || !a.s.tab.codeOf) return hipErrorInvalidValue;
    return dispatch_fill(C, a.s.f.band, store, [&](auto c, auto pb, auto st) {
        constexpr int kC = decltype(c)::value;
        constexpr bool kPB = decltype(pb)::value, kStore = decltype(st)::value;
        return a.scan.zdrop >= 0 ? launch_fill(k_zsub_fill<kC, kPB, kStore, true>, a, a.s.f, ldsBytes, stream)
                            : launch_fill(k_zsub_fill<kC, kPB, kStore, false>, a, a.s.f, ldsBytes, stream);
    });
}
