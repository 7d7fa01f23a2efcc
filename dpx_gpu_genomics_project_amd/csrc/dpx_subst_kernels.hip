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
 * The step itself, subst_step with its SubstState, lives in dpx_band_affine.hpp: k_zsub_fill (dpx_zsub_kernels.hip) runs the same text.
 *
 * The walks are BANW's two (one lane per pair; one wave per pair with an LDS window), the same templates under TableScorer
 * (dpx_band_affine.hpp: band_walk_lane, band_walk_wave), with mm = H_diag + s(r, q); the relation character
 * is still the byte compare.  The one-lane walk reads table and map from global memory (1280 bytes, resident in L1 after the first
 * steps); the wave walk keeps the table in LDS behind its window and translates a lane's two characters when it loads a window.
 */
#include "dpx_band_affine.hpp"

namespace {

using namespace dpx_band;

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
    DPX_TABLE_COPY_ROWS(img, sa.tab, lane)
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

/* the one-lane walk reads table and map from global memory (1280 bytes, resident in L1 after the first steps) */
__global__ void k_subst_traceback(const dpx_subst_args sa, int numPairs, const int32_t *endRow, const int32_t *endCol,
                                  const uint64_t *tbOff, char *tb, int32_t *tbLen) {
    band_walk_lane(sa.f, TableScorer{reinterpret_cast<const signed char *>(sa.tab.table), sa.tab.codeOf}, numPairs, endRow, endCol, tbOff, tb, tbLen);
}

/* the wave walk keeps the table in LDS behind its window and reads the map from global memory */
__global__ void __launch_bounds__(64) k_subst_traceback_wave(const dpx_subst_args sa, int numPairs, const int32_t *endRow, const int32_t *endCol,
                                                             const uint64_t *tbOff, char *tb, int32_t *tbLen) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smemTb[];
    band_walk_wave(sa.f, TableScorer{reinterpret_cast<const signed char *>(smemTb + BandWin::kBytes), sa.tab.codeOf}, sa.tab.table, smemTb, numPairs,
                   endRow, endCol, tbOff, tb, tbLen);
}

} // namespace

hipError_t dpx_launch_subst_fill(const dpx_subst_args &a, int C, bool store, bool ext, size_t ldsBytes, hipStream_t stream) {
    if (a.f.numPairs <= 0) return hipSuccess;
    return dispatch_fill(C, a.f.band, store, [&](auto c, auto pb, auto st) {
        constexpr int kC = decltype(c)::value;
        constexpr bool kPB = decltype(pb)::value, kStore = decltype(st)::value;
        return ext ? launch_fill(k_subst_fill<kC, kPB, kStore, true>, a, a.f, ldsBytes, stream)
                   : launch_fill(k_subst_fill<kC, kPB, kStore, false>, a, a.f, ldsBytes, stream);
    });
}

hipError_t dpx_launch_subst_traceback(const dpx_subst_args &a, int numPairs, int walk, const uint64_t *tbOff, char *tb, int32_t *tbLen,
                                      hipStream_t stream) {
    if (numPairs <= 0) return hipSuccess;
    if (walk == 2) /* one wave per pair with an LDS window, the table behind it */
        hipLaunchKernelGGL(k_subst_traceback_wave, dim3((unsigned)numPairs), dim3(64), (size_t)BandWin::kBytes + DPX_SUBST_TABLE_BYTES, stream, a,
                           numPairs, a.f.endRow, a.f.endCol, tbOff, tb, tbLen);
    else
        hipLaunchKernelGGL(k_subst_traceback, dim3((unsigned)((numPairs + 63) / 64)), dim3(64), 0, stream, a, numPairs, a.f.endRow, a.f.endCol,
                           tbOff, tb, tbLen);
    return hipGetLastError();
}
