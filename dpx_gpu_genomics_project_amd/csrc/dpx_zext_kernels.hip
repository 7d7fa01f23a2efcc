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
 */
#include <limits.h>

#include "dpx_band_affine.hpp"

namespace {

using namespace dpx_band;

/* the signed maximum over the 64 lanes, on the VALU: row_shr 1, 2, 4, 8 bring each row's maximum to its lane 15, row_bcast:15 and
 * row_bcast:31 carry it on to lane 63.  A lane without a source keeps INT_MIN.  All 64 lanes must be active. */
template <int CTRL, int ROWS>
__device__ __forceinline__ int dpp_max(const int v) {
    return max(v, __builtin_amdgcn_update_dpp(INT_MIN, v, CTRL, ROWS, 0xf, false));
}
__device__ __forceinline__ int wave_max_i32(int v) {
    v = dpp_max<0x111, 0xf>(v);
    v = dpp_max<0x112, 0xf>(v);
    v = dpp_max<0x114, 0xf>(v);
    v = dpp_max<0x118, 0xf>(v);
    v = dpp_max<0x142, 0xa>(v);
    v = dpp_max<0x143, 0xc>(v);
    return __builtin_amdgcn_readlane(v, 63);
}

/* the scan's update-or-drop rule for one non-empty anti-diagonal whose maximum dm sits at (ia, ja); true = the pair is dropped here */
__device__ __forceinline__ bool zdrop_test(const int dm, const int ia, const int ja, const int Z, const int pen, int &best, int &bi, int &bj) {
    if (dm > best) {
        best = dm;
        bi = ia;
        bj = ja;
        return false;
    }
    return ia >= bi && ja >= bj && best - dm > Z + pen * abs((ia - bi) - (ja - bj));
}

/* the pair's results from lane 0: the record, and the chosen score and end cell where BAXT's go */
__device__ __forceinline__ void write_results(const dpx_zext_args &a, const int p, const int m, const int maxScore, const int maxRow,
                                              const int maxCol, const int qeScore, const int qeCol, const int lastDiag, const bool dropped) {
    const int E = a.endBonus;
    const bool reached = E >= 0 && !dropped && qeCol >= 0 && qeScore + E > maxScore;
    a.f.score[p] = reached ? qeScore : maxScore;
    a.f.endRow[p] = reached ? m : maxRow;
    a.f.endCol[p] = reached ? qeCol : maxCol;
    u32x4 *rec = reinterpret_cast<u32x4 *>(a.ext + (size_t)p * 8u);
    const u32x4 w0 = {(unsigned)maxScore, (unsigned)maxRow, (unsigned)maxCol, (unsigned)qeScore};
    const u32x4 w1 = {(unsigned)qeCol, (unsigned)lastDiag, (dropped ? 1u : 0u) | (reached ? 2u : 0u), 0u};
    rec[0] = w0;
    rec[1] = w1;
}

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
    const int Z = a.zdrop, pen = e < 0 ? -e : 0;
    if (m <= 0 || n <= 0) {
        /* an empty sequence: the in-band cells are one border line, cell k (1 <= k <= L = min(max(m, n), B-1)) on anti-diagonal k with
         * H = o + k*e, and 0 at k = 0.  The scan, the maximum and the row-m rule run over it on lane 0. */
        if (lane == 0) {
            const int len = max(max(m, n), 0), L = min(len, B - 1);
            int best = 0, kb = 0, last = len, maxScore = 0, kmax = 0;
            bool dropped = false;
            for (int k = 1; k <= L; k++) {
                const int v = o + k * e;
                if (v > best) {
                    best = v;
                    kb = k;
                } else if (ZDROP && best - v > Z + pen * (k - kb)) {
                    last = k;
                    dropped = true;
                    break;
                }
            }
            const int seen = min(L, last); /* the computed cells are k = 0 .. seen */
            for (int k = 1; k <= seen; k++)
                if (o + k * e > maxScore) { maxScore = o + k * e; kmax = k; }
            int qeScore = INT_MIN, qeCol = -1;
            if (m <= 0) { /* row m is row 0: the line itself (or the single cell (0, 0)) */
                qeScore = 0;
                qeCol = 0;
                for (int k = 1; k <= (n > 0 ? seen : 0); k++)
                    if (o + k * e > qeScore) { qeScore = o + k * e; qeCol = k; }
            } else if (m <= seen) { /* n == 0: row m holds the one cell (m, 0) */
                qeScore = o + m * e;
                qeCol = 0;
            }
            write_results(a, p, max(m, 0), maxScore, m > 0 ? kmax : 0, m > 0 ? 0 : kmax, qeScore, qeCol, last, dropped);
        }
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
#define DPX_ZEXT_AFTER(A_, h_)                                                                                            \
    {                                                                                                                     \
        const int a_ = (A_) + 2;                                                                                          \
        if (a_ >= m && a_ - m <= n && abs(2 * m - a_) <= B - 1) {                                                         \
            const int sm_ = m - i0, ln_ = sm_ / C, cc_ = sm_ % C; /* (0 <= sm_ <= B-1: the cell is in the band) */          \
            int v_ = 0;                                                                                                   \
            _Pragma("unroll") for (int c = 0; c < C; c++)                                                                 \
                if (cc_ == c) v_ = __builtin_amdgcn_readlane((h_)[c], ln_);                                               \
            qe = max(qe, (int)(((unsigned)v_ << 16) | (0xFFFFu - (unsigned)(a_ - 1))));                                   \
        }                                                                                                                 \
        if constexpr (ZDROP) {                                                                                            \
            const int rb_ = 0xFFFF - i0 - lane * C;                                                                       \
            int k_ = INT_MIN;                                                                                             \
            _Pragma("unroll") for (int c = 0; c < C; c++) k_ = max(k_, (int)pack_lo16(rb_ - c, max((h_)[c], -32768)));    \
            k_ = wave_max_i32(k_);                                                                                        \
            const int dm_ = k_ >> 16;                                                                                     \
            if (dm_ > -32768) { /* (else: no cell on this anti-diagonal) */                                               \
                const int ia_ = 0xFFFF - (k_ & 0xFFFF);                                                                   \
                if (zdrop_test(dm_, ia_, a_ - ia_, Z, pen, best, bi, bj)) {                                               \
                    lastDiag = a_;                                                                                        \
                    stop = true;                                                                                          \
                }                                                                                                         \
            }                                                                                                             \
        }                                                                                                                 \
    }
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
    /* the maximum of H over the computed cells and its first cell in row-major order, as k_baxt_fill finds it: every slot's first
     * maximum (within a slot cells arrive in row-major order); across slots max score, min row, min col.  The border cells of
     * anti-diagonal 1 need no candidate: they count only when o + e > 0, and then the pair cannot drop at anti-diagonal 1, so (1, 1)
     * is computed and holds H >= 2 * (o + e) > o + e. */
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
    const int qeTop = qe;
    if (lane == 0) {
        const int hv = (int)(top >> 40);
        const int maxRow = hv > 0 ? (int)(0xFFFFFu - (unsigned)((top >> 20) & 0xFFFFFu)) : 0;
        const int maxCol = hv > 0 ? (int)(0xFFFFFu - (unsigned)(top & 0xFFFFFu)) : 0;
        const bool none = qeTop == INT_MIN;
        const int qeScore = none ? INT_MIN : (qeTop >> 16);
        const int qeCol = none ? -1 : (0xFFFF - (qeTop & 0xFFFF)) + 1 - m;
        write_results(a, p, m, hv, maxRow, maxCol, qeScore, qeCol, lastDiag, stop);
    }
}

} // namespace

hipError_t dpx_launch_zext_fill(const dpx_zext_args &a, int C, bool store, size_t ldsBytes, hipStream_t stream) {
    if (a.f.numPairs <= 0) return hipSuccess;
    if (!a.ext) return hipErrorInvalidValue;
    return dispatch_fill(C, a.f.band, store, [&](auto c, auto pb, auto st) {
        constexpr int kC = decltype(c)::value;
        constexpr bool kPB = decltype(pb)::value, kStore = decltype(st)::value;
        return a.zdrop >= 0 ? launch_fill(k_zext_fill<kC, kPB, kStore, true>, a, a.f, ldsBytes, stream)
                            : launch_fill(k_zext_fill<kC, kPB, kStore, false>, a, a.f, ldsBytes, stream);
    });
}
