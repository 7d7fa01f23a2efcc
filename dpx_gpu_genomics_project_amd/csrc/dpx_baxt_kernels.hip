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
 * Schedule, stores and the three phases are k_banw_fill's (anti-diagonals a = i+j, slot s = (i-j+B-1)>>1, lane l owns the C = ceil(B/64)
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
#include <hip/hip_runtime.h>
#include <stdint.h>

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

template <int C>
struct BaxtState {
    int prevH[C], prev2H[C]; /* H on anti-diagonals a-1 and a-2 */
    int prevI[C], prevD[C];  /* I and D on anti-diagonal a-1 */
    int qch[C], rch[C];      /* query / reference character of each slot's cell */
    int key[C];              /* running signed max of (H << 16 | 0xFFFF - A): max score, then earliest step */
    int lim;                 /* B-1 - lane*C: slot c is inside the band on a step of parity p when c + p <= lim */
};

/* INTERIOR: every in-band slot of this anti-diagonal lies inside the matrix, so validity is one compare against the per-lane
 * constant `lim` instead of two against the step's slot window, and there is no border slot */
template <int C, bool P1, bool INTERIOR>
__device__ __forceinline__ void baxt_step(BaxtState<C> &st, const int A, int &i0, int &j0, const int lane, const int m, const int n,
                                          const int B, const int match, const int mismatch, const int o, const int oe, const int e,
                                          const unsigned char *qL, const unsigned char *rL, int *outH, int *outI, int *outD) {
    const int p = P1 ? 1 : 0;
    if constexpr (P1) i0++; else j0++;
    const int smin = INTERIOR ? 0 : max(max(1 - i0, j0 - n), 0);
    const int smax = INTERIOR ? 0 : min(min(m - i0, j0 - 1), B - 1 - p);
    /* the in-band border cells of this anti-diagonal: (0, a) in slot -i0 and (a, 0) in slot j0, both H = o + a * e, while a <= B-1 */
    const int a = A + 2;
    const int bord = (INTERIOR || a > B - 1) ? DPX_NEG : o + a * e;
    const int sTop = (INTERIOR || a > n) ? -1 : -i0, sLeft = (INTERIOR || a > m) ? -1 : j0;
    const int lo = smin - lane * C, cnt = max(smax - smin + 1, 0), cTop = sTop - lane * C, cLeft = sLeft - lane * C;
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
    const int negA = 0xFFFF - A;
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
            /* slot lane * C + c against the step's window [smin, smax] and its two border slots, as compares of the constant c with
             * per-lane values: one unsigned range compare (cnt = 0 when the window is empty) */
            const bool valid = (unsigned)(c - lo) < (unsigned)cnt;
            h = valid ? h : ((c == cTop || c == cLeft) ? bord : DPX_NEG);
            d = valid ? d : DPX_NEG;
            ii = valid ? ii : DPX_NEG;
        }
        st.key[c] = max(st.key[c], (int)(((unsigned)h << 16) | (unsigned)negA)); /* (after the border select: border cells take part) */
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

    BaxtState<C> st;
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
        baxt_step<C, PB, INTERIOR_>(st, A0 + g, i0, j0, lane, m, n, B, match, mismatch, o, oe, e, qL, rL,                 \
                                    &accH[(g % G) * C], &accI[(g % G) * C], &accD[(g % G) * C]);                          \
        if constexpr (STORE && G == 1) {                                                                                  \
            if (INTERIOR_ || A0 + g < numGroups) DPX_BAXT_STORE(A0 + g)                                                   \
        }                                                                                                                 \
        baxt_step<C, !PB, INTERIOR_>(st, A0 + g + 1, i0, j0, lane, m, n, B, match, mismatch, o, oe, e, qL, rL,            \
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

template <class K>
hipError_t launch_baxt_kernel(K kernel, const dpx_fill_args &a, dim3 grid, size_t lds, hipStream_t s) {
    if (lds > 64u * 1024u) { /* opt in to more than the default 64 KiB of dynamic LDS */
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const unsigned wpb = a.wavesPerBlock; /* `lds` is the request of a four-wave workgroup */
    hipLaunchKernelGGL(kernel, grid, dim3(64u * wpb), lds / 4u * wpb, s, a);
    return hipGetLastError();
}

template <int C>
hipError_t launch_baxt_C(const dpx_fill_args &a, bool store, dim3 grid, size_t lds, hipStream_t s) {
    const bool pb = ((a.band + 1) & 1) != 0; /* parity of step A = 0 */
    if (pb) return store ? launch_baxt_kernel(k_baxt_fill<C, true, true>, a, grid, lds, s)
                         : launch_baxt_kernel(k_baxt_fill<C, true, false>, a, grid, lds, s);
    return store ? launch_baxt_kernel(k_baxt_fill<C, false, true>, a, grid, lds, s)
                 : launch_baxt_kernel(k_baxt_fill<C, false, false>, a, grid, lds, s);
}

} // namespace

hipError_t dpx_launch_baxt_fill(const dpx_fill_args &a, int C, bool store, size_t ldsBytes, hipStream_t stream) {
    if (a.numPairs <= 0) return hipSuccess;
    const int wavesPerBlock = (int)a.wavesPerBlock;
    dim3 grid((unsigned)((a.numPairs + wavesPerBlock - 1) / wavesPerBlock));
    switch (C) {
    case 1: return launch_baxt_C<1>(a, store, grid, ldsBytes, stream);
    case 2: return launch_baxt_C<2>(a, store, grid, ldsBytes, stream);
    case 4: return launch_baxt_C<4>(a, store, grid, ldsBytes, stream);
    case 8: return launch_baxt_C<8>(a, store, grid, ldsBytes, stream);
    default: return hipErrorInvalidValue;
    }
}
