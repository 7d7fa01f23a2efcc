/* dpx_banddir_fill.inc -- the frame of the band-direction fills: everything in k_bdir_fill, k_bdx_fill and k_bd2_fill outside their
 * steps, included inside each kernel (as dpx_affine_fill.inc is: the text sits in the kernel itself, so each kernel compiles to the code
 * it had with its own copy; profiles/banddir_sharing_ab.md).  Pair pick-up, the empty-sequence branch, string staging, the table image
 * into LDS, the state on anti-diagonals 0 and 1, the three phase loops of two-step bodies with one 16-byte store per Gd steps, the
 * partial last group, the tracker and row-m reductions and the result write.
 *
 * In scope, from the kernel:
 *   C, PB, EXT, TABLE, SCAN   the template parameters (k_bdir_fill: TABLE = false, SCAN = 0 as constants)
 *   a, x                      the dpx_fill_args and the block around it (table, codeOf, zdrop, endBonus, ext)
 *   State                     the step's state: prevH, prev2H, qch, rch, bestKey, bestA, lim, fin, w, and clear_gaps(c), which sets slot
 *                             c of every gap plane to DPX_NEG
 *   Gd, kStepBits             steps per 16-byte store, and the code bits one step pushes into the window (Gd * kStepBits = 128)
 *   kPickUniform              which row-m pick-up DPX_BANDDIR_SCAN_AFTER uses (dpx_banddir_dev.hpp, "Scalar registers")
 *   DPX_BANDDIR_WEIGHTS       declarations, expanded behind the pair pick-up (where each kernel had them: declared in front of it they moved
 *                             the argument loads of several instantiations), of
 *       match, mismatch, Z, pen   the byte-compare weights, the drop threshold and the drop test's gap penalty
 *       bord1, bord(k)            H of the in-band border cells of anti-diagonal 1, and of anti-diagonal k (a callable)
 *       line_first_max(L)         an empty sequence: the k in 0 .. L of the first maximum of the border line's cells 1 .. L (0 when L = 0)
 *                             and whatever else the step's arguments need.  The two callables capture BY VALUE: a capture by reference
 *                             takes the address of a weight, and that reordered the registers of every C = 1 instantiation
 *   DPX_BANDDIR_NO_CELL_H     H of a slot that holds no cell on anti-diagonals 0 and 1: DPX_NEG for the global and extension fills, 0 for the
 *                             local ones (k_bdl_fill, k_bdlt_fill), whose neighbours without a cell read H = 0
 *   DPX_BANDDIR_STEP(P1_, INTERIOR_, A_)   the unit's own step on anti-diagonal A_, with the unit's own arguments; it may name st, i0, j0,
 *                             lane, m, n, B, cEnd, qL, rL, tabL, codeL of this text
 *
 * Parity of step A is (A + B + 1) & 1; A0 is even, so even steps have parity PB and odd steps !PB.  Three phases: head (some slots
 * outside the matrix, border slots), interior, tail, each ending early on a drop.  The interior loop stops short of the last
 * anti-diagonal (A = NS-1), so BANW's end cell is always picked up by the general step.  When NS is odd the last pair of steps runs one
 * step past NS - 1, which holds no cell: its anti-diagonal is empty for the scan.
 *
 * A drop (SCAN == 2).  The loop body runs two steps; a drop after the first does not run the second.  The window then holds a partial
 * group: the missing steps are shifted in as zeros and the group goes to chunk (lastDiag - 2) / Gd (the chosen end cell may lie in it),
 * not to the pair's last chunk.  A drop on anti-diagonal 1 stores nothing.  Nothing is stored past the drop: the chunks behind it keep
 * what the pool held, and no walk reads them (a walk only visits smaller anti-diagonals than its start).
 *
 * DPX_BANDDIR_SCORE_ONLY (defined by dpx_bscore_kernels.hip and dpx_lscore_kernels.hip only, in front of the include): the same frame with
 * nothing stored but the results.  The window, the pair's place in the pool, store_group and the partial last group are not compiled;
 * State needs no w, and the kernel defines neither Gd nor kStepBits.  A dropped pair simply ends.  A preprocessor switch and not a
 * template constant: the text the storing units see is the text they had. */
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int kLogC = C == 8 ? 3 : C == 4 ? 2 : C == 2 ? 1 : 0;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int p = blockIdx.x * (int)a.wavesPerBlock + wv;
    if (p >= a.numPairs) return;
    if (a.order) p = a.order[p];
    const dpx_pair_dev pr = a.pairs[p];
    const int n = pr.n, m = pr.m, B = a.band;
    DPX_BANDDIR_WEIGHTS
    if (m <= 0 || n <= 0) { /* an empty sequence: no cell has a code and no diagonal step runs, so a table plays no part */
        if (lane == 0) {
            if constexpr (SCAN > 0) {
                scan_border_line<SCAN == 2>(a, x.scan.endBonus, x.scan.ext, p, m, n, B, bord, Z, pen);
            } else if constexpr (EXT) { /* the first maximum of the one border line, when it is above the 0 of (0, 0) */
                const int L = min(max(max(m, n), 0), B - 1);
                const int k = line_first_max(L);
                const int v = k > 0 ? bord(k) : 0;
                const bool take = v > 0;
                a.score[p] = take ? v : 0;
                a.endRow[p] = (take && m > 0) ? k : 0;
                a.endCol[p] = (take && m <= 0) ? k : 0;
            } else {
                a.score[p] = (m > 0 || n > 0) ? bord(max(m, n)) : 0;
                a.endRow[p] = max(m, 0);
                a.endCol[p] = max(n, 0);
            }
        }
        return;
    }
    const unsigned char *ref = reinterpret_cast<const unsigned char *>(a.seq + pr.refIdx);
    const unsigned char *qry = reinterpret_cast<const unsigned char *>(a.seq + pr.qryIdx);
    /* the wave's LDS slice: [staged query][staged reference] and, TABLE, [table image]; a.ldsPerWave counts all of it */
    unsigned char *my = smem + (size_t)wv * a.ldsPerWave;
    const unsigned char *qL = stage_bytes(my, qry, m, lane, 64);
    const unsigned char *rL = stage_bytes(my + a.ldsRefOff, ref, n, lane, 64);
    [[maybe_unused]] const signed char *tabL = nullptr;
    [[maybe_unused]] const unsigned char *codeL = nullptr;
    if constexpr (TABLE) {
        unsigned char *img = my + (a.ldsPerWave - (uint32_t)DPX_SUBST_IMAGE_BYTES);
        codeL = table_stage_rows(img, x.tab, lane);
        tabL = reinterpret_cast<const signed char *>(img);
    }

    State st;
    st.lim = B - 1 - lane * C;
    st.fin = DPX_NEG;
#ifndef DPX_BANDDIR_SCORE_ONLY
    st.w[0] = st.w[1] = st.w[2] = st.w[3] = 0u;
#endif
    { /* anti-diagonals a = 1 (prev: the border cells (0, 1) and (1, 0), in band when B >= 2) and a = 0 (prev2: H[0][0] = 0, which
       * shares its slot with cell (1, 1)); the character windows are those of a = 1, the first real step then slides one of them */
        const int p1 = B & 1;
        const int vi0 = (1 + p1 - (B - 1)) >> 1;
        const int vj0 = 1 - vi0;
#pragma unroll
        for (int c = 0; c < C; c++) {
            const int s = lane * C + c;
            const int qb = qL[min(max(vi0 + s - 1, 0), m - 1)], rb = rL[min(max(vj0 - s - 1, 0), n - 1)];
            if constexpr (TABLE) {
                st.qch[c] = codeL[qb];
                st.rch[c] = (int)codeL[rb] << 5;
            } else {
                st.qch[c] = qb;
                st.rch[c] = rb;
            }
            const int bi0 = vi0 + s; /* the slot's cell on a = 1 is (bi0, 1 - bi0) */
            st.prevH[c] = (B >= 2 && (bi0 == 0 || bi0 == 1)) ? bord1 : DPX_BANDDIR_NO_CELL_H;
            st.prev2H[c] = (s == ((B - 1) >> 1)) ? 0 : DPX_BANDDIR_NO_CELL_H;
            st.clear_gaps(c);
        }
        st.bestKey = 0xFFFFFFFFll; /* score 0 at row 0: only H > 0 displaces it */
        st.bestA = 0;
    }
    /* the lane and register that own the end cell (m, n) on the last anti-diagonal (BANW) */
    const int sEnd = (m - n + B - 1) >> 1;
    const int cEnd = (!EXT && lane == sEnd / C) ? (sEnd % C) : -1;
    /* is every in-band slot of anti-diagonal A inside the matrix?  (true for one contiguous range of A) */
    auto interior = [&](const int A) -> bool {
        const int aa = A + 2, pp = (aa + B - 1) & 1;
        const int ii0 = (aa + pp - (B - 1)) >> 1, jj0 = aa - ii0, top = B - 1 - pp;
        return ii0 >= 1 && ii0 + top <= m && jj0 - top >= 1 && jj0 <= n;
    };
    const int NS = m + n - 1;                 /* anti-diagonals a = 2 .. m+n */
#ifndef DPX_BANDDIR_SCORE_ONLY
    const int numGroups = (NS + Gd - 1) / Gd; /* == the layout's chunks of the pair: no store goes past the pair's last chunk */
    unsigned char *base = reinterpret_cast<unsigned char *>(a.mat) + (size_t)pr.matOff * 2u;
    const uint64_t cs = (uint64_t)pr.chunkStride * 2u;
#endif
    int i0 = (1 + (B & 1) - (B - 1)) >> 1;
    int j0 = 1 - i0;
    /* the scan's state.  Row m: every lane keeps (score, column) of the row-m cells its own slots held, replaced when strictly greater
     * (a lane meets them in column order), reduced across lanes at the end; (1, 0) is the only cell of row m that no step visits: in
     * band when B >= 2, on anti-diagonal 1.  That anti-diagonal is non-empty when B >= 2, and its maximum bord1 sits at its smallest
     * row, (0, 1) */
    [[maybe_unused]] int qeScore = (m == 1 && B >= 2) ? bord1 : DPX_NEG / 2 /* (none yet: every cell is above it) */, qeCol = (m == 1 && B >= 2) ? 0 : -1;
    [[maybe_unused]] int best = 0, bi = 0, bj = 0, lastDiag = m + n;
    bool stop = false;
    if constexpr (SCAN == 2) {
        if (B >= 2 && zdrop_test(bord1, 0, 1, Z, pen, best, bi, bj)) {
            lastDiag = 1;
            stop = true;
        }
    }
#ifndef DPX_BANDDIR_SCORE_ONLY
    auto store_group = [&](const int grp) {
        if (grp < numGroups)
            *reinterpret_cast<u32x4 *>(base + dpx_banddir_piece((uint64_t)grp, lane, cs)) = u32x4{st.w[0], st.w[1], st.w[2], st.w[3]};
    };
#define DPX_BANDDIR_STORE_AFTER(A_) if ((((A_) + 2) & (Gd - 1)) == 0) store_group(((A_) + 1) / Gd);
#else
#define DPX_BANDDIR_STORE_AFTER(A_)
#endif
#define DPX_BANDDIR_BODY(INTERIOR_)                                                                                       \
    {                                                                                                                     \
        DPX_BANDDIR_STEP(PB, INTERIOR_, A0);                                                                              \
        DPX_BANDDIR_SCAN_AFTER(A0)                                                                                        \
        if (stop) break; /* (a drop after the first step: the second does not run) */                                     \
        DPX_BANDDIR_STEP(!PB, INTERIOR_, A0 + 1);                                                                         \
        DPX_BANDDIR_SCAN_AFTER(A0 + 1)                                                                                    \
        DPX_BANDDIR_STORE_AFTER(A0)                                                                                       \
        if (stop) break;                                                                                                  \
    }
    int A0 = 0;
    for (; !stop && A0 < NS && !(interior(A0) && interior(A0 + 1)); A0 += 2) DPX_BANDDIR_BODY(false)
    for (; !stop && A0 + 2 < NS && interior(A0 + 1); A0 += 2) DPX_BANDDIR_BODY(true)
    for (; !stop && A0 < NS; A0 += 2) DPX_BANDDIR_BODY(false)
#undef DPX_BANDDIR_BODY
#undef DPX_BANDDIR_STORE_AFTER
    /* the partial last group.  `pushed` steps have entered the window, pushed % Gd of them since the last store (a drop on step A left
     * lastDiag = A + 2; a group that the dropping step completed has been stored already); the missing steps are shifted in as zeros
     * so that step t of the group sits at code t * C.  Without a drop the group is the pair's last chunk, after one the chunk of the
     * dropping step; a drop on anti-diagonal 1 ran no step and stores nothing. */
#ifndef DPX_BANDDIR_SCORE_ONLY
    const int pushed = stop ? lastDiag - 1 : A0;
    if (pushed & (Gd - 1)) {
        for (int t = pushed & (Gd - 1); t < Gd; t++) window_push<kStepBits>(st.w, 0u);
        store_group(pushed / Gd);
    }
#endif
    if constexpr (!EXT) {
        if (cEnd >= 0) { a.score[p] = st.fin; a.endRow[p] = m; a.endCol[p] = n; }
    } else {
        /* the lane's candidate; across lanes max score, then min row, then min column.  A border slot decodes to i = 0 or j = 0.
         * (The border cells of anti-diagonal 1, which no step visits, need no candidate: they count only when bord1 > 0, and then the
         * pair cannot drop at anti-diagonal 1, so (1, 1) is computed and holds H >= 2 * bord1 > bord1.) */
        int hv = (int)(st.bestKey >> 32);
        unsigned long long at = ~0ull;
        if (hv > 0) {
            const int i = (int)~(unsigned)(st.bestKey & 0xFFFFFFFFll);
            at = ((unsigned long long)(unsigned)i << 32) | (unsigned long long)(unsigned)(st.bestA + 2 - i);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int oh = __shfl_xor(hv, off, 64);
            const unsigned long long oa = __shfl_xor(at, off, 64);
            if (oh > hv || (oh == hv && oa < at)) { hv = oh; at = oa; }
        }
        if constexpr (SCAN > 0) { /* row m: the highest score, then the smallest column */
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const int os = __shfl_xor(qeScore, off, 64), oc = __shfl_xor(qeCol, off, 64);
                if (os > qeScore || (os == qeScore && oc < qeCol)) { qeScore = os; qeCol = oc; }
            }
        }
        if (lane == 0) {
            const int maxRow = hv > 0 ? (int)(at >> 32) : 0, maxCol = hv > 0 ? (int)(at & 0xFFFFFFFFull) : 0;
            if constexpr (SCAN > 0) {
                write_results(a, x.scan.endBonus, x.scan.ext, p, m, max(hv, 0), maxRow, maxCol, qeCol >= 0 ? qeScore : INT_MIN, qeCol, lastDiag, stop);
            } else {
                a.score[p] = hv;
                a.endRow[p] = maxRow;
                a.endCol[p] = maxCol;
            }
        }
    }
