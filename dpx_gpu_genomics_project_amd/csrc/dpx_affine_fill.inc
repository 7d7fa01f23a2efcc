/* dpx_affine_fill.inc -- body of the one-wave-per-pair affine-gap fill kernels, included by dpx_affine_kernels.hip inside k_affine_fill (ANW,
 * LOCAL = false), k_asw_fill (ASW, LOCAL = true) and k_asg_fill (ASG, SEMI = true: ANW's cells under a zero row-0 border, the end cell is
 * the first maximum of row m, column 0 included).  The body sits in each kernel itself rather than in a shared __device__ function:
 * passing the kernel argument block to a function changed the scheduling of the ANW kernel (its gfx950 code differed, and 4000 x 512^2
 * filled 3-8 % slower); included this way the ANW kernels compile to the code they compiled to before ASW existed.
 * dpx_scoretab_kernels.hip includes it inside k_scoretab_fill with TABLE = true (score-only batches under dpx_batch_set_score_table): the
 * diagonal term is tableG[codeOfG[reference byte] * 32 + codeOfG[query byte]], read from the wave's own LDS image.
 * In scope: `a` (the kernel's dpx_fill_args), R, STORE, LOCAL, SEMI, TABLE and the two global pointers tableG / codeOfG (null constants
 * where TABLE is false: nothing of the table survives in those kernels). */
    constexpr int MODE = LOCAL ? 1 : (SEMI ? 2 : 0); /* aff_cells: ANW, ASW, ASG */
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int p = blockIdx.x * (int)a.wavesPerBlock + wv;
    if (p >= a.numPairs) return;
    if (a.order) p = a.order[p];
    const dpx_pair_dev pr = a.pairs[p];
    const int n = pr.n, m = pr.m;
    const int match = a.match, mismatch = a.mismatch;
    const int o = a.gapOpen, e = a.gapExtend, oe = o + e;

    if (m <= 0 || n <= 0) {
        if (lane == 0) { /* H[m][n] on the border: 0 at the origin, else o + len*e (AffineNeedlemanWunsch.cpp:43-53); ASW: score 0 at (0, 0);
                          * ASG: row 0 is free (0 at (0, 0)), an empty reference leaves the query as one gap (o + m*e at (m, 0)) */
            const int len = m <= 0 ? max(n, 0) : m;
            a.score[p] = (LOCAL || len <= 0 || (SEMI && m <= 0)) ? 0 : o + len * e;
            a.endRow[p] = LOCAL ? 0 : max(m, 0);
            a.endCol[p] = (LOCAL || SEMI) ? 0 : max(n, 0);
        }
        return;
    }
    const unsigned char *ref = reinterpret_cast<const unsigned char *>(a.seq + pr.refIdx);
    const unsigned char *qry = reinterpret_cast<const unsigned char *>(a.seq + pr.qryIdx);
    unsigned char *my = smem + (size_t)wv * a.ldsPerWave;
    int16_t *edgeH = reinterpret_cast<int16_t *>(my);
    int16_t *edgeD = reinterpret_cast<int16_t *>(my + a.ldsEdge2Off);
    const unsigned char *refl = stage_bytes(my + a.ldsRefOff + 64, ref, n, lane, 64) - 64;
    /* row-0 border H[0][j] = o + j*e (AffineNeedlemanWunsch.cpp:50-53); D[0][j] is the virtual DPX_NEG (k == 0 below) */
    for (int x = lane; x <= n + 1; x += 64) { edgeH[x] = (int16_t)((LOCAL || SEMI) ? 0 : o + x * e); edgeD[x] = 0; } /* (ASW / ASG: H[0][j] = 0) */
    [[maybe_unused]] unsigned char *img = nullptr;
    [[maybe_unused]] const unsigned char *codeL = nullptr;
    if constexpr (TABLE) { /* the wave's own table image behind its LDS slice (a.ldsPerWave counts it); the staged reference becomes codes, once */
        img = my + (a.ldsPerWave - (uint32_t)DPX_SUBST_IMAGE_BYTES);
        codeL = table_stage(img, tableG, codeOfG, lane);
        table_translate(const_cast<unsigned char *>(refl) + 64, n, lane, 64, codeL);
    }

    int16_t *Mp = a.mat + pr.matOff;
    const int W = n + 63;
    const int S = dpx_tiled_stripes(m, R);
    AffState<R> st;
    [[maybe_unused]] int bestv = 0, bestrow = 0, bestcol = 0; /* ASW */
    [[maybe_unused]] const int rsel = (m - 1) % R;            /* ASG: the register of row m in the lane that owns it (a stripe is 64 * R rows) */

    if (STORE && S >= 2 && n >= 128) {
        /* ---------- rolling schedule (see k_linear_fill): lanes run straight on into the next stripe ---------- */
        const unsigned char *ql = stage_bytes(my + a.ldsQryOff, qry, m, lane, 64);
        int row0 = lane * R;
        int nrows = min(max(m - row0, 0), R);
        int jl = 1 - lane, kl = 0;
        load_query_rows<R>(st.qc, qry, row0, nrows);
#pragma unroll
        for (int r = 0; r < R; r++) {
            st.Hl[r] = LOCAL ? 0 : o + (row0 + 1 + r) * e;
            st.Il[r] = DPX_NEG;
            st.Dl[r] = DPX_NEG;
            st.key[r] = 0u;
        }
        st.dtop = (LOCAL || row0 == 0) ? 0 : o + row0 * e;
        int j0 = 1;
        bool sw = false;
        int rcN = refl[63 + jl];
        int eHN = edgeH[1];
        int eDN = DPX_NEG; /* lane 0 is in stripe 0 first: virtual D[0][j] */
        const size_t cs = pr.chunkStride;
        int16_t *tile = Mp + (size_t)lane * R;
        const int total = S * n + 63;
        auto roll_step = [&](const int T) {
            const int rc = rcN, eH = eHN, eD = eDN;
            const int jn = (jl >= n) ? 1 : jl + 1;
            rcN = refl[63 + jn];
            j0 = (j0 >= n) ? 1 : j0 + 1;
            eHN = edgeH[j0];
            eDN = (T + 1 < n) ? DPX_NEG : (int)edgeD[j0]; /* lane 0 leaves stripe 0 after n steps */
            const int upH = wave_shr1(st.Hl[R - 1], eH);
            const int upD = wave_shr1(st.Dl[R - 1], eD);
            if (sw) {
                if constexpr (LOCAL) fold_row_keys<R>(st.key, row0, nrows, bestv, bestrow, bestcol);
                row0 += 64 * R;
                nrows = min(max(m - row0, 0), R);
#pragma unroll
                for (int r = 0; r < R; r++) {
                    st.qc[r] = (r < nrows) ? (int)ql[row0 + r] : 0x100;
                    st.Hl[r] = LOCAL ? 0 : o + (row0 + 1 + r) * e;
                    st.Il[r] = DPX_NEG;
                    st.Dl[r] = DPX_NEG;
                    st.key[r] = 0u;
                }
                st.dtop = LOCAL ? 0 : o + row0 * e;
            }
            if (jl >= 1 && kl < S && nrows > 0) {
                aff_cells<R, MODE>(st, upH, upD, rc, match, mismatch, oe, e, 0xFFFFu - (unsigned)jl, rsel);
                if (lane == 63 && kl + 1 < S) {
                    edgeH[jl] = (int16_t)st.Hl[R - 1];
                    edgeD[jl] = (int16_t)st.Dl[R - 1];
                }
            }
            if constexpr (STORE) {
                if (ramp_stores<R>(lane, T, S * n, a.rampLines)) { /* on the pair's two ramps only the lines with cells */
                    int16_t *dst = tile + (size_t)T * cs;
                    store_tile<R>(dst, st.Hl);
                    store_tile<R>(dst + 64 * R, st.Il);
                    store_tile<R>(dst + 128 * R, st.Dl);
                }
            }
            sw = false;
            if (jl >= n) { jl = 1; kl++; sw = kl < S; }
            else jl++;
        };
        int T = 0;
        for (; T + 1 < total; T += 2) {
            roll_step(T);
            roll_step(T + 1);
        }
        if (T < total) roll_step(T);
        if constexpr (LOCAL) fold_row_keys<R>(st.key, row0, nrows, bestv, bestrow, bestcol);
    } else {
    for (int k = 0; k < S; k++) {
            const int base = k * 64 * R;
            const int row0 = base + lane * R;
            const int nrows = min(max(m - row0, 0), R);
            const bool laneHasRows = nrows > 0;
            const bool hasNext = (k + 1 < S);
            load_query_rows<R>(st.qc, qry, row0, nrows);
            if constexpr (TABLE) { /* the LDS addresses of the lane's query codes' columns of the transposed image (table_column), once per stripe (rows past m: some code, their cells are never read back) */
    #pragma unroll
                for (int r = 0; r < R; r++) st.qc[r] = table_column(img, codeL, st.qc[r]);
            }
    #pragma unroll
            for (int r = 0; r < R; r++) {
                st.Hl[r] = LOCAL ? 0 : o + (row0 + 1 + r) * e; /* H[i][0] = o + i*e (:43-46); ASW: 0 */
                st.Il[r] = DPX_NEG;                /* virtual I[i][0] */
                st.Dl[r] = DPX_NEG;
                st.key[r] = 0u;
            }
            st.dtop = (LOCAL || row0 == 0) ? 0 : o + row0 * e; /* H[0][0] = 0 */
            const size_t cs = pr.chunkStride;
            int16_t *tile = Mp + (size_t)k * (size_t)n * cs + (size_t)lane * R;
    
            const unsigned char *rp = refl + 64 - lane;
            int rcN = rp[0];
            int eHN = edgeH[1];
            int eDN = k == 0 ? DPX_NEG : (int)edgeD[1];
    #define DPX_AFF_STEP(MASKED_, WHOLE_, HASROWS_)                                                                               \
            {                                                                                                             \
                const int rc = rcN, eH = eHN, eD = eDN;                                                                   \
                rcN = rp[t + 1];                                                                                          \
                eHN = edgeH[min(t + 2, n + 1)];                                                                           \
                eDN = k == 0 ? DPX_NEG : (int)edgeD[min(t + 2, n + 1)];                                                   \
                aff_step<R, MODE, STORE, MASKED_, WHOLE_, TABLE>(st, t, lane, n, HASROWS_, match, mismatch, oe, e, eH, eD, rc, edgeH, edgeD, \
                                            hasNext, tile + (size_t)t * cs, storeLanes, a.rampLines, rsel);               \
            }
            const bool fast = (base + 64 * R <= m) && (n >= 64);
            const int storeLanes = (S == 1) ? store_lanes<R>(m) : 64;
            if (S == 1) {
                if (fast) {
                    int t = 0;
                    for (; t < 63; t++) DPX_AFF_STEP(true, true, true)
                    for (; t + 1 < n;) { DPX_AFF_STEP(false, true, true) t++; DPX_AFF_STEP(false, true, true) t++; } /* two steps per trip */
                    for (; t < n; t++) DPX_AFF_STEP(false, true, true)
                    for (; t < W; t++) DPX_AFF_STEP(true, true, true)
                } else {
                    for (int t = 0; t < W; t++) DPX_AFF_STEP(true, true, laneHasRows)
                }
            } else if (fast) { /* stripes share their ramp chunks: masked stores on the ramps */
                int t = 0;
                for (; t < 63; t++) DPX_AFF_STEP(true, false, true)
                for (; t + 1 < n;) { DPX_AFF_STEP(false, false, true) t++; DPX_AFF_STEP(false, false, true) t++; }
                for (; t < n; t++) DPX_AFF_STEP(false, false, true)
                for (; t < W; t++) DPX_AFF_STEP(true, false, true)
            } else {
                for (int t = 0; t < W; t++) DPX_AFF_STEP(true, false, laneHasRows)
            }
    #undef DPX_AFF_STEP
            if constexpr (LOCAL) fold_row_keys<R>(st.key, row0, nrows, bestv, bestrow, bestcol);
        }
}
    if constexpr (LOCAL) {
        sw_publish(a, p, lane, bestv, bestrow, bestcol);
        return;
    }
    const int lastBase = (S - 1) * 64 * R;
    const int lm = (m - 1 - lastBase) / R, rm = (m - 1 - lastBase) % R;
    if constexpr (SEMI) { /* row m's key is that of lane lm in the last stripe (on the rolling schedule too: a lane stops switching there, and
                           * its key starts again with every stripe) */
        if (lane == lm) asg_publish(a, p, m, st.key[0], o + m * e);
        return;
    }
    if (lane == lm) {
        int v = st.Hl[0];
#pragma unroll
        for (int r = 1; r < R; r++) v = (r == rm) ? st.Hl[r] : v;
        a.score[p] = v; /* scoringMemo[m][n] (:365) */
        a.endRow[p] = m;
        a.endCol[p] = n;
    }
