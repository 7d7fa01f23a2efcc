/* dpx_affine_dir.inc -- body of the affine-gap direction fills, included by dpx_dir_kernels.hip inside k_affine_dir (ANW, LOCAL = false)
 * k_asw_dir (ASW, LOCAL = true) and k_asg_dir (ASG, SEMI = true), for the reason given in dpx_affine_fill.inc, and by
 * dpx_dirtab_kernels.hip inside k_dirtab_fill (TABLE = true: the diagonal term is table[codeOf[reference byte] * 32 + codeOf[query
 * byte]], dpx_batch_set_direction_table).  In scope: `a`, R, GLOBAL, LOCAL, SEMI, TABLE and the table's dpx_table_ref `tref` (null constants
 * where TABLE is false: nothing of the table survives in those kernels). */
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int G = 32 / R;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int slot = blockIdx.x * (int)a.wavesPerBlock + wv; /* in this launch (the scratch area's index) */
    if (a.firstSlot + slot >= a.numPairs) return;
    const int p = a.order ? a.order[a.firstSlot + slot] : a.firstSlot + slot;
    const dpx_pair_dev pr = a.pairs[p];
    const int n = pr.n, m = pr.m;
    [[maybe_unused]] const int match = a.match, mismatch = a.mismatch;
    const int o = a.gapOpen, e = a.gapExtend, oe = o + e;

    if (m <= 0 || n <= 0) {
        if (lane == 0) { /* H[m][n] on the border: 0 at the origin, else o + len*e (AffineNeedlemanWunsch.cpp:43-53); ASW: 0 at (0, 0);
                          * ASG: 0 at (0, 0) for an empty query, else o + m*e at (m, 0) */
            const int len = m <= 0 ? max(n, 0) : m;
            a.score[p] = (LOCAL || len <= 0 || (SEMI && m <= 0)) ? 0 : o + len * e;
            a.endRow[p] = LOCAL ? 0 : max(m, 0);
            a.endCol[p] = (LOCAL || SEMI) ? 0 : max(n, 0);
        }
        return;
    }
    const unsigned char *ref = reinterpret_cast<const unsigned char *>(a.seq + pr.refIdx);
    const unsigned char *qry = reinterpret_cast<const unsigned char *>(a.seq + pr.qryIdx);
    unsigned char *my;
    if constexpr (GLOBAL) my = a.scratch + (size_t)slot * a.ldsPerWave;
    else my = smem + (size_t)wv * a.ldsPerWave; /* (TABLE: a.ldsPerWave counts the image behind the staged reference) */
    int32_t *edgeH = reinterpret_cast<int32_t *>(my);
    int32_t *edgeD = reinterpret_cast<int32_t *>(my + a.ldsEdge2Off);
    const unsigned char *refl = stage_bytes(my + a.ldsRefOff + 64, ref, n, lane, 64) - 64;
    for (int x = lane; x <= n + 1; x += 64) { edgeH[x] = (LOCAL || SEMI) ? 0 : o + x * e; edgeD[x] = DPX_NEG; } /* H[0][j] (:50-53; ASW / ASG 0), virtual D[0][j] */
    [[maybe_unused]] const signed char *tabL = nullptr;
    [[maybe_unused]] const unsigned char *codeL = nullptr;
    if constexpr (TABLE) { /* the wave's own table image (dpx_table_dev.hpp) behind its LDS slice, or -- GLOBAL -- the only thing it keeps in LDS */
        unsigned char *img = GLOBAL ? smem + (size_t)wv * DPX_SUBST_IMAGE_BYTES : my + (a.ldsPerWave - (uint32_t)DPX_SUBST_IMAGE_BYTES);
        tabL = reinterpret_cast<const signed char *>(img);
        codeL = table_stage_rows(img, tref, lane);
        /* the staged reference becomes codes, once (the walk and the export read the caller's bytes from a.seq, never the stage) */
        unsigned char *sref = const_cast<unsigned char *>(refl) + 64;
        /* table_translate's loop, written out: the stage is in global memory when GLOBAL, and through the call the nine LDS instantiations
         * compile to other operand orders in their cell loop */
        if constexpr (GLOBAL) __threadfence_block(); /* (a lane translates bytes that other lanes staged) */
        for (int x = lane; x < n; x += 64) sref[x] = codeL[sref[x]];
        if constexpr (!GLOBAL) dpx_table::wave_publish_lds();
    }
    if constexpr (GLOBAL) __threadfence_block();

    const int S = dpx_tiled_stripes(m, R);
    const int Wp = (int)dpx_dir_stripe_steps(n, R);
    const size_t cs = (size_t)pr.chunkStride * 2u;
    unsigned char *cbase = a.codes + (size_t)pr.matOff * 2u + (size_t)lane * 16u;

    int Hl[R], Il[R], qc[R];
    [[maybe_unused]] int bestv = 0, bestrow = 0, bestcol = 0; /* ASW: the lane's first strict maximum */
    [[maybe_unused]] int bv[R], bc[R];                         /* ASW: per row, best H and its first column (int32: no 16-bit keys); ASG: bv[0] / bc[0], of register rsel */
    [[maybe_unused]] const int rsel = (m - 1) % R;             /* ASG: the register of row m in the lane that owns it */
    for (int k = 0; k < S; k++) {
        const int row0 = k * 64 * R + lane * R;
        const int nrows = min(max(m - row0, 0), R);
        const bool hasRows = nrows > 0, hasNext = k + 1 < S;
#pragma unroll
        for (int r = 0; r < R; r++) {
            if constexpr (TABLE) qc[r] = r < nrows ? (int)codeL[qry[row0 + r]] : 0; /* the lane's query codes, once per stripe (rows past m: any code, never read back) */
            else qc[r] = r < nrows ? (int)qry[row0 + r] : 0x100;
            Hl[r] = LOCAL ? 0 : o + (row0 + 1 + r) * e; /* H[i][0] = o + i*e (:43-46); ASW: 0 */
            Il[r] = DPX_NEG;                /* virtual I[i][0] */
            if constexpr (LOCAL) { bv[r] = 0; bc[r] = 0; }
        }
        if constexpr (SEMI) { bv[0] = o + m * e; bc[0] = 0; } /* ASG: row m's column-0 border takes part, and wins a tie (read from the lane that owns row m) */
        int dBot = DPX_NEG;                 /* D of the lane's bottom row, for the lane below */
        int dtop = (LOCAL || row0 == 0) ? 0 : o + row0 * e;
        const unsigned char *rp = refl + 64 - lane;
        int rcN = rp[0];
        int eHN = edgeH[1], eDN = edgeD[1];
        unsigned char *dst = cbase + (size_t)k * (size_t)(Wp / G) * cs;
        for (int t0 = 0; t0 < Wp; t0 += G) {
            uint32_t acc[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int q = 0; q < G; q++) {
                const int t = t0 + q;
                const int rc = rcN, eH = eHN, eD = eDN;
                rcN = rp[t + 1];
                eHN = edgeH[min(t + 2, n + 1)];
                eDN = edgeD[min(t + 2, n + 1)];
                const int upH = wave_shr1(Hl[R - 1], eH);
                const int upD = wave_shr1(dBot, eD);
                const int j = t - lane + 1;
                uint32_t w[2] = {0u, 0u};
                if (hasRows && j >= 1 && j <= n) {
                    int uH = upH, uD = upD, d = dtop;
                    [[maybe_unused]] const signed char *trow = nullptr;
                    if constexpr (TABLE) trow = tabL + (rc << 5); /* the table's row is the reference code */
#pragma unroll
                    for (int r = 0; r < R; r++) {
                        const int lH = Hl[r];
                        int s;
                        if constexpr (TABLE) s = trow[qc[r]]; /* one signed byte from LDS */
                        else s = (qc[r] == rc) ? match : mismatch;
                        const int dOpen = uH + oe, dExt = uD + e; /* :185-197 */
                        const int Dn = max(dOpen, dExt);
                        const int iOpen = lH + oe, iExt = Il[r] + e; /* :201-213 */
                        const int In = max(iOpen, iExt);
                        const int mm = d + s; /* :216-236 */
                        const int v = max(Dn, mm);
                        int h = max(In, v);
                        uint32_t code = In >= v ? 3u : (Dn >= mm ? 2u : 1u);
                        if constexpr (LOCAL) { /* ASW: H = max(0, best); move 0 where H == 0 (the walk stops there) */
                            h = max(h, 0);
                            if (h == 0) code = 0u;
                            if (h > bv[r]) { bv[r] = h; bc[r] = j; } /* first strict maximum of the row */
                        }
                        code |= (iOpen >= iExt ? 0u : 4u) | (dOpen >= dExt ? 0u : 8u);
                        w[(r * 4) >> 5] |= code << ((r * 4) & 31);
                        d = lH;
                        uH = h;
                        uD = Dn;
                        Hl[r] = h;
                        Il[r] = In;
                    }
                    dBot = uD;
                    dtop = upH;
                    if constexpr (SEMI) { /* the first maximum of ONE row: register rsel (a select chain on the wave-uniform rsel) */
                        int hm = Hl[0];
#pragma unroll
                        for (int r = 1; r < R; r++) hm = (r == rsel) ? Hl[r] : hm;
                        if (hm > bv[0]) { bv[0] = hm; bc[0] = j; }
                    }
                    if (hasNext && lane == 63) { edgeH[j] = Hl[R - 1]; edgeD[j] = dBot; }
                }
                dir_put<R>(acc, q, w[0], w[1]);
            }
            dir_store(dst + (size_t)(t0 / G) * cs, acc);
        }
        if constexpr (GLOBAL) __threadfence_block();
        if constexpr (LOCAL) {
#pragma unroll
            for (int r = 0; r < R; r++)
                if (r < nrows && bv[r] > bestv) { bestv = bv[r]; bestrow = row0 + 1 + r; bestcol = bc[r]; }
        }
    }
    if constexpr (LOCAL) { /* first strict maximum in row-major order (k_linear_dir) */
        const unsigned long long mine = ((unsigned long long)(unsigned)bestv << 32) | (unsigned)(0x7FFFFFFF - bestrow);
        const unsigned long long top = wave_max_u64(mine);
        if ((int)(top >> 32) == 0) {
            if (lane == 0) { a.score[p] = 0; a.endRow[p] = 0; a.endCol[p] = 0; }
        } else if (mine == top) {
            a.score[p] = bestv;
            a.endRow[p] = bestrow;
            a.endCol[p] = bestcol;
        }
        return;
    }
    const int lastBase = (S - 1) * 64 * R;
    const int lm = (m - 1 - lastBase) / R, rm = (m - 1 - lastBase) % R;
    if constexpr (SEMI) { /* row m: register rm of lane lm of the last stripe */
        if (lane == lm) {
            a.score[p] = bv[0];
            a.endRow[p] = m;
            a.endCol[p] = bc[0];
        }
        return;
    }
    if (lane == lm) {
        int v = Hl[0];
#pragma unroll
        for (int r = 1; r < R; r++) v = (r == rm) ? Hl[r] : v;
        a.score[p] = v; /* scoringMemo[m][n] (:365) */
        a.endRow[p] = m;
        a.endCol[p] = n;
    }
