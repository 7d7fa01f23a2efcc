/* dpx_affine_lanes.inc -- body of the lane-packed affine-gap kernels, included by dpx_affine_kernels.hip inside k_affine_lanes (ANW, LOCAL = false)
 * k_asw_lanes (ASW, LOCAL = true) and k_asg_lanes (ASG, SEMI = true), for the reason given in dpx_affine_fill.inc, and by
 * dpx_scoretab_kernels.hip inside k_scoretab_lanes (TABLE = true: the diagonal term from the wave's LDS table image, as in
 * dpx_affine_fill.inc; the image sits behind the wave's reference area, a.ldsPerWave counts it).  In scope: `a`, R, STORE, LOCAL, SEMI,
 * TABLE and the global pointers tableG / codeOfG (null constants where TABLE is false). */
    constexpr int MODE = LOCAL ? 1 : (SEMI ? 2 : 0); /* aff_cells_g: ANW, ASW, ASG */
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    static_assert(R == 8, "one 8-row block per lane");
    constexpr int kPlane = 64 * kStageLine; /* bytes of one plane's lines */
    constexpr int kStageBytes = 3 * kPlane;
    constexpr int kStepElems = 3 * 512;     /* int16 elements of one chunk of the wave's stream (dpx_layout.h) */
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int w = blockIdx.x * (DPX_ALANES_THREADS / 64) + wv;
    if (w >= a.numPairs) return; /* wave-uniform; numPairs = number of wave descriptors */
    const LaneSlot sl = find_slot(a.waves + w, lane);
    const bool has = sl.has;
    const int p = sl.p, l = sl.l;
    const dpx_pair_dev pr = a.pairs[p];
    const int n = has ? pr.n : 0, m = has ? pr.m : 0;
    const int o = a.gapOpen, e = a.gapExtend, oe = o + e;
    const int matchG = (TABLE ? 0 : a.match) - oe, mismatchG = a.mismatch - oe; /* (TABLE: matchG is the frame's -(o+e) alone, aff_cells_g) */
    const unsigned char *ref = reinterpret_cast<const unsigned char *>(a.seq + pr.refIdx);
    const unsigned char *qry = reinterpret_cast<const unsigned char *>(a.seq + pr.qryIdx);

    unsigned char *tileL = smem + (size_t)wv * a.ldsPerWave;
    unsigned char *refl = tileL + (STORE ? kStageBytes : kLaneScratch) + sl.refOff;
    const unsigned char *refs = stage_bytes(refl, ref, n, l, max(sl.num, 1));
    [[maybe_unused]] unsigned char *img = nullptr;
    [[maybe_unused]] const unsigned char *codeL = nullptr;
    if constexpr (TABLE) { /* the wave's table image behind its reference area (a.ldsPerWave counts it); every slot's staged reference becomes
                            * codes, once, by the slot's own lanes */
        img = tileL + (a.ldsPerWave - (uint32_t)DPX_SUBST_IMAGE_BYTES);
        codeL = table_stage(img, tableG, codeOfG, lane);
        table_translate(const_cast<unsigned char *>(refs), n, l, max(sl.num, 1), codeL);
    }

    const int row0 = l * R;
    const int nrows = min(max(m - row0, 0), R);
    AffStateG<R> st;
    load_query_rows<R>(st.qc, qry, row0, nrows);
    if constexpr (TABLE) { /* the LDS addresses of the lane's query codes' columns of the transposed image (table_column), once (rows past m: some code, their cells are never read back) */
#pragma unroll
        for (int r = 0; r < R; r++) st.qc[r] = table_column(img, codeL, st.qc[r]);
    }
#pragma unroll
    for (int r = 0; r < R; r++) {
        st.Hoe[r] = (LOCAL ? 0 : o + (row0 + 1 + r) * e) + oe; /* H[i][0] = o + i*e (AffineNeedlemanWunsch.cpp:43-46); ASW: 0 */
        st.Ie[r] = DPX_NEG + e;                  /* virtual I[i][0] */
        st.key[r] = 0u;
    }
    st.dtopOe = ((LOCAL || row0 == 0) ? 0 : o + row0 * e) + oe; /* H[0][0] = 0 */
    st.DeLast = DPX_NEG + e;

    [[maybe_unused]] const int rsel = (m - 1) & (R - 1); /* ASG: the register of row m in the slot's lane (m-1)/8 */
    const int skew = l + sl.d; /* this lane runs column j = t - skew + 1 in step t; skew = lane (mod 8) */
    const int n8 = (n + 7) & ~7;
    const int LB = (int)dpx_tile8_row_blocks(m);
    /* routing, once: a lane's lines are complete in the steps skew + 7, skew + 15, ... <= n8 + skew - 1 (first | last << 16); every lane
     * keeps the words of the eight lanes of its group in registers */
    uint32_t rt[8];
    if constexpr (STORE) {
        const bool rowsHere = has && (LB - l) > 0;
        uint32_t *mine = reinterpret_cast<uint32_t *>(tileL + lane * kStageLine + 128);
        mine[0] = rowsHere ? ((uint32_t)(skew + 7) | ((uint32_t)(n8 + skew - 1) << 16)) : 0x00007FFFu; /* (never valid: first > last) */
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int k = 0; k < 8; k++) rt[k] = *reinterpret_cast<const uint32_t *>(tileL + ((lane & ~7) | k) * kStageLine + 128);
    }
    int16_t *waveBase = a.mat + (size_t)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(pr.matOff >> 32)) << 32) |
                                         (unsigned)__builtin_amdgcn_readfirstlane((int)(pr.matOff & 0xFFFFFFFFull)));
    const int steps = __builtin_amdgcn_readfirstlane(wave_max_i32(has ? (STORE ? n8 : n) + skew : 0));
    const unsigned char *rp = refs - skew;
    const unsigned nEff = nrows > 0 ? (unsigned)n : 0u;
    const int rpLast = n + skew; /* rp[rpLast] = refs[n]: inside the slack of stage_bytes */
    unsigned char *putPtr = tileL + lane * kStageLine; /* + plane * kPlane + (t & 7) * 16 */
    const unsigned char *fetchPtr[8]; /* piece lane % 8 of the line of lane k of this lane's group, rotated by its owner (see k_linear_lanes) */
#pragma unroll
    for (int k = 0; k < 8; k++) fetchPtr[k] = tileL + ((lane & ~7) | k) * kStageLine + (((lane + k) & 7) << 4);
    u32x4 pend[3];
    bool pendOk = false;
    int16_t *pendDst = nullptr;
    int bordOe = ((LOCAL || SEMI) ? 0 : o + (1 - skew) * e) + oe; /* first lane of a slot: H[0][j] + (o+e), j = t - skew + 1 (ASW / ASG: H[0][j] = 0) */
    int rcN = rp[0];
    auto flush = [&]() __attribute__((always_inline)) {
        if (pendOk) {
#pragma unroll
            for (int pl = 0; pl < 3; pl++) stream_store(reinterpret_cast<u32x4 *>(pendDst + (pl << 9)), pend[pl]);
        }
    };
    auto pack8 = [](const int (&v)[R]) __attribute__((always_inline)) -> u32x4 {
        u32x4 x = {pack_lo16(v[0], v[1]), pack_lo16(v[2], v[3]), pack_lo16(v[4], v[5]), pack_lo16(v[6], v[7])};
        return x;
    };
    auto lane_step = [&](const int t, auto kTag) __attribute__((always_inline)) {
        constexpr int K = decltype(kTag)::value; /* t & 7 */
        const int tms = t - skew;
        const int rc = rcN;
        rcN = rp[min(t + 1, rpLast)];
        const int shH = wave_shr1(st.Hoe[R - 1], 0), shD = wave_shr1(st.DeLast, 0);
        const int upHoe = (l == 0) ? bordOe : shH;          /* row-0 border H[0][j] = o + j*e (:50-53) */
        const int upDe = (l == 0) ? (DPX_NEG + e) : shD;    /* virtual D[0][j] */
        if constexpr (!LOCAL && !SEMI) bordOe += e;
        if ((unsigned)tms < nEff) {
            int Hv[R], Iv[R], Dv[R];
            aff_cells_g<R, MODE, TABLE>(st, upHoe, upDe, rc, matchG, mismatchG, oe, e, Hv, Iv, Dv, 0xFFFEu - (unsigned)tms, rsel);
            if constexpr (STORE) {
                *reinterpret_cast<u32x4 *>(putPtr + 0 * kPlane + (K << 4)) = pack8(Hv);
                *reinterpret_cast<u32x4 *>(putPtr + 1 * kPlane + (K << 4)) = pack8(Iv);
                *reinterpret_cast<u32x4 *>(putPtr + 2 * kPlane + (K << 4)) = pack8(Dv);
            }
        }
        if constexpr (STORE) {
            flush();
            constexpr int O = (K + 1) & 7; /* the owners of the lines that are complete now */
            const uint32_t r = rt[O];
            pendOk = (uint32_t)t >= (r & 0xFFFFu) && (uint32_t)t <= (r >> 16);
            pendDst = waveBase + (size_t)t * kStepElems + (lane << 3);
#pragma unroll
            for (int pl = 0; pl < 3; pl++) pend[pl] = *reinterpret_cast<const u32x4 *>(fetchPtr[O] + pl * kPlane);
        }
    };
    {
        int t = 0;
        for (; t + 8 <= steps; t += 8) {
            lane_step(t + 0, std::integral_constant<int, 0>{}); lane_step(t + 1, std::integral_constant<int, 1>{});
            lane_step(t + 2, std::integral_constant<int, 2>{}); lane_step(t + 3, std::integral_constant<int, 3>{});
            lane_step(t + 4, std::integral_constant<int, 4>{}); lane_step(t + 5, std::integral_constant<int, 5>{});
            lane_step(t + 6, std::integral_constant<int, 6>{}); lane_step(t + 7, std::integral_constant<int, 7>{});
        }
        if (t + 0 < steps) lane_step(t + 0, std::integral_constant<int, 0>{});
        if (t + 1 < steps) lane_step(t + 1, std::integral_constant<int, 1>{});
        if (t + 2 < steps) lane_step(t + 2, std::integral_constant<int, 2>{});
        if (t + 3 < steps) lane_step(t + 3, std::integral_constant<int, 3>{});
        if (t + 4 < steps) lane_step(t + 4, std::integral_constant<int, 4>{});
        if (t + 5 < steps) lane_step(t + 5, std::integral_constant<int, 5>{});
        if (t + 6 < steps) lane_step(t + 6, std::integral_constant<int, 6>{});
    }
    if constexpr (STORE) flush();
    if constexpr (LOCAL) {
        /* first strict maximum in row-major order over the slot's lanes (k_linear_lanes): rows past the slot's query end stay out of the
         * keys (nrows), the slot's first lane scans its lanes' (score, row, column) in the lane scratch (the line stage, dead by now) */
        int bestv = 0, bestrow = 0, bestcol = 0;
        fold_row_keys<R>(st.key, row0, nrows, bestv, bestrow, bestcol);
        int *mine = reinterpret_cast<int *>(tileL + lane * 16);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        mine[0] = bestv; mine[1] = bestrow; mine[2] = bestcol;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (has && l == 0) {
            for (int k = 1; k < sl.num; k++) {
                const int *ot = reinterpret_cast<const int *>(tileL + (lane + k) * 16);
                if (ot[0] > bestv) { bestv = ot[0]; bestrow = ot[1]; bestcol = ot[2]; }
            }
            a.score[p] = bestv; a.endRow[p] = bestv > 0 ? bestrow : 0; a.endCol[p] = bestv > 0 ? bestcol : 0;
        }
        return;
    }
    const int lm = (m - 1) / R, rm = (m - 1) % R;
    if constexpr (SEMI) { /* row m's key: register rm of the slot's lane (m-1)/8 (the host keeps pairs without cells off this kernel) */
        if (has && l == lm) asg_publish(a, p, m, st.key[0], o + m * e);
        return;
    }
    if (has && l == lm) {
        int v = st.Hoe[0];
#pragma unroll
        for (int r = 1; r < R; r++) v = (r == rm) ? st.Hoe[r] : v;
        a.score[p] = v - oe; /* scoringMemo[m][n] (:365); the state is H + (o+e) */
        a.endRow[p] = m;
        a.endCol[p] = n;
    }
