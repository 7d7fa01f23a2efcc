/*
 * plan_tool -- runs the batch planner (csrc/dpx_plan.cpp) on one case from stdin and prints what it decided.  No GPU, no libdpxalign.so.
 *
 * Input, one case:
 *     params <algo> <match> <mismatch> <gapOpen> <gapExtend> <band>
 *     flags <flags>
 *     knobs <DPX_R> <DPX_PACKED> <DPX_LANES> <DPX_LANES_PK> <DPX_SPLIT> <DPX_ROW_TAGS> <DPX_RAMP_LINES> <DPX_WPB> <DPX_GROUP> <DPX_TB_WALK>
 *           (the values refresh_knobs() would read: 0 for an unset DPX_R / DPX_WPB / DPX_GROUP, -1 for the others)
 *     input <packed2: 0|1> <numBytes> <firstPair> <numPairs>
 *     mode <zdrop> <endBonus> <substAlphabet>                      (optional: what a batch can change after its creation, as
 *           dpx_batch_set_extension / _set_substitution / _set_extension_table leave it; absent: -1 -1 0.  The setters' own
 *           refusals are not applied: the planner is asked what such a batch would run)
 *     gap2 <gapOpen2> <gapExtend2>                                 (optional, after the mode line if there is one: the second gap piece
 *           of a DPX_TWO_PIECE_GAPS / DPX_LOCAL_TWO_PIECE_GAPS plan as dpx_batch_set_second_gap leaves it; absent: piece 1)
 *     <referenceIdx> <referenceSize> <queryIdx> <querySize>        (firstPair + numPairs lines)
 *
 * Output, one line: "status=<n>", then for a refusal " err=<text>" when there is one, else dpx_batch_describe()'s text up to the pool
 * fields, " info=<numPairs>,<cells>,<matrixBytes>,<algorithmicBytes>" (dpx_batch_info), " state=<16 hex digits>" and, only when a mode
 * line was given, " walk=<family>:<mode>": the traceback's family (plain, dir, basw, banw, subst, bdir, bd2, bdl, lb2) and walk (0, 1 or 2) of
 * dpx_plan_route, which describe's traceback= shows for the banded affine kernels only.
 *
 * state is FNV-1a 64 over, in this order (integers as 8 little-endian bytes, sign-extended):
 *   1. the number of pairs, then of every dpx_pair_dev: refIdx, n, qryIdx, m, matOff, chunkStride, lanes, rows
 *   2. count and entries of singles; of couples; count of waves and their bytes; count and entries of tbOff
 *   3. seqLo, seqHi, R, kernelAlgo, dirs, bandDirs, packed, split, lanePacked, lanesPk, splitWaves, splitLds, ldsBytes, pkLdsBytes, dirScratch
 *   4. of args, then pkArgs: numPairs, match, mismatch, gapOpen, gapExtend, band, ldsPerWave, wavesPerBlock, ldsEdge2Off, ldsRefOff,
 *      ldsQryOff, ldsBufStride, rowTags, rampLines; of dirArgs: numPairs, match, mismatch, gapOpen, gapExtend, ldsPerWave, wavesPerBlock,
 *      ldsEdge2Off, ldsRefOff, firstSlot
 */
#include <cstdio>
#include <string>
#include <vector>

#include "../csrc/dpx_plan.h"

namespace {
struct Fnv {
    uint64_t h = 1469598103934665603ull;
    void u64(uint64_t v) { for (int k = 0; k < 8; k++) { h ^= (v >> (8 * k)) & 0xffu; h *= 1099511628211ull; } }
    void i64(long long v) { u64((uint64_t)v); }
    void bytes(const void *p, size_t n) { for (size_t k = 0; k < n; k++) { h ^= ((const unsigned char *)p)[k]; h *= 1099511628211ull; } }
};

uint64_t plan_state(const dpx_plan &b) {
    Fnv f;
    f.u64(b.pairs.size());
    for (const dpx_pair_dev &pd : b.pairs) { f.i64(pd.refIdx); f.i64(pd.n); f.i64(pd.qryIdx); f.i64(pd.m); f.u64(pd.matOff); f.u64(pd.chunkStride); f.u64(pd.lanes); f.u64(pd.rows); }
    f.u64(b.singles.size()); for (int32_t v : b.singles) f.i64(v);
    f.u64(b.couples.size()); for (int32_t v : b.couples) f.i64(v);
    f.u64(b.waves.size()); f.bytes(b.waves.data(), b.waves.size() * sizeof(dpx_wave_desc));
    f.u64(b.tbOff.size()); for (uint64_t v : b.tbOff) f.u64(v);
    f.u64(b.seqLo); f.u64(b.seqHi); f.i64(b.R); f.i64(b.kernelAlgo);
    f.u64(b.dirs); f.u64(b.bandDirs); f.u64(b.packed); f.u64(b.split); f.u64(b.lanePacked); f.u64(b.lanesPk);
    f.i64(b.splitWaves); f.u64(b.splitLds); f.u64(b.ldsBytes); f.u64(b.pkLdsBytes); f.u64(b.dirScratch);
    for (const dpx_fill_args *x : {&b.args, &b.pkArgs}) {
        f.i64(x->numPairs); f.i64(x->match); f.i64(x->mismatch); f.i64(x->gapOpen); f.i64(x->gapExtend); f.i64(x->band);
        f.u64(x->ldsPerWave); f.u64(x->wavesPerBlock); f.u64(x->ldsEdge2Off); f.u64(x->ldsRefOff); f.u64(x->ldsQryOff); f.u64(x->ldsBufStride);
        f.i64(x->rowTags); f.i64(x->rampLines);
    }
    const dpx_dir_args &d = b.dirArgs;
    f.i64(d.numPairs); f.i64(d.match); f.i64(d.mismatch); f.i64(d.gapOpen); f.i64(d.gapExtend);
    f.u64(d.ldsPerWave); f.u64(d.wavesPerBlock); f.u64(d.ldsEdge2Off); f.u64(d.ldsRefOff); f.i64(d.firstSlot);
    return f.h;
}
} // namespace

int main() {
    dpx_params prm{};
    unsigned flags = 0;
    Knobs kn;
    int packed2 = 0;
    size_t numBytes = 0, firstPair = 0, numPairs = 0;
    if (scanf(" params %d %d %d %d %d %d", &prm.algo, &prm.match, &prm.mismatch, &prm.gapOpen, &prm.gapExtend, &prm.band) != 6 ||
        scanf(" flags %u", &flags) != 1 ||
        scanf(" knobs %d %d %d %d %d %d %d %d %d %d", &kn.rowsPerLane, &kn.packed, &kn.lanes, &kn.lanesPk, &kn.split, &kn.rowTags, &kn.rampLines,
              &kn.wavesPerBlock, &kn.group, &kn.tbWalk) != 10 ||
        scanf(" input %d %zu %zu %zu", &packed2, &numBytes, &firstPair, &numPairs) != 4) {
        fprintf(stderr, "plan_tool: malformed case header\n");
        return 2;
    }
    int zdrop = -1, endBonus = -1, substAlphabet = 0;
    const bool mode = scanf(" mode %d %d %d", &zdrop, &endBonus, &substAlphabet) == 3; /* (a pair line stops the match at its first character) */
    if (!mode) { zdrop = endBonus = -1; substAlphabet = 0; }
    int gapOpen2 = 0, gapExtend2 = 0;
    const bool gap2 = scanf(" gap2 %d %d", &gapOpen2, &gapExtend2) == 2; /* (as dpx_batch_set_second_gap leaves a two-piece plan) */
    std::vector<dpx_seq_pair> pairs(firstPair + numPairs);
    for (dpx_seq_pair &sp : pairs)
        if (scanf("%d %d %d %d", &sp.referenceIdx, &sp.referenceSize, &sp.queryIdx, &sp.querySize) != 4) {
            fprintf(stderr, "plan_tool: malformed pair line\n");
            return 2;
        }
    dpx_plan plan;
    std::string err;
    int rc = validate_params(&prm);
    if (rc == DPX_OK) rc = dpx_plan_batch(prm, pairs.data(), firstPair, numPairs, numBytes, packed2 != 0, flags, kn, plan, err);
    if (rc != DPX_OK) {
        printf("status=%d%s%s\n", rc, err.empty() ? "" : " err=", err.c_str());
        return 0;
    }
    if (gap2 && plan.twoPiece) { plan.gapOpen2 = gapOpen2; plan.gapExtend2 = gapExtend2; }
    char text[4096];
    dpx_plan_describe(plan, kn.tbWalk, zdrop, endBonus, substAlphabet, text, sizeof text);
    printf("status=0 %s info=%zu,%llu,%llu,%llu state=%016llx", text, plan.numPairs, (unsigned long long)plan.cells,
           (unsigned long long)(plan.matElems * sizeof(int16_t)), (unsigned long long)plan.algBytes, (unsigned long long)plan_state(plan));
    if (mode) {
        static const char *const family[] = {"plain", "dir", "basw", "banw", "subst", "bdir", "bd2", "bdl", "lb2"}; /* dpx_walk_family */
        const dpx_route r = dpx_plan_route(plan, kn.tbWalk, zdrop, endBonus, substAlphabet);
        printf(" walk=%s:%d", family[r.walk], r.walkMode);
    }
    printf("\n");
    return 0;
}
