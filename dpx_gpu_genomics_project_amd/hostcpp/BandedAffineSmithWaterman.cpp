#include "BandedAffineSmithWaterman.h"

#include <cstdio>

void BandedAffineSmithWaterman::init_matrix() { gpu = DpxPairResult(); }

void BandedAffineSmithWaterman::print_matrix() {
    if (gpu.H.empty())
        dpxAlignPair(5 /* DPX_ALGO_BASW */, reference_str, query_str, matchWeight, mismatchWeight, gapOpenWeight, gapExtendWeight, bandWidth, true, gpu);
    printf("[Scoring Matrix]\n");
    dpxPrintScoreMatrix(reference_str, query_str, gpu.H);
    printf("[Query Insertion Matrix]\n");
    dpxPrintScoreMatrix(reference_str, query_str, gpu.I);
    printf("[Query Deletion Matrix]\n");
    dpxPrintScoreMatrix(reference_str, query_str, gpu.D);
}

void BandedAffineSmithWaterman::score_matrix() {
#ifdef PRINT_MATRIX
    const bool wantMatrix = true;
#else
    const bool wantMatrix = false;
#endif
    dpxAlignPair(5 /* DPX_ALGO_BASW */, reference_str, query_str, matchWeight, mismatchWeight, gapOpenWeight, gapExtendWeight, bandWidth,
                 wantMatrix, gpu);
}

void BandedAffineSmithWaterman::backtrack() {
#ifdef USE_THREADS
    printLock();
#endif
    printf("%d | %d\n%s\n%s\n%s\n", pairNum, gpu.score, /* (score 0: the device lines are empty -- three empty lines) */ gpu.refLine.c_str(), gpu.relLine.c_str(), gpu.qryLine.c_str());
#ifdef USE_THREADS
    printUnlock(); // (no flush per block: stdio orders printf and the drivers' cout lines by itself, and 4000 one-block write() calls were 8 % of the run)
#endif
}

void BandedAffineSmithWaterman::align() {
    init_matrix();
#ifdef PRINT_MATRIX
    print_matrix();
#endif
    score_matrix();
#ifdef PRINT_MATRIX
    print_matrix();
#endif
    backtrack();
}

void BandedAffineSmithWaterman::print_results() {}
