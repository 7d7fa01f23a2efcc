// AffineSmithWaterman.h -- local alignment with affine (Gotoh) gaps on the MI355X engine (DPX_ALGO_ASW, include/dpx_align.h).
// The reference has no such class: same constructor and shape as AffineNeedlemanWunsch; the fill runs in k_asw_fill / k_asw_lanes,
// the walk (ANW's three states, stopping where H = 0) in the device traceback; it prints LinearSmithWaterman's block.
#pragma once
#include <deque>
#include <iomanip>
#include <iostream>
#include <vector>
#include "SequenceAligner.h"
#include "debug.h"
#include "printLock.h"
#include "DpxPair.h"

class AffineSmithWaterman : public SequenceAligner {
  private:
    int matchWeight;
    int mismatchWeight;
    int gapOpenWeight;
    int gapExtendWeight;
    DpxPairResult gpu;

  public:
    AffineSmithWaterman(const std::string inputReference, const std::string inputQuery, const int pairNum,
                          const int matchWeight, const int mismatchWeight, const int gapOpenWeight, const int gapExtendWeight)
        : SequenceAligner(inputReference, inputQuery, pairNum), matchWeight(matchWeight), mismatchWeight(mismatchWeight),
          gapOpenWeight(gapOpenWeight), gapExtendWeight(gapExtendWeight) {}

    void init_matrix();
    void print_matrix();
    void score_matrix();
    void backtrack(); // prints the result block (LinearSmithWaterman's layout: three empty lines for a zero score)
    void align();
    void print_results();
};
