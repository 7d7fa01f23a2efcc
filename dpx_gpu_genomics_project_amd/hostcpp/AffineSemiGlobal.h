// AffineSemiGlobal.h -- semi-global alignment with affine (Gotoh) gaps on the MI355X engine (DPX_ALGO_ASG, include/dpx_align.h): the whole
// query against the stretch of the reference that fits it best.  The reference has no such class: same constructor and shape as
// AffineNeedlemanWunsch; the fill runs in k_asg_fill / k_asg_lanes, the walk (ANW's three states, stopping on row 0) in the device
// traceback; it prints the header and the three lines whatever the sign of the score.
#pragma once
#include <deque>
#include <iomanip>
#include <iostream>
#include <vector>
#include "SequenceAligner.h"
#include "debug.h"
#include "printLock.h"
#include "DpxPair.h"

class AffineSemiGlobal : public SequenceAligner {
  private:
    int matchWeight;
    int mismatchWeight;
    int gapOpenWeight;
    int gapExtendWeight;
    DpxPairResult gpu;

  public:
    AffineSemiGlobal(const std::string inputReference, const std::string inputQuery, const int pairNum,
                          const int matchWeight, const int mismatchWeight, const int gapOpenWeight, const int gapExtendWeight)
        : SequenceAligner(inputReference, inputQuery, pairNum), matchWeight(matchWeight), mismatchWeight(mismatchWeight),
          gapOpenWeight(gapOpenWeight), gapExtendWeight(gapExtendWeight) {}

    void init_matrix();
    void print_matrix();
    void score_matrix();
    void backtrack(); // prints the result block (the path whatever the score's sign; three empty lines only for an empty query)
    void align();
    void print_results();
};
