// BandedAffineSmithWaterman.h -- banded local alignment with affine (Gotoh) gaps on the MI355X engine (DPX_ALGO_BASW, include/dpx_align.h).
// The reference has no such class: AffineSmithWaterman's constructor and shape plus BandedSmithWaterman's band argument (cells with
// |i-j| <= band-1; everything else reads H = 0, I = D = -infinity).  The fill runs in k_basw_fill, the walk in the device traceback;
// it prints LinearSmithWaterman's block.
#pragma once
#include <deque>
#include <iomanip>
#include <iostream>
#include <vector>
#include "SequenceAligner.h"
#include "debug.h"
#include "printLock.h"
#include "DpxPair.h"

class BandedAffineSmithWaterman : public SequenceAligner {
  private:
    int matchWeight;
    int mismatchWeight;
    int gapOpenWeight;
    int gapExtendWeight;
    int bandWidth;
    DpxPairResult gpu;

  public:
    BandedAffineSmithWaterman(const std::string inputReference, const std::string inputQuery, const int pairNum,
                              const int matchWeight, const int mismatchWeight, const int gapOpenWeight, const int gapExtendWeight,
                              const int bandWidth)
        : SequenceAligner(inputReference, inputQuery, pairNum), matchWeight(matchWeight), mismatchWeight(mismatchWeight),
          gapOpenWeight(gapOpenWeight), gapExtendWeight(gapExtendWeight), bandWidth(bandWidth) {}

    void init_matrix();
    void print_matrix();
    void score_matrix();
    void backtrack(); // prints the result block (LinearSmithWaterman's layout: three empty lines for a zero score)
    void align();
    void print_results();
};
