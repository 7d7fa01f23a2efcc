// BandedAffineNeedlemanWunsch.h -- banded global alignment with affine (Gotoh) gaps on the MI355X engine (DPX_ALGO_BANW, include/dpx_align.h):
// what a read mapper runs between two anchors.  The reference has no such class: AffineNeedlemanWunsch's constructor and shape plus
// BandedSmithWaterman's band argument (cells with |i-j| <= band-1, borders included; everything else is -infinity).  The pair must
// satisfy |m - n| <= band-1, or the library refuses the batch.  The fill runs in k_banw_fill, the walk in the device traceback; it
// prints AffineNeedlemanWunsch's block.
#pragma once
#include <deque>
#include <iomanip>
#include <iostream>
#include <vector>
#include "SequenceAligner.h"
#include "debug.h"
#include "printLock.h"
#include "DpxPair.h"

class BandedAffineNeedlemanWunsch : public SequenceAligner {
  private:
    int matchWeight;
    int mismatchWeight;
    int gapOpenWeight;
    int gapExtendWeight;
    int bandWidth;
    DpxPairResult gpu;

  public:
    BandedAffineNeedlemanWunsch(const std::string inputReference, const std::string inputQuery, const int pairNum,
                              const int matchWeight, const int mismatchWeight, const int gapOpenWeight, const int gapExtendWeight,
                              const int bandWidth)
        : SequenceAligner(inputReference, inputQuery, pairNum), matchWeight(matchWeight), mismatchWeight(mismatchWeight),
          gapOpenWeight(gapOpenWeight), gapExtendWeight(gapExtendWeight), bandWidth(bandWidth) {}

    void init_matrix();
    void print_matrix();
    void score_matrix();
    void backtrack(); // prints the result block (the path whatever the score's sign)
    void align();
    void print_results();
};
