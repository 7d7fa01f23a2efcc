// BandedAffineExtension.h -- banded extension alignment with affine (Gotoh) gaps on the MI355X engine (DPX_ALGO_BAXT, include/dpx_align.h):
// what a read mapper runs past its first and last anchor.  The reference has no such class: BandedAffineNeedlemanWunsch's constructor and
// shape.  The alignment leaves from (0, 0), stays in the band (cells with |i-j| <= band-1, borders included) and ends on the first cell
// that holds the maximum of H; any pair of lengths is accepted.  The fill runs in k_baxt_fill, the walk in the device traceback; it
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

class BandedAffineExtension : public SequenceAligner {
  private:
    int matchWeight;
    int mismatchWeight;
    int gapOpenWeight;
    int gapExtendWeight;
    int bandWidth;
    DpxPairResult gpu;

  public:
    BandedAffineExtension(const std::string inputReference, const std::string inputQuery, const int pairNum,
                        const int matchWeight, const int mismatchWeight, const int gapOpenWeight, const int gapExtendWeight,
                        const int bandWidth)
        : SequenceAligner(inputReference, inputQuery, pairNum), matchWeight(matchWeight), mismatchWeight(mismatchWeight),
          gapOpenWeight(gapOpenWeight), gapExtendWeight(gapExtendWeight), bandWidth(bandWidth) {}

    void init_matrix();
    void print_matrix();
    void score_matrix();
    void backtrack(); // prints the result block (the path from the end cell back to the anchor; empty lines when the score is 0)
    void align();
    void print_results();
};
