/*
 * dpx_bdlt_kernels.hip -- local band-direction batches (DPX_KEEP_LOCAL_BAND_DIRECTIONS) of BSW and BASW under
 * dpx_batch_set_local_direction_table for gfx950: the fill, k_bdlt_fill<C, PB, AFFINE>, and nothing else.  The walk and the export are
 * dpx_bdl_kernels.hip's (k_bdl_traceback follows stored codes and never scores a cell; the relation line and the H plane's MATCH /
 * MISMATCH are byte equality whatever scored the cell).
 *
 * The kernel is k_bdl_fill's with one difference: the diagonal term of a cell is table[(codeOf[ref byte] << 5) + codeOf[qry byte]]
 * instead of match / mismatch by byte equality.  The step is the shared bdl_step of dpx_bdl_dev.hpp with TABLE = true; the frame,
 * dpx_banddir_fill.inc, is included in its EXT form with TABLE = true and no scan, so it stages the 1280-byte table image into the
 * wave's LDS slice behind the staged strings and translates the characters of anti-diagonal 1's windows.  The zero floor, the H = 0 of
 * every slot without a cell (DPX_BANDDIR_NO_CELL_H), the zero border callables, the tie orders, the codes and the tracker of the first
 * maximum in row-major order are k_bdl_fill's.  a.match / a.mismatch are not read.
 *
 * Its own unit: tests/test_bdl_kernels_isa.py holds dpx_bdl_kernels.hip to exactly its 16 fills, one walk and one export.
 */
#include "dpx_bdl_dev.hpp"

namespace {

using namespace dpx_band;

template <int C, bool PB, bool AFFINE>
__global__ void __launch_bounds__(DPX_FILL_THREADS) k_bdlt_fill(const dpx_bdx_args x) { /* (the frame's argument block: x.f and x.tab are read, x.scan is off) */
    constexpr bool EXT = true, TABLE = true;
    constexpr int SCAN = 0;
    const dpx_fill_args &a = x.f;
    using State = BdlState<C, AFFINE>;
    constexpr int Gd = 32 / C, kStepBits = 4 * C; /* steps per 16-byte store (a multiple of 4); a nibble per cell */
    [[maybe_unused]] constexpr bool kPickUniform = false;
    /* (every border cell is 0: the border line of an empty sequence never displaces the 0 of (0, 0)) */
#define DPX_BANDDIR_WEIGHTS                                                                                              \
    const int e = a.gapExtend, g = AFFINE ? a.gapOpen + a.gapExtend : a.gapOpen;                                         \
    [[maybe_unused]] const int Z = -1, pen = 0;                                                                          \
    const int bord1 = 0;                                                                                                 \
    auto bord = [](const int) -> int { return 0; };                                                                      \
    auto line_first_max = [](const int L) -> int { return min(L, 1); };
#define DPX_BANDDIR_NO_CELL_H 0
#define DPX_BANDDIR_STEP(P1_, INTERIOR_, A_) \
    bdl_step<C, AFFINE, true, P1_, INTERIOR_>(st, A_, i0, j0, lane, m, n, B, 0, 0, g, e, qL, rL, tabL, codeL)
#include "dpx_banddir_fill.inc"
#undef DPX_BANDDIR_STEP
#undef DPX_BANDDIR_NO_CELL_H
#undef DPX_BANDDIR_WEIGHTS
}

} // namespace

hipError_t dpx_launch_bdlt_fill(const dpx_subst_args &t, int C, bool affine, hipStream_t stream) {
    if (t.f.numPairs <= 0) return hipSuccess;
    if (!t.tab.table || !t.tab.codeOf) return hipErrorInvalidValue;
    const dpx_bdx_args x = {t.f, t.tab, {-1, -1, nullptr}};
    return dispatch_fill(C, t.f.band, affine, [&](auto c, auto pb, auto af) {
        return launch_banddir_fill(k_bdlt_fill<decltype(c)::value, decltype(pb)::value, decltype(af)::value>, x, x.f, stream);
    });
}
