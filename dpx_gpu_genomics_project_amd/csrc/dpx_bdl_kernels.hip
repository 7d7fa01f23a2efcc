/*
 * dpx_bdl_kernels.hip -- local band-direction batches (DPX_KEEP_LOCAL_BAND_DIRECTIONS) of BSW and BASW for gfx950: fill, walk and export.
 *
 * The cells are k_banded_fill's / k_basw_fill's, value for value, in int32 registers: the band |i-j| <= B-1 of the cells with i, j >= 1,
 * a zero floor, and every neighbour that is a border cell, lies outside the band or outside the matrix reads H = 0 (BASW: I = D =
 * DPX_NEG).  The schedule, the code window and the store per Gd = 32 / C steps are k_bdir_fill's (dpx_banddir_kernels.hip), the layout is
 * dpx_banddir.h's unchanged; everything outside bdl_step is the frame shared with the three other band-direction fills,
 * dpx_banddir_fill.inc, included below in its EXT form with no table and no scan.  A slot that holds no cell -- a border slot included:
 * there is no border value here -- hands on H = 0, so the frame starts from H = 0 in every slot (DPX_BANDDIR_NO_CELL_H) and its
 * empty-sequence branch sees a border line of zeros: score 0 at (0, 0).  Nothing but codes leaves the registers.
 *
 * The step, bdl_step, and its state are dpx_bdl_dev.hpp's (the codes are described there), shared with the table fills of
 * dpx_bdlt_kernels.hip; here it is instantiated with TABLE = false, the text this unit had of its own.
 *
 * End cell: the frame's tracker, the first maximum in row-major order; only H > 0 displaces (0, 0).  A slot without a cell offers H = 0,
 * which displaces nothing.
 *
 * Walk (banddir_walk's LOCAL form): from the end cell in SCORING until H == 0 -- BSW: bit 2, BASW: move 0, either: a cell without a
 * code -- with no tails.  It may step onto a cell outside the band and stops there, as the matrix batch's walk does.  Export
 * (banddir_export's LOCAL form): 0 on the borders and outside the band in every plane, the stored bits everywhere else.
 */
#include "dpx_bdl_dev.hpp"

namespace {

using namespace dpx_band;

template <int C, bool PB, bool AFFINE>
__global__ void __launch_bounds__(DPX_FILL_THREADS) k_bdl_fill(const dpx_fill_args f) {
    constexpr bool EXT = true, TABLE = false;
    constexpr int SCAN = 0;
    const dpx_bdx_args x = {f, {nullptr, nullptr}, {-1, -1, nullptr}}; /* (the frame's names; nothing of it but x.f is read) */
    const dpx_fill_args &a = x.f;
    using State = BdlState<C, AFFINE>;
    constexpr int Gd = 32 / C, kStepBits = 4 * C; /* steps per 16-byte store (a multiple of 4); a nibble per cell */
    [[maybe_unused]] constexpr bool kPickUniform = false;
    /* (every border cell is 0: the border line of an empty sequence never displaces the 0 of (0, 0)) */
#define DPX_BANDDIR_WEIGHTS                                                                                              \
    const int match = a.match, mismatch = a.mismatch, e = a.gapExtend, g = AFFINE ? a.gapOpen + a.gapExtend : a.gapOpen; \
    [[maybe_unused]] const int Z = -1, pen = 0;                                                                          \
    const int bord1 = 0;                                                                                                 \
    auto bord = [](const int) -> int { return 0; };                                                                      \
    auto line_first_max = [](const int L) -> int { return min(L, 1); };
#define DPX_BANDDIR_NO_CELL_H 0
#define DPX_BANDDIR_STEP(P1_, INTERIOR_, A_) \
    bdl_step<C, AFFINE, false, P1_, INTERIOR_>(st, A_, i0, j0, lane, m, n, B, match, mismatch, g, e, qL, rL, tabL, codeL)
#include "dpx_banddir_fill.inc"
#undef DPX_BANDDIR_STEP
#undef DPX_BANDDIR_NO_CELL_H
#undef DPX_BANDDIR_WEIGHTS
}

/* NibbleCodec with the move 0 of a local cell: NONE in the H plane, not a diagonal */
struct LocalNibbleCodec : NibbleCodec {
    static __device__ __forceinline__ int decode(const int c, const int which) {
        if (which == 0 && (c & 3) == 0) return 0;
        return NibbleCodec::decode(c, which);
    }
};

__global__ void __launch_bounds__(64) k_bdl_traceback(const dpx_fill_args a, int numPairs, int linear, const uint64_t *tbOff, char *tb, int32_t *tbLen) {
    __shared__ __attribute__((aligned(16))) unsigned char ring[kRingBytes];
    banddir_walk<LocalNibbleCodec, true>(ring, a, numPairs, tbOff, tb, tbLen, linear != 0);
}

/* `which` 0 directionMain, 1 / 2 directionIndel of I / D (BASW) */
__global__ void __launch_bounds__(256) k_bdl_export(const unsigned char *codes, const dpx_pair_dev pr, const char *seq, int band, int which,
                                                    uint8_t *out) {
    banddir_export<LocalNibbleCodec, true>(codes, pr, seq, band, which, out);
}

} // namespace

hipError_t dpx_launch_bdl_fill(const dpx_fill_args &a, int C, bool affine, hipStream_t stream) {
    if (a.numPairs <= 0) return hipSuccess;
    return dispatch_fill(C, a.band, affine, [&](auto c, auto pb, auto af) {
        return launch_banddir_fill(k_bdl_fill<decltype(c)::value, decltype(pb)::value, decltype(af)::value>, a, a, stream);
    });
}

hipError_t dpx_launch_bdl_traceback(const dpx_fill_args &a, int numPairs, bool affine, const uint64_t *tbOff, char *tb, int32_t *tbLen,
                                    hipStream_t stream) {
    if (numPairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_bdl_traceback, dim3((unsigned)numPairs), dim3(64), 0, stream, a, numPairs, affine ? 0 : 1, tbOff, tb, tbLen);
    return hipGetLastError();
}

hipError_t dpx_launch_bdl_export(const uint8_t *codes, const dpx_pair_dev &pr, const char *seq, int band, int which, uint8_t *out,
                                 hipStream_t stream) {
    const uint64_t total = (uint64_t)(pr.m + 1) * (uint64_t)(pr.n + 1);
    if (!total) return hipSuccess;
    uint64_t blocks = (total + 255) / 256;
    if (blocks > 65536u) blocks = 65536u;
    hipLaunchKernelGGL(k_bdl_export, dim3((unsigned)blocks), dim3(256), 0, stream, codes, pr, seq, band, which, out);
    return hipGetLastError();
}
