/*
 * dpx_banddir2.h -- two-piece banded direction batches (DPX_KEEP_BAND_DIRECTIONS | DPX_TWO_PIECE_GAPS on BANW / BAXT): the 8-bit code
 * layout and the launchers of dpx_bd2_kernels.hip.  Shared by host and device code.
 *
 * Code of one cell (one byte):
 *   bits 0-2  the move: 1 diagonal, 2 up piece 1 (D1), 3 left piece 1 (I1), 4 up piece 2 (D2), 5 left piece 2 (I2); MATCH versus MISMATCH
 *             is rebuilt from the two bases
 *   bit 3     the I1 cell extends rather than opens        bit 4     the D1 cell extends
 *   bit 5     the I2 cell extends                          bit 6     the D2 cell extends                bit 7     0
 *
 * Layout.  dpx_banddir.h's schedule, slots and 1-KiB chunks with bytes in place of nibbles: step A = i + j - 2, slot s = (i - j + B-1) >> 1,
 * lane l = s / C, c = s % C with C = dpx_band_cpl(B) <= 4 slots per lane (B <= 256).  A lane collects its C codes of Gd = 16 / C steps in
 * four registers and stores them with ONE 16-byte store.  Chunk A / Gd:
 *
 *       byte(i, j) = base + (A / Gd) * chunkStrideBytes + l * 16 + (A % Gd) * C + c
 *
 * base = 2 * matOff bytes and the chunk stride are dpx_pair_dev's, as in dpx_banddir.h.  A pair takes ceil((m + n - 1) / Gd) chunks.  Only
 * in-band cells with i, j >= 1 have a byte.  dpx_banddir2_byte is the one index function: the fill places a lane's 16 bytes with
 * dpx_banddir_piece, export and walk call dpx_banddir2_byte per cell.
 */
#ifndef DPX_BANDDIR2_H
#define DPX_BANDDIR2_H

#include <stdint.h>

#include "dpx_banddir.h"

#define DPX_BANDDIR2_MAX_BAND 256 /* C = 8 does not fit the register file */

DPX_HD int dpx_banddir2_group(int C) { return 16 / C; } /* steps per 16-byte lane store */
DPX_HD uint64_t dpx_banddir2_chunks(int m, int n, int band) { /* 1-KiB chunks of one pair */
    if (m <= 0 || n <= 0) return 0;
    const uint64_t Gd = (uint64_t)dpx_banddir2_group(dpx_band_cpl(band));
    return ((uint64_t)m + (uint64_t)n - 1u + Gd - 1u) / Gd;
}
/* byte offset of in-band cell (i, j), i, j >= 1, relative to the pair's base */
DPX_HD uint64_t dpx_banddir2_byte(int i, int j, int band, uint64_t chunkStrideBytes) {
    const int C = dpx_band_cpl(band), sc = dpx_log2(C), sg = 4 - sc; /* Gd = 2^sg */
    const int A = i + j - 2;
    const int s = (i - j + (band - 1)) >> 1;
    const int l = s >> sc, c = s & (C - 1);
    return dpx_banddir_piece((uint64_t)(A >> sg), l, chunkStrideBytes) + (uint64_t)(((A & ((1 << sg) - 1)) << sc) + c);
}

#if defined(__HIPCC__) /* the launchers (the layout above is plain C) */
#include "dpx_kernels.h"

/* k_bd2_fill: dpx_bdx_args' fields and meaning (`tab`, both pointers NULL: byte compare; `scan`, zdrop / endBonus both -1: no scan, `ext`
 * batches only) plus the second gap piece; piece 1 is f.gapOpen / f.gapExtend.  Every mode is legal, "nothing on" included. */
typedef struct dpx_bd2_args {
    dpx_fill_args f;
    dpx_table_ref tab;
    dpx_ext_ref scan;
    int32_t gapOpen2, gapExtend2;
} dpx_bd2_args;
hipError_t dpx_launch_bd2_fill(const dpx_bd2_args &a, int C, bool ext, hipStream_t stream);
/* dpx_launch_bdir_traceback's contract over the byte codes (five states) */
hipError_t dpx_launch_bd2_traceback(const dpx_fill_args &a, int numPairs, const uint64_t *tbOff, char *tb, int32_t *tbLen, hipStream_t stream);
/* one pair's plane `which`: 0 H, 1 I (piece 1), 2 D (piece 1), 3 I2, 4 D2 as c++/backtrack.h's enums, 5 the piece of H's gap move */
hipError_t dpx_launch_bd2_export(const uint8_t *codes, const dpx_pair_dev &pr, const char *seq, int band, int which, uint8_t *out,
                                 hipStream_t stream);

/* dpx_lb2_kernels.hip: the local twin (DPX_KEEP_LOCAL_BAND_DIRECTIONS | DPX_LOCAL_TWO_PIECE_GAPS on BASW), the same byte code and layout;
 * move 0 is a cell with H == 0.  k_lb2_fill: `tab` as above, no scan; piece 1 is f.gapOpen / f.gapExtend. */
typedef struct dpx_lb2_args {
    dpx_fill_args f;
    dpx_table_ref tab;
    int32_t gapOpen2, gapExtend2;
} dpx_lb2_args;
hipError_t dpx_launch_lb2_fill(const dpx_lb2_args &a, int C, hipStream_t stream);
/* dpx_launch_bdl_traceback's contract over the byte codes (five states, the walk ends on H == 0, no tails) */
hipError_t dpx_launch_lb2_traceback(const dpx_fill_args &a, int numPairs, const uint64_t *tbOff, char *tb, int32_t *tbLen, hipStream_t stream);
/* dpx_launch_bd2_export's six selectors under the local export's rule: every plane 0 on the borders and outside the band */
hipError_t dpx_launch_lb2_export(const uint8_t *codes, const dpx_pair_dev &pr, const char *seq, int band, int which, uint8_t *out,
                                 hipStream_t stream);
#endif

#endif
