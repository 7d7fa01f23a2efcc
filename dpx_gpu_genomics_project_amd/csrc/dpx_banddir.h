/*
 * dpx_banddir.h -- banded direction batches (DPX_KEEP_BAND_DIRECTIONS on BANW / BAXT, DPX_KEEP_LOCAL_BAND_DIRECTIONS on BSW / BASW): the
 * 4-bit code layout and the launchers of dpx_banddir_kernels.hip and dpx_bdl_kernels.hip.  Shared by host and device code.
 *
 * Code of one cell (one nibble) -- dpx_dir.h's ANW code:
 *   bits 0-1  the move: 1 diagonal, 2 up (QUERY_DELETION), 3 left (QUERY_INSERTION); MATCH versus MISMATCH is rebuilt from the two bases
 *   bit 2     the I (horizontal gap) cell extends rather than opens
 *   bit 3     the D (vertical gap) cell extends rather than opens
 * BASW stores dpx_dir.h's ASW code (the same, with move 0 where H == 0), BSW its LSW code (move 0-3, bit 2: H == 0).
 *
 * Layout.  The fill runs k_banw_fill's schedule (dpx_layout.h, "Banded SW"): step A = i + j - 2, slot s = (i - j + B-1) >> 1, lane
 * l = s / C, c = s % C with C = dpx_band_cpl(B) slots per lane.  A lane collects its C codes of Gd = 32 / C consecutive steps in four
 * registers (32 nibbles) and stores them with ONE 16-byte store, so every store of the wave writes one contiguous KiB.  Chunk A / Gd:
 *
 *       byte(i, j) = base + (A / Gd) * chunkStrideBytes + l * 16 + nib / 2,   nib = (A % Gd) * C + c   (low nibble first)
 *
 * base and the chunk stride come from dpx_pair_dev.matOff / chunkStride, counted in int16 units as for every other layout (a chunk is
 * 512 of them), so base = 2 * matOff bytes.  A pair takes ceil((m + n - 1) / Gd) chunks.  Only in-band cells with i, j >= 1 have a
 * nibble; the in-band border cells are closed-form.  dpx_banddir_byte is the one index function: the fill places a lane's 16 bytes
 * with dpx_banddir_piece (the part of it that does not depend on the nibble), export and walk call it per cell.
 */
#ifndef DPX_BANDDIR_H
#define DPX_BANDDIR_H

#include <stdint.h>

#include "dpx_layout.h"

#define DPX_BANDDIR_CHUNK_BYTES 1024u /* one wave store: 64 lanes x 16 B */

DPX_HD int dpx_banddir_group(int C) { return 32 / C; } /* steps per 16-byte lane store */
DPX_HD uint64_t dpx_banddir_chunks(int m, int n, int band) { /* 1-KiB chunks of one pair */
    if (m <= 0 || n <= 0) return 0;
    const uint64_t Gd = (uint64_t)dpx_banddir_group(dpx_band_cpl(band));
    return ((uint64_t)m + (uint64_t)n - 1u + Gd - 1u) / Gd;
}
/* byte offset, relative to the pair's base, of the 16 bytes lane l writes for chunk `chunk` */
DPX_HD uint64_t dpx_banddir_piece(uint64_t chunk, int l, uint64_t chunkStrideBytes) { return chunk * chunkStrideBytes + (uint64_t)(l * 16); }
/* byte offset of in-band cell (i, j), i, j >= 1, relative to the pair's base, and the nibble's shift inside that byte */
DPX_HD uint64_t dpx_banddir_byte(int i, int j, int band, uint64_t chunkStrideBytes, int *shift) {
    const int C = dpx_band_cpl(band), sc = dpx_log2(C), sg = 5 - sc; /* Gd = 2^sg */
    const int A = i + j - 2;
    const int s = (i - j + (band - 1)) >> 1;
    const int l = s >> sc, c = s & (C - 1);
    const int nib = ((A & ((1 << sg) - 1)) << sc) + c;
    *shift = (nib & 1) * 4;
    return dpx_banddir_piece((uint64_t)(A >> sg), l, chunkStrideBytes) + (uint64_t)(nib >> 1);
}

#if defined(__HIPCC__) /* the launchers (the layout above is plain C) */
#include "dpx_kernels.h"

/* the fill: a.mat is the code pool (byte addressed from 2 * matOff), a.ldsPerWave / ldsRefOff are k_banw_fill's staging;
 * `ext` false: BANW's end cell (m, n), true: BAXT's first maximum in row-major order.  C = dpx_band_cpl(a.band) */
hipError_t dpx_launch_bdir_fill(const dpx_fill_args &a, int C, bool ext, hipStream_t stream);
/* one wave per pair walks the codes from endRow / endCol and writes the three right-aligned lines at tbOff[p] (capacity (m+n+1+3)&~3)
 * and tbLen[p], the contract of dpx_launch_traceback that dpx_launch_output and the CIGAR kernels consume */
hipError_t dpx_launch_bdir_traceback(const dpx_fill_args &a, int numPairs, const uint64_t *tbOff, char *tb, int32_t *tbLen, hipStream_t stream);
/* one pair's direction matrix `which` (0 H, 1 I, 2 D) as the row-major (m+1) x (n+1) uint8 enums of c++/backtrack.h */
hipError_t dpx_launch_bdir_export(const uint8_t *codes, const dpx_pair_dev &pr, const char *seq, int band, int which, uint8_t *out,
                                  hipStream_t stream);

/* dpx_bdl_kernels.hip -- the same three for DPX_KEEP_LOCAL_BAND_DIRECTIONS batches of BSW (`affine` false: LSW's code, bit 2 = "H is 0") and
 * BASW (true: ASW's code, move 0 = "H is 0") in the same layout: zero floor, neighbours without a cell read H = 0, the end cell is the first
 * maximum in row-major order, the walk stops where H == 0 and has no tails, the export is 0 on the borders */
hipError_t dpx_launch_bdl_fill(const dpx_fill_args &a, int C, bool affine, hipStream_t stream);
hipError_t dpx_launch_bdl_traceback(const dpx_fill_args &a, int numPairs, bool affine, const uint64_t *tbOff, char *tb, int32_t *tbLen,
                                    hipStream_t stream);
hipError_t dpx_launch_bdl_export(const uint8_t *codes, const dpx_pair_dev &pr, const char *seq, int band, int which, uint8_t *out,
                                 hipStream_t stream);
/* dpx_bdlt_kernels.hip -- dpx_launch_bdl_fill's cells, codes, stores and results with the diagonal term of t.tab (k_bdlt_fill;
 * dpx_batch_set_local_direction_table).  t.f.ldsPerWave includes DPX_SUBST_IMAGE_BYTES behind the staged strings, and the launch asks for
 * t.f.ldsPerWave * t.f.wavesPerBlock bytes of LDS; t.f.match / mismatch are not read.  Walk and export are the two above. */
hipError_t dpx_launch_bdlt_fill(const dpx_subst_args &t, int C, bool affine, hipStream_t stream);
#endif

#endif
