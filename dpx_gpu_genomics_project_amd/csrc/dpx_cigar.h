/* dpx_cigar.h -- interface between the C-ABI layer (dpx_output.cpp) and the CIGAR kernels (dpx_cigar_kernels.hip). */
#ifndef DPX_CIGAR_H
#define DPX_CIGAR_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dpx_align.h"
#include "dpx_layout.h"

/* uint64 entries of scratch the scan needs behind the records: the tile totals (ceil(numPairs / 2048)) */
size_t dpx_cigar_scan_tiles(size_t numPairs);

/* Traceback lines of a batch (tbOff / tb / tbLen as k_traceback leaves them: three lines per pair, right-aligned in a capacity of
 * (m + n + 1 + 3) & ~3, in a 256-byte aligned buffer) -> one dpx_alignment per pair in `records`, the packed ops in `ops` (room for
 * one op per column: tbOff[numPairs] / 3) and their number in `*total`.  Three stages on `stream`, no host round trip between them:
 * k_cigar_count (every field of the records but opsOffset), k_cigar_scan (opsOffset = exclusive prefix of numOps, *total),
 * k_cigar_write (the ops).  `flags` are DPX_CIGAR_EXTENDED / DPX_CIGAR_M. */
hipError_t dpx_launch_cigars(const dpx_pair_dev *pairs, const int32_t *endRow, const int32_t *endCol, const int32_t *tbLen,
                             const uint64_t *tbOff, const char *tb, int numPairs, unsigned flags, dpx_alignment *records,
                             unsigned long long *tileSums, unsigned long long *total, uint32_t *ops, hipStream_t stream);

#endif
