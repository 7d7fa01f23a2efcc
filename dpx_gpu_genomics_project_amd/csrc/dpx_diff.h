/* dpx_diff.h -- interface between the C-ABI layer (dpx_output.cpp) and the difference-string kernels (dpx_diff_kernels.hip). */
#ifndef DPX_DIFF_H
#define DPX_DIFF_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dpx_align.h"
#include "dpx_layout.h"

/* uint64 entries of scratch the scan needs behind the numPairs + 1 offsets: the tile totals (ceil(numPairs / 2048)) */
size_t dpx_diff_scan_tiles(size_t numPairs);

/* Traceback lines of a batch (tbOff / tb / tbLen as k_traceback leaves them, see dpx_cigar.h) -> the MD (kind == DPX_DIFF_MD) or cs
 * (DPX_DIFF_CS) string of every pair, back to back in `text`, and the numPairs + 1 byte offsets of the strings in `offsets`
 * (offsets[numPairs] = the total).  `text` needs tbOff[numPairs] bytes: a pair's string never exceeds three times its line capacity
 * (include/dpx_align.h derives the bound).  Three stages on `stream`, no host round trip between them: k_diff_count (the pair's
 * byte length, into offsets[p]), k_diff_scan (exclusive prefix in place, and the total), k_diff_write (the bytes). */
hipError_t dpx_launch_diffs(unsigned kind, const dpx_pair_dev *pairs, const int32_t *tbLen, const uint64_t *tbOff, const char *tb,
                            int numPairs, unsigned long long *offsets, unsigned long long *tileSums, char *text, hipStream_t stream);

#endif
