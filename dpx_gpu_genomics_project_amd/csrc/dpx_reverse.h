/* dpx_reverse.h -- interface between the C-ABI layer (dpx_settings.cpp, dpx_output.cpp) and the orientation kernels (dpx_reverse_kernels.hip):
 * dpx_batch_set_reversed's device work. */
#ifndef DPX_REVERSE_H
#define DPX_REVERSE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dpx_align.h"
#include "dpx_layout.h"

/* one string to copy back to front: `len` bytes at byte offset `src` of the sequence buffer -> byte offset `dst` (a multiple of 16) of
 * the same buffer */
typedef struct dpx_rev_job {
    int32_t src, dst, len, reserved;
} dpx_rev_job;

/* bytes one reversed copy of `len` bytes occupies behind its (16-byte aligned) start: whole 16-byte blocks, which is what the kernel
 * stores and what stage_bytes loads, plus one block that the dword reads of the walks (load4, CharWin) may touch behind the last byte */
static inline size_t dpx_rev_slot_bytes(size_t len) { return ((len + 15) & ~(size_t)15) + 16; }

/* `seq` is 256-byte aligned and padded to a multiple of 256 behind its last byte: the aligned 16-byte blocks that hold a byte of a
 * source string never leave it.  Every job's destination slot (dpx_rev_slot_bytes) lies inside it and overlaps no source and no other slot. */
hipError_t dpx_launch_reverse_strings(char *seq, const dpx_rev_job *jobs, int numJobs, hipStream_t stream);

/* The three traceback lines (dpx_cigar.h: the contract of every walk) of the pairs listed in `flagged`, each reversed in place: the
 * tbLen[p] characters stay right-aligned in their capacity, and no byte outside them changes. */
hipError_t dpx_launch_flip_lines(const dpx_pair_dev *pairs, const int32_t *flagged, int numFlagged, const int32_t *tbLen, const uint64_t *tbOff,
                                 char *tb, hipStream_t stream);

/* dpx_alignment records of the listed pairs, from the reversed frame to the original strings: refStart = n - refEnd and refEnd =
 * n - refStart, the query likewise with m; nothing else changes */
hipError_t dpx_launch_map_records(const dpx_pair_dev *pairs, const int32_t *flagged, int numFlagged, dpx_alignment *records, hipStream_t stream);

#endif
