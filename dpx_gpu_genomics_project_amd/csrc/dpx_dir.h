/*
 * dpx_dir.h -- direction-matrix batches (DPX_KEEP_DIRECTIONS): the 4-bit code layout and the launchers of
 * dpx_dir_kernels.hip.  Shared by host and device code; dpx_kernels.h / dpx_layout.h are included read-only.
 *
 * Code of one cell (one nibble):
 *   bits 0-1  the move the reference's direction matrix records: 0 none, 1 diagonal, 2 up (QUERY_DELETION / UPPER_GAP),
 *             3 left (QUERY_INSERTION / LEFT_GAP); MATCH versus MISMATCH is rebuilt from the two bases
 *   bit 2     LSW: H of this cell is 0 (the walk stops there, c++/LinearSmithWaterman.cpp:222);
 *             ANW: the I (horizontal gap) cell extends rather than opens
 *   bit 3     ANW: the D (vertical gap) cell extends rather than opens
 *
 * Layout.  The fill runs the striped one-wave-per-pair schedule of k_linear_fill: lane l owns rows [l*R, l*R+R) of a 64*R-row
 * stripe and is on column j = t - l + 1 in step t of the stripe.  Every stripe owns Wp = n + 63 steps rounded up to a multiple
 * of G = 32 / R, so the pair's step is T = k*Wp + t.  A lane collects its R codes of G consecutive steps in four registers
 * (32 nibbles) and stores them with ONE 16-byte store: every store instruction of the wave writes one whole, contiguous KiB
 * (sixteen 64-byte sectors), whatever R is.  Chunk c = T / G of a pair:
 *
 *       byte(i, j) = base + c * chunkStrideBytes + l * 16 + nib / 2,   nib = (T % G) * R + r   (low nibble first)
 *       with i0 = i-1, k = i0 / (64R), l = (i0 / R) % 64, r = i0 % R, T = k*Wp + (j-1) + l
 *
 * base and the chunk stride come from dpx_pair_dev.matOff / chunkStride, counted in int16 units as for the score layouts
 * (the host's placement code is shared: a chunk is 512 of them), so base = 2 * matOff bytes.  Border row 0 / column 0 are
 * closed-form and not stored.
 */
#ifndef DPX_DIR_H
#define DPX_DIR_H

#include <stdint.h>

#include "dpx_kernels.h"
#include "dpx_layout.h"

#define DPX_DIR_CHUNK_BYTES 1024u /* one wave store: 64 lanes x 16 B */

DPX_HD int dpx_dir_group(int R) { return 32 / R; } /* steps per 16-byte lane store */
DPX_HD uint32_t dpx_dir_stripe_steps(int n, int R) {
    const uint32_t G = (uint32_t)dpx_dir_group(R);
    return ((uint32_t)n + 63u + G - 1u) / G * G;
}
DPX_HD uint64_t dpx_dir_chunks(int m, int n, int R) { /* 1-KiB chunks of one pair */
    if (m <= 0 || n <= 0) return 0;
    return (uint64_t)dpx_tiled_stripes(m, R) * (uint64_t)(dpx_dir_stripe_steps(n, R) / (uint32_t)dpx_dir_group(R));
}
/* byte offset of cell (i, j) relative to the pair's base, and the nibble's shift inside that byte (R and G are powers of two: shifts) */
DPX_HD uint64_t dpx_dir_byte(int i, int j, int n, int R, uint64_t chunkStrideBytes, int *shift) {
    const int sr = dpx_log2(R), sg = 5 - sr, i0 = i - 1;
    const int k = i0 >> (sr + 6), l = (i0 >> sr) & 63, r = i0 & (R - 1);
    const uint64_t T = (uint64_t)k * dpx_dir_stripe_steps(n, R) + (uint64_t)(j - 1) + (uint64_t)l;
    const int nib = ((int)(T & (uint64_t)((1 << sg) - 1)) << sr) + r;
    *shift = (nib & 1) * 4;
    return (T >> sg) * chunkStrideBytes + (uint64_t)(l * 16 + (nib >> 1));
}

typedef struct dpx_dir_args {
    const char *seq;
    const dpx_pair_dev *pairs;
    const int32_t *order;    /* launch order (longest pairs first) or NULL */
    int32_t numPairs;
    int32_t match, mismatch, gapOpen, gapExtend;
    uint8_t *codes;          /* the batch's code pool */
    int32_t *score, *endRow, *endCol;
    uint32_t ldsPerWave;     /* bytes of one wave's edge rows + staged reference (in LDS, or in `scratch`) */
    uint32_t wavesPerBlock;
    uint32_t ldsEdge2Off;    /* ANW: offset of the D edge row */
    uint32_t ldsRefOff;      /* offset of the staged reference */
    unsigned char *scratch;  /* long references: the same per-wave area in global memory, else NULL */
    int32_t firstSlot;       /* launch slot of the kernel's first wave (long references run DPX_DIR_SCRATCH_SLOTS waves per launch) */
} dpx_dir_args;

/* waves per launch of a batch whose edge rows live in global memory: the scratch holds this many per-wave areas (more than the chip keeps
 * resident: 256 CUs x 8), launches on one stream reuse it one after the other */
#define DPX_DIR_SCRATCH_SLOTS 2048

hipError_t dpx_launch_fill_dir(const dpx_dir_args &a, int algo, int R, hipStream_t stream);

/* ANW / ASW / ASG direction batches under a substitution table (dpx_batch_set_direction_table; dpx_dirtab_kernels.hip): the same fill,
 * codes and stores with the diagonal term table[codeOf[reference byte] * 32 + codeOf[query byte]] (`tab`: dpx_kernels.h's
 * dpx_table_ref, the device image with the map behind the table); d.match / d.mismatch are not read.  Every wave keeps the
 * image in LDS: with the edge rows in LDS d.ldsPerWave includes DPX_SUBST_IMAGE_BYTES behind the staged reference and the launch asks
 * for d.ldsPerWave * d.wavesPerBlock; with the edge rows in d.scratch d.ldsPerWave is the scratch area's as before and the launch asks
 * for DPX_SUBST_IMAGE_BYTES * d.wavesPerBlock. */
typedef struct dpx_dirtab_args {
    dpx_dir_args d;
    dpx_table_ref tab;
} dpx_dirtab_args;
hipError_t dpx_launch_dirtab_fill(const dpx_dirtab_args &a, int algo, int R, hipStream_t stream);
/* one wave per pair walks the codes in runs and writes the three right-aligned lines at tbOff[p] (capacity (m+n+1+3)&~3) and tbLen[p],
 * the contract of dpx_launch_traceback that dpx_launch_output formats */
hipError_t dpx_launch_traceback_dir(const dpx_dir_args &a, int numPairs, int algo, int R, const uint64_t *tbOff, char *tb, int32_t *tbLen,
                                    hipStream_t stream);
/* one pair's direction matrix `which` (0 H, 1 I, 2 D) as the reference's row-major (m+1) x (n+1) uint8 enums (c++/backtrack.h) */
hipError_t dpx_launch_export_dir(const uint8_t *codes, const dpx_pair_dev &pr, const char *seq, int algo, int R, int which, uint8_t *out,
                                 hipStream_t stream);

#endif
