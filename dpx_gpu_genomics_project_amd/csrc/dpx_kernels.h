/* dpx_kernels.h -- interface between the C-ABI layer (dpx_capi.cpp) and the HIP kernel units: dpx_kernels.hip (linear-gap fills),
 * dpx_affine_kernels.hip, dpx_bsw_kernels.hip, dpx_traceback_kernels.hip, dpx_output_kernels.hip and the banded affine units. */
#ifndef DPX_KERNELS_H
#define DPX_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpx_layout.h"

/* same numbering as dpx_algo in include/dpx_align.h */
#define DPX_K_LNW 0
#define DPX_K_LSW 1
#define DPX_K_ANW 2
#define DPX_K_BSW 3
#define DPX_K_ASW 4 /* affine-gap Smith-Waterman: the ANW kernels' Gotoh recurrence with LSW's zero floor and start cell */
#define DPX_K_BASW 5 /* banded affine-gap Smith-Waterman: ASW's recurrence on BSW's band and anti-diagonal schedule (dpx_basw_kernels.hip) */
#define DPX_K_ASG 6 /* affine-gap semi-global alignment: the ANW kernels under a zero row-0 border, ending on the first maximum of row m */
#define DPX_K_BANW 7 /* banded affine-gap Needleman-Wunsch: ANW's recurrence and borders inside BSW's band, minus infinity outside (dpx_banw_kernels.hip) */
#define DPX_K_BAXT 10 /* banded affine-gap extension: BANW's cells, ending on the first maximum of H over the band (dpx_baxt_kernels.hip; 8 and 9 are unassigned) */


typedef struct dpx_fill_args {
    const char *seq;            /* flat sequence bytes (device copy of parseInput's buffer) */
    const dpx_pair_dev *pairs;  /* per-pair geometry + matrix offset */
    const int32_t *order;       /* optional launch order (longest pairs first) or NULL */
    const dpx_wave_desc *waves; /* lane-packed kernels: one descriptor per wave (numPairs = number of waves) */
    int32_t numPairs;
    int32_t match, mismatch, gapOpen, gapExtend, band;
    int16_t *mat;               /* matrix pool (int16, engine layout) or NULL when score-only */
    int32_t *score, *endRow, *endCol;
    uint32_t ldsPerWave;        /* bytes of dynamic LDS per wave */
    uint32_t wavesPerBlock;     /* independent waves per workgroup of the one-wave-per-pair / -couple kernels: 4, or 1 for small launches */
    uint32_t ldsEdge2Off;       /* ANW: offset of the second edge row (D) */
    uint32_t ldsRefOff;         /* offset of the staged reference characters */
    uint32_t ldsQryOff;         /* offset of the staged query characters (rolling multi-stripe path) */
    uint32_t ldsBufStride;      /* split kernel: int16 elements between two edge rows */
    int32_t rowTags;            /* packed SW kernel: 1 = one (score, row-in-lane, column) key per pair and lane (needs max score * R + R-1 <= 65535),
                                   0 = one (score, column) key per pair and row */
    int32_t rampLines;          /* 1: skew-ramp steps store only the 128-byte lines that hold cells (byte-bound batches); 0: whole chunks */
} dpx_fill_args;

hipError_t dpx_launch_fill(const dpx_fill_args &a, int algo, int R, bool store, size_t ldsBytes, hipStream_t stream);
hipError_t dpx_launch_fill_lanes(const dpx_fill_args &a, int algo, int R, bool store, size_t ldsBytes, hipStream_t stream);
/* between units, not for dpx_capi.cpp: what the two dispatchers above (dpx_kernels.hip) hand the other families' batches to.
 * dpx_affine_kernels.hip takes ANW / ASW / ASG, dpx_bsw_kernels.hip BSW (C = cells per lane); a.numPairs > 0 */
hipError_t dpx_launch_affine_fill(const dpx_fill_args &a, int algo, int R, bool store, size_t ldsBytes, hipStream_t stream);
hipError_t dpx_launch_affine_lanes(const dpx_fill_args &a, int algo, int R, bool store, size_t ldsBytes, hipStream_t stream);
hipError_t dpx_launch_bsw_fill(const dpx_fill_args &a, int C, bool store, size_t ldsBytes, hipStream_t stream);
hipError_t dpx_launch_fill_lanes_packed(const dpx_fill_args &a, int algo, size_t ldsBytes, hipStream_t stream);
hipError_t dpx_launch_fill_split(const dpx_fill_args &a, int algo, int R, int waves, size_t ldsBytes, hipStream_t stream);
hipError_t dpx_launch_banded_packed(const dpx_fill_args &a, int C, size_t ldsBytes, hipStream_t stream);
hipError_t dpx_launch_fill_packed(const dpx_fill_args &a, int algo, int R, size_t ldsBytes, hipStream_t stream);
hipError_t dpx_launch_export(const int16_t *mat, const dpx_pair_dev &pr, int algo, int R, int planes, int plane, int gapOpen,
                             int gapExtend, int band, int16_t *out, hipStream_t stream);
/* walk: 0 = one lane per pair, three parallel 2-byte loads per step; 1 = one lane per pair through register-resident 8-row
 * column vectors (LSW / LNW, pays off when the batch is bound by sector requests rather than by load latency); 2 = one WAVE
 * per pair with an LDS window of 32 rows x 64 columns (LSW / LNW on layouts with 8-row vectors; other pairs fall back to 0) */
hipError_t dpx_launch_traceback(const dpx_fill_args &a, int numPairs, int algo, int R, int planes, int walk,
                                const uint64_t *tbOff, char *tb, int32_t *tbLen, hipStream_t stream);
size_t dpx_out_scan_tiles(size_t numPairs);
hipError_t dpx_launch_output(const dpx_pair_dev *pairs, const int32_t *score, const int32_t *tbLen, const uint64_t *tbOff, const char *tb,
                             int numPairs, unsigned long long firstNumber, unsigned long long *tileSums, unsigned long long *outOff, char *out,
                             bool scanOnly, bool compactOnly, hipStream_t stream);
/* banded affine SW (dpx_basw_kernels.hip): the fill (C = dpx_band_cpl(band) cells per lane), one plane of one pair as a row-major matrix,
 * and the traceback (walk 2: one wave per pair with an LDS window of the three planes; otherwise one lane per pair) */
hipError_t dpx_launch_basw_fill(const dpx_fill_args &a, int C, bool store, size_t ldsBytes, hipStream_t stream);
hipError_t dpx_launch_basw_export(const int16_t *mat, const dpx_pair_dev &pr, int plane, int band, int16_t *out, hipStream_t stream);
hipError_t dpx_launch_basw_traceback(const dpx_fill_args &a, int numPairs, int walk, const uint64_t *tbOff, char *tb, int32_t *tbLen,
                                     hipStream_t stream);
/* banded affine NW (dpx_banw_kernels.hip): the same three entry points; the export also needs the gap weights (in-band border cells are
 * not stored) */
hipError_t dpx_launch_banw_fill(const dpx_fill_args &a, int C, bool store, size_t ldsBytes, hipStream_t stream);
hipError_t dpx_launch_banw_export(const int16_t *mat, const dpx_pair_dev &pr, int plane, int band, int gapOpen, int gapExtend, int16_t *out,
                                  hipStream_t stream);
hipError_t dpx_launch_banw_traceback(const dpx_fill_args &a, int numPairs, int walk, const uint64_t *tbOff, char *tb, int32_t *tbLen,
                                     hipStream_t stream);
/* banded affine extension (dpx_baxt_kernels.hip): the fill only -- the stored layout, the edge rule and the border rule are BANW's, so
 * dpx_launch_banw_export and dpx_launch_banw_traceback serve it (both walks start from endRow / endCol) */
hipError_t dpx_launch_baxt_fill(const dpx_fill_args &a, int C, bool store, size_t ldsBytes, hipStream_t stream);
/* BAXT's extension mode, as every kernel that runs it takes it (dpx_zext_args, dpx_zsub_args, dpx_bdx_args, dpx_bd2_args): z-drop
 * termination (zdrop >= 0), the best score of row m and the end-bonus choice (endBonus >= 0; -1 = off for either).  `ext` is the device
 * array of per-pair records, eight int32 each in dpx_extension's field order. */
typedef struct dpx_ext_ref {
    int32_t zdrop, endBonus;
    int32_t *ext;
} dpx_ext_ref;
/* BAXT in extension mode (dpx_zext_kernels.hip, k_zext_fill): k_baxt_fill's cells and stores with the scan of dpx_ext_ref (zdrop /
 * endBonus: not both off).  Export and walks are BANW's, as for dpx_launch_baxt_fill. */
typedef struct dpx_zext_args {
    dpx_fill_args f;
    dpx_ext_ref scan;
} dpx_zext_args;
hipError_t dpx_launch_zext_fill(const dpx_zext_args &a, int C, bool store, size_t ldsBytes, hipStream_t stream);
/* A batch's substitution table on the device, as every table kernel takes it: `table` is 1 KiB of int8 with a row stride of 32 (row =
 * reference code, column = query code, unused entries 0), `codeOf` the 256-byte map from sequence byte to code, both 16-byte aligned in
 * device memory: one allocation of DPX_SUBST_IMAGE_BYTES, the map behind the table.  A cell's diagonal term is
 * H + table[(codeOf[ref byte] << 5) + codeOf[qry byte]]. */
#define DPX_SUBST_TABLE_BYTES 1024
#define DPX_SUBST_IMAGE_BYTES 1280
typedef struct dpx_table_ref {
    const int8_t *table;
    const uint8_t *codeOf;
} dpx_table_ref;
/* A fill's arguments under a table, two families' worth.
 * BANW / BAXT (dpx_subst_kernels.hip, dpx_batch_set_substitution): k_banw_fill's / k_baxt_fill's cells, stores and results (`ext`: BAXT's
 * end cell) with the diagonal term of dpx_table_ref.  f.ldsPerWave and `ldsBytes` include DPX_SUBST_IMAGE_BYTES per wave behind the
 * staged strings.  The walks are BANW's with the same diagonal term; the export is dpx_launch_banw_export.
 * ANW / ASW / ASG score-only batches (dpx_scoretab_kernels.hip, dpx_batch_set_score_table): k_affine_fill's / k_asw_fill's / k_asg_fill's
 * cells and results without stores (k_scoretab_fill) and the lane-packed kernels' (k_scoretab_lanes, R = 8) with the same diagonal term;
 * f.match / f.mismatch are not read.  f.ldsPerWave includes DPX_SUBST_IMAGE_BYTES behind the wave's slice (the one-wave kernel) or behind
 * its reference area (the lane-packed one), and each launch asks for f.ldsPerWave * f.wavesPerBlock bytes of LDS. */
typedef struct dpx_subst_args {
    dpx_fill_args f;
    dpx_table_ref tab;
} dpx_subst_args;
hipError_t dpx_launch_subst_fill(const dpx_subst_args &a, int C, bool store, bool ext, size_t ldsBytes, hipStream_t stream);
hipError_t dpx_launch_subst_traceback(const dpx_subst_args &a, int numPairs, int walk, const uint64_t *tbOff, char *tb, int32_t *tbLen,
                                      hipStream_t stream);
hipError_t dpx_launch_scoretab_fill(const dpx_subst_args &a, int algo, int R, hipStream_t stream);
hipError_t dpx_launch_scoretab_lanes(const dpx_subst_args &a, int algo, int R, hipStream_t stream);
/* BAXT in extension mode under a substitution table (dpx_zsub_kernels.hip, k_zsub_fill; dpx_batch_set_extension_table): k_subst_fill's
 * cells with k_zext_fill's scan and results.  `s` is what dpx_launch_subst_fill takes (LDS sizes include the table image), `scan` is
 * dpx_zext_args'.  The walks are dpx_launch_subst_traceback's, the export is dpx_launch_banw_export. */
typedef struct dpx_zsub_args {
    dpx_subst_args s;
    dpx_ext_ref scan;
} dpx_zsub_args;
hipError_t dpx_launch_zsub_fill(const dpx_zsub_args &a, int C, bool store, size_t ldsBytes, hipStream_t stream);
/* A band-direction batch (dpx_banddir.h) under dpx_batch_set_direction_scoring (dpx_bdx_kernels.hip, k_bdx_fill): k_bdir_fill's cells,
 * codes and stores with the diagonal term from a table (`tab`, both pointers NULL: byte compare) and, `ext` only, BAXT's extension mode
 * (`scan`; zdrop and endBonus both -1: off).  At least one of the two is on; BANW takes a table only.  With a table f.ldsPerWave includes
 * DPX_SUBST_IMAGE_BYTES behind the staged strings; the launch asks for f.ldsPerWave * f.wavesPerBlock bytes of LDS, as
 * dpx_launch_bdir_fill does.  Walk and export are dpx_launch_bdir_traceback / _export. */
typedef struct dpx_bdx_args {
    dpx_fill_args f;
    dpx_table_ref tab;
    dpx_ext_ref scan;
} dpx_bdx_args;
hipError_t dpx_launch_bdx_fill(const dpx_bdx_args &a, int C, bool ext, hipStream_t stream);
/* DPX_LONG_SCORES: the band-direction fills with nothing stored but the results; f.mat is not read.  LDS and waves per workgroup as for the
 * storing twin (with a table f.ldsPerWave includes DPX_SUBST_IMAGE_BYTES).
 * dpx_bscore_kernels.hip (k_bscore_fill; BANW / BAXT): k_bdir_fill's / k_bdx_fill's cells and results in every mode, "no table, no scan"
 * included (`tab` NULL: byte compare; `scan` both -1: off; BANW takes no scan).
 * dpx_lscore_kernels.hip (k_lscore_fill; BSW / BASW, `affine`): k_bdl_fill's / k_bdlt_fill's cells and results; `scan` is not read. */
hipError_t dpx_launch_bscore_fill(const dpx_bdx_args &a, int C, bool ext, hipStream_t stream);
hipError_t dpx_launch_lscore_fill(const dpx_bdx_args &a, int C, bool affine, hipStream_t stream);
hipError_t dpx_launch_unpack2(const uint32_t *packed, uint32_t alphabet, char *out, size_t numDwords, hipStream_t stream);
hipError_t dpx_launch_prim_eval(const int32_t *op, const uint32_t *a, const uint32_t *b, const uint32_t *c, size_t count,
                                uint32_t *res, uint32_t *pred, hipStream_t stream);

#endif
