/*
 * dpx_align.h -- C ABI of libdpxalign.so, the MI355X (gfx950) pairwise-alignment DP engine.
 *
 * This is the drop-in boundary for ONE hot path of mickgordinier/DPX_GPU_Genomics_Project:
 * the anti-diagonal wavefront matrix fill of a batch of independent pairwise alignments
 * (SURVEY.md section 8).  The reference has no FFI of its own -- its boundary is its C++ headers
 * (c++/SequenceAligner.h, c++/parseInput.h, c++/backtrack.h) and the `<<<grid,block>>>` launches in
 * its cuda/ *.cu mains.  Every entry point below names the reference interface it replaces.
 * Plain pointers and sizes only; no C++/torch types.  All functions return 0 (DPX_OK) or a negative
 * dpx_status; none of them exits the process.
 *
 * Thread-safety: every call is safe from concurrent host threads (the reference's CPU driver runs
 * 20 pthreads, c++/main.cpp:18-19,203); calls on the SAME dpx_batch must be serialised by the caller.
 */
#ifndef DPX_ALIGN_H
#define DPX_ALIGN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1: round 1.  2: + dpx_batch_create_on, dpx_batch_fill_timed, dpx_batch_last_fill_usec, dpx_batch_output_begin/_end/_take,
 * dpx_text_free, DPX_TUNE_PLACEMENT (round 2).  3: + dpx_pool_reserve, dpx_text_reserve, dpx_batch_last_output_usec, dpx_pack2, dpx_batch_create_packed2; dpx_batch_describe reports the
 * matrix pool (round 3); + DPX_KEEP_DIRECTIONS, dpx_batch_directions (detect them by the exported symbol: the number stays 3); + DPX_ALGO_ASW
 * (detect it by creating a batch: an older library returns DPX_ERR_INVALID for algo 4); + DPX_ALGO_BASW (likewise: DPX_ERR_INVALID for algo 5); + DPX_ALGO_ASG (likewise: DPX_ERR_INVALID for algo 6); + DPX_ALGO_BANW (likewise: DPX_ERR_INVALID for algo 7); + DPX_ALGO_BAXT (likewise: DPX_ERR_INVALID for algo 10); + dpx_batch_cigars_begin / _end, dpx_cigar_text (detect them by the exported symbol); + DPX_KEEP_LOCAL_BAND_DIRECTIONS (an older library ignores the bit: dpx_batch_describe then shows kernel=k_banded_fill / k_basw_fill).  Additions only: a caller built against an older version keeps working; dpx_abi_version() >= the version
 * a caller needs is the check. */
#define DPX_ABI_VERSION 3

typedef enum dpx_status {
    DPX_OK = 0,
    DPX_ERR_INVALID = -1,      /* bad argument (NULL, negative size, unknown algo ...) */
    DPX_ERR_NO_DEVICE = -2,    /* no usable gfx950 device / HIP runtime failure at init */
    DPX_ERR_HIP = -3,          /* a HIP call failed; dpx_last_error() has the text */
    DPX_ERR_RANGE = -4,        /* scores of this batch cannot be held in int16 cells */
    DPX_ERR_NOMEM = -5,        /* device or host allocation failed */
    DPX_ERR_NOT_FILLED = -6,   /* results requested before dpx_batch_fill() */
    DPX_ERR_NO_MATRIX = -7,    /* matrix / traceback requested from a DPX_SCORE_ONLY batch */
    DPX_ERR_UNSUPPORTED = -8   /* parameter combination the engine does not implement */
} dpx_status;

/* Algorithm selector.  Replaces the compile-time switch `#define LSW_ENABLE / LNW_ENABLE / ANW_ENABLE`
 * (c++/main.cpp:22-24) and the one-program-per-algorithm split of cuda/ *.cu. */
typedef enum dpx_algo {
    DPX_ALGO_LNW = 0, /* LinearNeedlemanWunsch   c++/LinearNeedlemanWunsch.cpp:89-135, cuda/LNW/ *.cu      */
    DPX_ALGO_LSW = 1, /* LinearSmithWaterman     c++/LinearSmithWaterman.cpp:70-114,  cuda/LinearSmithWaterman.cu */
    DPX_ALGO_ANW = 2, /* AffineNeedlemanWunsch   c++/AffineNeedlemanWunsch.cpp:167-240, cuda/AffineNeedlemanWunsch.cu */
    DPX_ALGO_BSW = 3, /* BandedSmithWaterman     python/LinearBandedSmithWaterman.py:62-104 (C++/CUDA twins are broken) */
    DPX_ALGO_ASW = 4, /* affine-gap (Gotoh) Smith-Waterman, no reference counterpart: ANW's D / I / H recurrence and tie order with
                         H = max(0, best) and zero borders; score = max H, end cell = its first cell in row-major order (LSW's rule);
                         the walk follows ANW's three states from there and stops where H = 0 (no end gaps); LSW's text block.  Same
                         dpx_params fields as ANW (band ignored).  Every flag ANW takes: matrices, DPX_SCORE_ONLY, DPX_KEEP_DIRECTIONS.
                         Added without an ABI bump: a library that predates it returns DPX_ERR_INVALID for algo 4. */
    DPX_ALGO_BASW = 5, /* banded affine-gap Smith-Waterman, no reference counterpart: ASW's parameters plus BSW's band B >= 1.  A cell
                         (i, j), 1 <= i <= m, 1 <= j <= n, is in the band when |i - j| <= B - 1 (BSW's rule).  In-band cells follow ASW's
                         recurrence and tie order: D = max(H_up + o + e, D_up + e), I = max(H_left + o + e, I_left + e), GAP_OPEN wins a
                         tie; best = H_diag + s, D >= best takes it, then I >= best takes it; H = max(0, best), move NONE where H == 0.
                         Every neighbour that is a border cell or lies outside the band reads H = 0, I = D = -infinity, so the first
                         in-band cell of a row or column always opens.  Cells outside the band: H = 0, and dpx_batch_matrix exports
                         H = I = D = 0 there, as on the borders.  Score = max H, end cell = its first cell in row-major order ((0, 0)
                         and 0 when every H is 0).  The walk is ASW's three-state walk from the end cell and stops where H == 0; it
                         cannot leave the band (an extension out of a cell outside the band costs -infinity + e, so GAP_OPEN wins there).
                         LSW's / ASW's text block.  B >= max(m, n) of the batch runs as ASW (same results); otherwise B <= 512, a wider
                         band that does not cover the matrix is DPX_ERR_UNSUPPORTED.  gapOpen = 0 gives BSW's H matrix with linear gap
                         gapExtend.  Matrices and DPX_SCORE_ONLY; DPX_KEEP_DIRECTIONS is DPX_ERR_UNSUPPORTED, as for BSW (4-bit codes per
                         in-band cell: DPX_KEEP_LOCAL_BAND_DIRECTIONS).
                         Added without an ABI bump or a new symbol: a library that predates it returns DPX_ERR_INVALID for algo 5. */
    DPX_ALGO_ASG = 6, /* affine-gap semi-global alignment ("fitting", "glocal", ends-free in the reference), no reference counterpart: the
                         whole query is aligned end to end against the stretch of the reference that fits it best; the reference before
                         and after that stretch costs nothing.  Same dpx_params fields as ANW; band is ignored.  Reference of length n
                         along columns j, query of length m along rows i.
                         Borders: H[0][j] = 0 for 0 <= j <= n (leading reference bases are free); H[i][0] = gapOpen + i*gapExtend for
                         i >= 1 (ANW's column border); I and D have virtual -infinity borders exactly as in ANW, so row 1 always opens
                         D and column 1 always opens I.
                         Cells: ANW's recurrence and tie order, unchanged: D = max(H_up + o + e, D_up + e), I = max(H_left + o + e,
                         I_left + e), GAP_OPEN wins a tie; best = H_diag + s (MATCH or MISMATCH), D >= best takes it (QUERY_DELETION),
                         then I >= best takes it (QUERY_INSERTION).  There is no zero floor.
                         Score = max over 0 <= j <= n of H[m][j]; the end cell is (m, j*) with j* the smallest such j (trailing
                         reference bases are free).  j = 0 takes part: when the whole query as one gap beats everything else the result
                         is (m, 0) with score o + m*e.  m = 0 gives score 0 at (0, 0); n = 0 with m > 0 gives o + m*e at (m, 0).  The
                         score may be zero or negative with a real path.
                         Walk: ANW's three-state walk from the end cell in state SCORING while i != 0 && j != 0; then the remaining i
                         query characters are emitted as deletions (ANW's column-0 tail); the remaining j reference characters are NOT
                         emitted: the walk stops at row 0.  The reference start column of the alignment is endCol minus the number of
                         non-'_' characters of the reference line (refStart of the pair's dpx_alignment record).
                         Text: the "<pair> | <score>\n" header, then the reference, relation and query lines; the path is printed
                         whatever the sign of the score, only m = 0 gives three empty lines (unlike LSW's zero-score case).
                         dpx_batch_matrix: row-major (m+1) x (n+1), H with the borders above, I and D with 0 on the borders, as for
                         ANW.  dpx_batch_directions: H plane NONE_MAIN along row 0 ((0, 0) included) and QUERY_DELETION down column 0
                         for i >= 1; I and D planes 0 on the borders.
                         Every flag ANW takes: matrices, DPX_SCORE_ONLY, DPX_KEEP_DIRECTIONS (int32 scores, references past 65 000
                         columns); packed2 input, dpx_align_batch, the output pipeline, dpx_batch_create_on and a caller's stream.
                         ASG(ref, qry).score == max over 0 <= a <= b <= n of ANW(ref[a:b], qry).score.
                         Added without an ABI bump or a new symbol: a library that predates it returns DPX_ERR_INVALID for algo 6. */
    DPX_ALGO_BANW = 7, /* banded affine-gap Needleman-Wunsch (global alignment between two anchors), no reference counterpart.  BASW's
                         dpx_params fields: match, mismatch, gapOpen o, gapExtend e, band B >= 1.  Reference of length n along columns
                         j, query of length m along rows i.
                         Band: a cell (i, j), 0 <= i <= m, 0 <= j <= n, is in the band when |i - j| <= B - 1 (BSW's rule; here it
                         applies to border cells too).
                         Borders: H[0][0] = 0; H[i][0] = o + i*e for 1 <= i <= B - 1; H[0][j] = o + j*e for 1 <= j <= B - 1 (ANW's
                         borders); I and D are -infinity on every border.  Outside the band H = I = D = -infinity.
                         Cells: for in-band cells with i, j >= 1, ANW's recurrence and tie order, unchanged: D = max(H_up + o + e,
                         D_up + e), I = max(H_left + o + e, I_left + e), GAP_OPEN wins a tie; best = H_diag + s (MATCH or MISMATCH),
                         D >= best takes it (QUERY_DELETION), then I >= best takes it (QUERY_INSERTION).  No zero floor; -infinity plus
                         anything is -infinity.  It follows that every in-band H is finite (the diagonal neighbour of an in-band cell
                         is in band), that I of a cell on the lower edge (i - j = B - 1) is -infinity and that D of a cell on the upper
                         edge (j - i = B - 1) is -infinity.
                         Score = H[m][n], end cell (m, n).  m = 0 gives o + n*e (0 when n = 0 as well), n = 0 gives o + m*e.
                         Admission: a global path exists only when |m - n| <= B - 1.  A batch that holds a pair with |m - n| >= B is
                         refused at create with DPX_ERR_UNSUPPORTED, and dpx_last_error() names the first such pair and the band it
                         would need; nothing is widened.  The caller chooses B, as a mapper sets its band from the length difference.
                         Covering band: B >= max(m, n) + 1 over the batch runs as ANW, with the same results (+1: at B = max(m, n) the
                         border cell (m, 0) is outside the band and I[m][1] is -infinity).  Otherwise B <= 512; a wider band that
                         does not cover is DPX_ERR_UNSUPPORTED, as for BASW.
                         Walk: ANW's three-state walk from (m, n) in SCORING while i != 0 && j != 0: I >= max(D, mm) goes to
                         INSERTION, else D >= mm to DELETION, else the diagonal; in a gap state GAP_OPEN applies when H + o + e >=
                         (I or D) + e at the neighbour, and a neighbour that is a border cell opens the gap.  Then ANW's two tails:
                         the remaining i as deletions, the remaining j as insertions.  The walk cannot leave the band.
                         Text: ANW's block (header, then the reference, relation and query lines), whatever the sign of the score.
                         dpx_batch_matrix: row-major (m+1) x (n+1); in-band H carries the borders above, I and D are 0 on in-band
                         borders (as for ANW), every plane is 0 outside the band (as for BASW), and an in-band I or D that is
                         -infinity exports as -32768; the range check keeps every finite value at or above -32767.
                         Matrices and DPX_SCORE_ONLY; DPX_KEEP_DIRECTIONS is DPX_ERR_UNSUPPORTED, as for BSW and BASW (4-bit
                         directions and int32 scores: DPX_KEEP_BAND_DIRECTIONS).  packed2
                         input, dpx_align_batch, the output pipeline, dpx_batch_create_on and a caller's stream as for BASW.
                         Added without an ABI bump or a new symbol: a library that predates it returns DPX_ERR_INVALID for algo 7. */
    /* 8 and 9 are unassigned: DPX_ERR_INVALID */
    DPX_ALGO_BAXT = 10 /* banded affine-gap extension alignment (what a read mapper runs past its first and last anchor; ksw2's extz,
                         BWA-MEM's extension), no reference counterpart: anchored at (0, 0), inside a band, ending wherever the score
                         peaks.  BANW's dpx_params fields, band B >= 1.  Reference of length n along columns j, query of length m
                         along rows i.
                         Band and borders: exactly BANW's.  A cell (i, j), 0 <= i <= m, 0 <= j <= n, is in the band when
                         |i - j| <= B - 1; H[0][0] = 0; in-band border cells carry o + k*e; I and D are -infinity on the borders;
                         everything outside the band is -infinity.
                         Cells: BANW's recurrence and tie order, unchanged, no zero floor.  Where BANW admits a pair, BAXT's H, I and D
                         equal BANW's cell for cell.
                         Score = the maximum of H over all in-band cells, border cells and (0, 0) included; it is therefore >= 0.
                         End cell = the first cell in row-major order that holds the maximum (the LSW / BASW rule with row 0 and
                         column 0 taking part).  A score of 0 always ends at (0, 0).
                         BAXT(ref, qry, B).score == max over in-band (i, j) of BANW(ref[:j], qry[:i], B).score.
                         Admission: none.  Any m and n, zero included; when |m - n| >= B the cell (m, n) is simply never reached.
                         Walk: BANW's three-state walk from the end cell in SCORING while i != 0 && j != 0, then ANW's two tails; the
                         path always reaches the anchor (0, 0).  The ungapped characters of the reference line are ref[:endCol],
                         those of the query line qry[:endRow].  The walk cannot leave the band.
                         Text: ANW's block (header, then three lines); the lines are empty when the end cell is (0, 0).
                         dpx_batch_matrix: as for BANW (H carries the in-band borders, I and D are 0 there, every plane is 0 outside
                         the band, an in-band -infinity exports as -32768).
                         Band limit: B <= 512; a wider band is DPX_ERR_UNSUPPORTED even when it would cover the matrix -- no unbanded
                         extension kernel exists to fall back on.  A band up to 512 that covers the matrix runs the banded kernel like
                         any other band.
                         Range: BANW's int16 bounds, and m + n <= 65000 (the kernel packs the step index into 16 bits, as BASW's);
                         otherwise DPX_ERR_RANGE.
                         Matrices and DPX_SCORE_ONLY; DPX_KEEP_DIRECTIONS is DPX_ERR_UNSUPPORTED, as for the other banded
                         algorithms (4-bit directions, int32 scores and no m + n limit: DPX_KEEP_BAND_DIRECTIONS).  packed2 input, dpx_align_batch, the output pipeline, dpx_batch_create_on and a caller's stream
                         as for BANW.  z-drop termination, ksw2's "best score reaching the end of the query" and an end bonus are
                         per-batch settings of this algorithm: dpx_batch_set_extension below.
                         Added without an ABI bump or a new symbol: a library that predates it returns DPX_ERR_INVALID for algo 10. */
} dpx_algo;

/* Identical in layout to the reference's `struct seqPair` (c++/parseInput.h:22-29): byte offsets into the
 * flat `sequences` buffer parseInput() produced, plus lengths. */
typedef struct dpx_seq_pair {
    int32_t referenceIdx;
    int32_t referenceSize;
    int32_t queryIdx;
    int32_t querySize;
} dpx_seq_pair;

/* Scoring parameters: the reference's argv `-match -mismatch -open(-gap) -extend` (c++/main.cpp:133-150,
 * cuda/LinearSmithWaterman.cu:205-216).  LNW/LSW/BSW use gapOpen as THE linear gap (main.cpp:52,77). */
typedef struct dpx_params {
    int32_t algo;      /* dpx_algo */
    int32_t match;
    int32_t mismatch;
    int32_t gapOpen;   /* linear gap for LNW/LSW/BSW; gap-open for ANW / ASW / BASW / ASG / BANW / BAXT */
    int32_t gapExtend; /* ANW / ASW / BASW / ASG / BANW / BAXT only */
    int32_t band;      /* BSW / BASW / BANW / BAXT: cells with |i-j| <= band-1 are computed */
} dpx_params;

/* dpx_batch_create flags */
#define DPX_KEEP_MATRICES 0x0u /* default: write the int16 score matrices (H; H,I,D for ANW / ASW / BASW / ASG / BANW / BAXT) to HBM */
#define DPX_SCORE_ONLY    0x1u /* no matrix writeback (not HBM-bound; never used for the roofline figure) */
#define DPX_TIME_FILLS    0x2u /* bracket every dpx_batch_fill() with HIP events: dpx_batch_last_fill_usec() */
#define DPX_TUNE_PLACEMENT 0x4u /* the batch will be filled many times: time its matrix pool (>= 1 GiB) with hipMemset and shop for a better
                                   one with the batch's OWN FILL on four more candidate pools (the same fill runs 2 - 27 % apart on
                                   two pools of the same construction); every candidate's times go into dpx_batch_describe's pool_* fields */
#define DPX_KEEP_DIRECTIONS 0x8u /* LNW / LSW / ANW / ASW / ASG: keep one 4-bit direction code per cell instead of the int16 score matrices, compute in
                                    int32 (the reference's evolved kernels keep directions only, cuda/LNW/LinearNeedlemanWunschV6.cu:167).  Same
                                    scores, end cells, text and tracebacks as a DPX_KEEP_MATRICES batch; half a byte per cell plus ~32 B of stripe
                                    padding per query row (about a quarter of an int16 H batch's bytes, a twelfth of ANW's H/I/D, from
                                    a few hundred rows on; short reads keep a larger fraction); scores may exceed int16 (bounds checked against 2^28) and references 65 000 columns.
                                    dpx_batch_matrix() returns DPX_ERR_NO_MATRIX, dpx_batch_directions() exports the codes.  With
                                    DPX_SCORE_ONLY: DPX_ERR_INVALID; with BSW / BASW / BANW / BAXT: DPX_ERR_UNSUPPORTED, with or without 0x10
                                    (BANW and BAXT keep directions under DPX_KEEP_BAND_DIRECTIONS below, BSW and BASW under DPX_KEEP_LOCAL_BAND_DIRECTIONS). */
#define DPX_KEEP_BAND_DIRECTIONS 0x10u /* BANW / BAXT: keep one 4-bit direction code per IN-BAND cell instead of the three int16 planes, compute in int32
                                    (k_bdir_fill; half a byte per in-band cell in whole 1-KiB chunks, a twelfth of the matrix batch's bytes).
                                    The definitions of BANW and BAXT do not change: same scores, end cells, traceback lines, text blocks and
                                    CIGAR records as a DPX_KEEP_MATRICES batch wherever that batch is admitted -- and batches it refuses with
                                    DPX_ERR_RANGE run: bounds are BANW's, checked against 2^28, and BAXT has no m + n <= 65000 limit here.
                                    dpx_batch_matrix() returns DPX_ERR_NO_MATRIX.  dpx_batch_directions() exports c++/backtrack.h enums: in-band
                                    cells with i, j >= 1 carry MATCH / MISMATCH / QUERY_INSERTION / QUERY_DELETION in DPX_MAT_H and GAP_OPEN /
                                    GAP_EXTEND in DPX_MAT_I / DPX_MAT_D (I on the band's lower edge and D on its upper edge: GAP_OPEN,
                                    -infinity >= -infinity); in-band borders of H are ANW's (QUERY_DELETION down column 0, QUERY_INSERTION
                                    along row 0, NONE_MAIN at (0, 0)), borders of I and D are 0; every plane is 0 outside the band.
                                    A separate bit because 0x8 on a banded algorithm is pinned to DPX_ERR_UNSUPPORTED, and stays so.
                                    With DPX_SCORE_ONLY: DPX_ERR_INVALID.  With another algorithm than BANW / BAXT: DPX_ERR_UNSUPPORTED (BSW /
                                    BASW: DPX_KEEP_LOCAL_BAND_DIRECTIONS).  Band > 512 (BANW: not covering): DPX_ERR_UNSUPPORTED, BANW's admission rule
                                    |m - n| < B unchanged, as for matrix batches.  A BANW band that covers the matrix (B >= max(m, n) + 1)
                                    runs as an ANW DPX_KEEP_DIRECTIONS batch (kernel_algo=ANW), the fall-back the matrix batch takes.
                                    dpx_batch_set_extension and dpx_batch_set_substitution on such a batch: DPX_ERR_UNSUPPORTED, the batch is
                                    left as it was (both keep refusing: dpx_batch_set_direction_scoring is the way in).  DPX_TIME_FILLS, dpx_batch_fill_timed, repeated fills, a caller's
                                    stream, dpx_batch_create_on, packed2 input, the output pipeline and dpx_batch_cigars_* as for a BANW
                                    matrix batch; DPX_TB_WALK has no effect (one walk, k_bdir_traceback).  Strings are staged in LDS as for
                                    BANW; where four waves' strings do not fit a workgroup the fill runs one-wave workgroups, and a pair
                                    whose two strings exceed ~160 KB is DPX_ERR_UNSUPPORTED.
                                    Added without an ABI bump or a new symbol.  Detecting it: a library that predates the flag ignores the
                                    bit and builds an int16 matrix batch -- dpx_batch_describe then shows kernel=k_banw_fill / k_baxt_fill
                                    (this library: kernel=k_bdir_fill, or k_affine_dir under a covering BANW band) and dpx_batch_directions
                                    returns DPX_ERR_NO_MATRIX. */
#define DPX_KEEP_LOCAL_BAND_DIRECTIONS 0x40u /* BSW / BASW: keep one 4-bit direction code per IN-BAND cell (i, j >= 1) instead of the int16 planes, compute in
                                    int32 (k_bdl_fill; dpx_banddir.h's layout unchanged: half a byte per in-band cell in whole 1-KiB chunks, a quarter
                                    of BSW's bytes and a twelfth of BASW's).  The definitions of BSW and BASW do not change: same scores, end
                                    cells, traceback lines, text blocks, dpx_alignment records and CIGAR ops as a DPX_KEEP_MATRICES batch wherever
                                    that batch is admitted -- and batches it refuses with DPX_ERR_RANGE run: the bounds are LSW's (BSW) and ASW's
                                    (BASW; a band only removes paths), checked against 2^28, with no n or m + n limit.
                                    dpx_batch_matrix() returns DPX_ERR_NO_MATRIX.  dpx_batch_directions() exports c++/backtrack.h enums, row-major
                                    (m+1) x (n+1); every plane is 0 on the borders and outside the band.  BSW, DPX_MAT_H only: NONE_MAIN iff
                                    t = max(up, left, corner) < 0, else QUERY_DELETION when up == H, else QUERY_INSERTION when left == H, else
                                    MATCH / MISMATCH -- a cell with t == 0 has H == 0 and still carries a move (the walk stops there all the
                                    same); the other selectors answer what an LSW direction batch answers.  BASW: DPX_MAT_H is NONE_MAIN where
                                    H == 0; DPX_MAT_I / DPX_MAT_D are GAP_OPEN / GAP_EXTEND for every in-band cell (on the band's edges the
                                    neighbour outside it reads H = 0, I = D = -infinity, so the cell opens).
                                    A separate bit because 0x10 on BSW / BASW is pinned to DPX_ERR_UNSUPPORTED, as 0x8 is, and both stay so.
                                    With DPX_SCORE_ONLY, 0x10 or 0x20: DPX_ERR_INVALID.  With 0x8 on BSW / BASW: DPX_ERR_UNSUPPORTED (the rule
                                    above wins).  With another algorithm than BSW / BASW: DPX_ERR_UNSUPPORTED.  Band > 512 and not covering:
                                    DPX_ERR_UNSUPPORTED.  A band that covers the matrix (B >= max(m, n) over the batch) runs as an LSW / ASW
                                    DPX_KEEP_DIRECTIONS batch (kernel_algo=LSW / ASW, k_linear_dir / k_asw_dir), the fall-back the matrix batch
                                    takes.  Strings are staged in LDS as for 0x10: one-wave workgroups where four waves' strings do not fit, and
                                    DPX_ERR_UNSUPPORTED where one wave's do not.  DPX_TIME_FILLS, dpx_batch_fill_timed, repeated fills, a caller's
                                    stream, dpx_batch_create_on, packed2 input, the output pipeline and dpx_batch_cigars_* as for a BSW / BASW
                                    matrix batch; DPX_TB_WALK has no effect (one walk, k_bdl_traceback).  Every setter refuses as it does for
                                    a BSW / BASW matrix batch (z-drop, end bonus, two-piece gaps and reversed pairs are not built for these
                                    batches), and leaves the batch as it was; a substitution table comes through the batches' own setter,
                                    dpx_batch_set_local_direction_table (k_bdlt_fill).
                                    Added without an ABI bump or a new symbol.  Detecting it: a library that predates the flag ignores the
                                    bit and builds an int16 matrix batch -- dpx_batch_describe then shows kernel=k_banded_fill /
                                    k_banded_fill_pk / k_basw_fill (this library: kernel=k_bdl_fill, or k_linear_dir / k_asw_dir under a
                                    covering band) and dpx_batch_directions returns DPX_ERR_NO_MATRIX. */
#define DPX_LONG_SCORES 0x100u /* BANW / BAXT / BSW / BASW: the scoring pass of long banded pairs.  Legal only together with exactly one of 0x10
                                    (BANW / BAXT) or 0x40 (BSW / BASW), and means that direction batch with nothing stored but the results: its
                                    definitions, int32 arithmetic, range check against 2^28, absence of any n or m + n limit and strings staged in
                                    LDS (one-wave workgroups where four waves' strings do not fit, DPX_ERR_UNSUPPORTED where one wave's do not),
                                    and no pool (k_bscore_fill on 0x10, k_lscore_fill on 0x40).  "Score everything here, realign the hits on a
                                    direction batch": pairs the int16 DPX_SCORE_ONLY batch refuses with DPX_ERR_RANGE run.
                                    Results.  dpx_batch_results and dpx_batch_device_results equal what the same pairs give on the 0x10 / 0x40
                                    batch without this bit; under z-drop / end bonus dpx_batch_extensions is equal too, the chosen end, lastDiag
                                    and flags included; wherever the int16 DPX_SCORE_ONLY batch admits the pairs, they equal that batch's.
                                    No pool.  dpx_batch_info reports matrixBytes == 0; dpx_batch_matrix, dpx_batch_directions,
                                    dpx_batch_traceback, dpx_batch_output_begin, dpx_batch_cigars_begin and dpx_batch_diffs_begin answer
                                    DPX_ERR_NO_MATRIX, as on a DPX_SCORE_ONLY batch; DPX_TUNE_PLACEMENT is ignored (there is no pool to shop
                                    for).  DPX_TIME_FILLS, dpx_batch_fill_timed, repeated fills, a caller's stream, dpx_batch_create_on and
                                    packed2 input work as for the direction batch.  (dpx_align_batch takes no flags and stays the int16 one-shot.)
                                    Setters.  On 0x10 | 0x100: dpx_batch_set_direction_scoring (a table on BANW; table, z-drop and end bonus on
                                    BAXT) and dpx_batch_set_reversed, with their arguments, lifecycle and invalidation rules (the results stay
                                    in the reversed frame; there are no lines to flip).  On 0x40 | 0x100: dpx_batch_set_local_direction_table.
                                    Every other setter refuses as it does on the direction batch and leaves the batch as it was.
                                    Flags.  Without 0x10 / 0x40, with both, or with DPX_SCORE_ONLY: DPX_ERR_INVALID.  With 0x8: the rules for 0x8
                                    on a banded algorithm win (DPX_ERR_UNSUPPORTED).  With 0x20 or 0x80: DPX_ERR_UNSUPPORTED -- the two-piece
                                    steps are not built for this pass, so dpx_batch_set_second_gap refuses too.  Wrong algorithm for the storage
                                    bit: DPX_ERR_UNSUPPORTED, as without this bit.
                                    Bands.  Band > 512: DPX_ERR_UNSUPPORTED always -- no unbanded int32 score-only kernel exists to fall back on.
                                    A band up to 512 that covers the matrix runs the band kernel like any other band (BAXT's rule, here for all
                                    four); BANW keeps its admission rule |m - n| < B.
                                    dpx_batch_describe shows kernel=k_bscore_fill / k_lscore_fill and store=0, adds ` subst=<alphabet>` under a
                                    table and ` zdrop=<z> end_bonus=<b>` in extension mode, and names no traceback= and no matrix=.
                                    Added without an ABI bump or a new symbol.  Detecting it: a library that predates the flag ignores the bit
                                    and builds the direction batch -- dpx_batch_describe then says kernel=k_bdir_fill / k_bdl_fill and
                                    dpx_batch_directions succeeds. */

/* matrix selectors for dpx_batch_matrix / dpx_batch_directions */
#define DPX_MAT_H 0 /* scoring matrix   (reference: memo / scoringMemo)            */
#define DPX_MAT_I 1 /* the affine algorithms' horizontal-gap matrix (queryInsertionMemo) */
#define DPX_MAT_D 2 /* the affine algorithms' vertical-gap matrix   (queryDeletionMemo)  */

typedef struct dpx_batch dpx_batch; /* opaque, device-resident batch of pairs */

/* ---- process / device ------------------------------------------------------------------------------ */

/* Bind the calling process to HIP device `device` (one process per GPU; multi-GPU = one rank per device).
 * Replaces cudaGetDeviceCount/cudaGetDeviceProperties(0) at the top of every cuda/ *.cu main
 * (cuda/LinearSmithWaterman.cu:176-190).  Idempotent. */
int dpx_init(int device);
int dpx_device_count(int *count);
/* name (<=255 chars), CU count, HBM bytes of the bound device; any pointer may be NULL */
int dpx_device_info(char *name, size_t nameCap, int *computeUnits, size_t *hbmBytes);
int dpx_shutdown(void);
/* Allocate `count` (1..8; one if `bytes` >= 16 GiB) matrix pools of `bytes` each on the default device and park them for the batches to come (any batch
 * whose matrices fit takes a parked pool instead of allocating), together with two streams per pool for those batches.  Meant for a helper thread while the caller parses its input:
 * the reference sizes its device buffers once, before the batch loop (cuda/LNW/LinearNeedlemanWunschV14.cu:144-213). */
int dpx_pool_reserve(size_t bytes, int count);
/* The same for `count` (1..9) pinned host buffers of `bytes` (<= 1 GiB) each, which the result text of the batches to come is copied
 * into (dpx_batch_output_end / _take; a parked buffer of up to 32 MiB serves any text of 2 MiB or more that fits). */
int dpx_text_reserve(size_t bytes, int count);
const char *dpx_strerror(int status);
const char *dpx_last_error(void); /* thread-local text of the last HIP failure */
int dpx_abi_version(void);

/* ---- batched path (replaces the batched cuda mains, cuda/LNW/LinearNeedlemanWunschV19.cu:422-612) --- */

/* Copy `sequences[0..numBytes)` and pairs[firstPair .. firstPair+numPairs) to HBM and allocate result
 * storage.  Replaces cudaMalloc+cudaMemcpy of sequences/seqPair[] (V19.cu:422-440) and the per-batch matrix
 * pool (V19.cu:488-529).  Sequences are plain bytes ('\0'-separated as parseInput leaves them); any byte
 * value is legal, matching is plain byte equality (BANW / BAXT: or a substitution table, dpx_batch_set_substitution).  Zero-length sequences are legal. */
int dpx_batch_create(const dpx_params *params, const char *sequences, size_t numBytes, const dpx_seq_pair *pairs,
                     size_t firstPair, size_t numPairs, unsigned flags, dpx_batch **out);

/* The same on an explicit device (0 .. dpx_device_count()-1; -1 = the default device): one host process can drive
 * several GPUs, each batch lives on the device it was created on and every call on it runs there.  The class surface
 * uses this to spread the batches it forms from the reference's 20 threads over all visible devices (hostcpp/DpxPair.cpp;
 * rehearsed with several leaders on one GPU only, never run on a multi-GPU box); one process per GPU (dpx_init(rank)) remains
 * the layout of the batched driver and of bench.py.  device >= count is DPX_ERR_INVALID. */
int dpx_batch_create_on(int device, const dpx_params *params, const char *sequences, size_t numBytes, const dpx_seq_pair *pairs,
                        size_t firstPair, size_t numPairs, unsigned flags, dpx_batch **out);

/* ---- 2-bit packed input (the input side of c++/parseInput.cpp:78-112) -------------------------------------------
 * The reference keeps one byte per base.  A caller whose sequences use at most four distinct byte values (DNA: "ACGT", the
 * reference's datasets: "0123") may hand the engine four bases per byte: base k sits in bits 2*(k%4) of byte k/4, alphabet[code] is
 * the byte a code stands for, and the pairs keep the reference's struct seqPair -- their indices count bases of the packed buffer
 * exactly as they counted bytes of the flat one.  The engine moves a quarter of the bytes over PCIe and expands them on the device
 * (k_unpack2) into the byte buffer that the fill, traceback and output kernels read: results, matrices and printed text are
 * those of the byte batch.  dpx_pack2() is the host side: it derives the alphabet from the bytes inside the pairs' ranges (order of
 * first appearance) and packs `sequences` (bytes outside every pair, e.g. parseInput's separators, become code 0);
 * DPX_ERR_UNSUPPORTED when the pairs use more than four byte values (the caller keeps dpx_batch_create).  `packed` must hold
 * (numBytes + 3) / 4 bytes. */
int dpx_pack2(const char *sequences, size_t numBytes, const dpx_seq_pair *pairs, size_t numPairs, uint8_t alphabet[4], uint8_t *packed);
int dpx_batch_create_packed2(int device, const dpx_params *params, const uint8_t *packed, size_t numBases, const uint8_t alphabet[4],
                             const dpx_seq_pair *pairs, size_t firstPair, size_t numPairs, unsigned flags, dpx_batch **out);

/* Launch the DP fill for every pair of the batch on `stream` (a hipStream_t, or NULL for the batch's own
 * stream).  Asynchronous.  Replaces `needleman_wunsch_kernel<<<BATCH/2,32,smem>>>` (V19.cu:536),
 * `smith_waterman_kernel<<<1,32>>>` (cuda/LinearSmithWaterman.cu:263) and
 * `affine_needleman_wunsch_kernel<<<1,32>>>` (cuda/AffineNeedlemanWunsch.cu:338).  May be called repeatedly.
 * A caller-owned stream must stay valid until the batch has been synchronised or destroyed: dpx_batch_destroy()
 * waits on the stream of the last fill before it parks the batch's buffers for reuse by the next batch.
 * (The inputs of a small batch are still on their way when dpx_batch_create() returns -- one asynchronous copy on the batch's own
 * stream; the first fill on a caller's stream waits for it on the host, fills on the batch's stream are simply ordered behind it.) */
int dpx_batch_fill(dpx_batch *b, void *stream);

/* Run `repeats` fills back-to-back and return the mean device time of one fill in microseconds, measured with
 * hipEvents on the launch stream (the reference's kernel_time accumulator, V19.cu:531-586). */
int dpx_batch_fill_timed(dpx_batch *b, int repeats, double *usecPerFill);

/* Device time of the most recent dpx_batch_fill() of a batch created with DPX_TIME_FILLS, without stalling the launch:
 * the events are recorded on the fill's stream, this call waits only for the second one (the reference accumulates
 * kernel_time the same way around its launches, V19.cu:531-586, but synchronously). */
int dpx_batch_last_fill_usec(dpx_batch *b, double *usec);
/* The same for the device side of the most recent dpx_batch_output_begin(): traceback + text kernels (the reference's
 * backtracking() launch, V19.cu:546-560), without the D2H copies. */
int dpx_batch_last_output_usec(dpx_batch *b, double *usec);

int dpx_batch_sync(dpx_batch *b); /* cudaDeviceSynchronize analogue for this batch's stream */

/* Device pointers of the int32 result arrays (numPairs each) for collectives (RCCL gather of scores).
 * endRow/endCol are the LSW/BSW start cell of the traceback (first strict max in row-major order,
 * c++/LinearSmithWaterman.cpp:145-157); for LNW/ANW they are (m, n). */
int dpx_batch_device_results(dpx_batch *b, void **dScores, void **dEndRow, void **dEndCol);

/* D2H of the per-pair results (any pointer may be NULL).  Replaces cudaMemcpy of similarityScores (V19.cu:590). */
int dpx_batch_results(dpx_batch *b, int32_t *scores, int32_t *endRow, int32_t *endCol);

/* Export one pair's matrix as the reference lays it out: row-major (m+1) x (n+1) int16 including the border
 * row/column (memo[i][j], c++/LinearSmithWaterman.cpp:14-17; cuda scoringMatrix[row*numCols+col]).  `out` is host
 * memory of (m+1)*(n+1) int16.  On the device the matrix lives in the engine's wavefront-tiled layout
 * (DESIGN.md); this call un-tiles it with a device kernel and copies it back. */
int dpx_batch_matrix(dpx_batch *b, size_t pair, int which, int16_t *out);

/* Export one pair's direction matrix of a DPX_KEEP_DIRECTIONS batch as the reference's back-trackers read it: row-major (m+1) x (n+1)
 * uint8 including the border row / column, values of c++/backtrack.h -- `which` DPX_MAT_H: enum directionMain (NONE_MAIN 0, MATCH 1,
 * MISMATCH 2, QUERY_INSERTION 3, QUERY_DELETION 4; LNW / ANW borders: QUERY_DELETION down column 0, QUERY_INSERTION along row 0;
 * LSW: NONE_MAIN where the best candidate is negative, c++/LinearSmithWaterman.cpp:106-109; ASW: NONE_MAIN wherever H == 0, borders
 * included; ASG: NONE_MAIN along row 0, QUERY_DELETION down column 0); DPX_MAT_I / DPX_MAT_D (ANW / ASW / ASG):
 * enum directionIndel (GAP_OPEN 1, GAP_EXTEND 2; 0 on the borders).  DPX_ERR_NO_MATRIX on a batch without the flag. */
int dpx_batch_directions(dpx_batch *b, size_t pair, int which, uint8_t *out);

/* Device traceback of one pair from the stored matrices, with the reference's tie rules.
 * Produces the three lines the reference prints (reference / relation / query; c++/backtrack.cpp:21-356).
 * Each buffer needs m+n+1 bytes; *len receives the alignment length. */
int dpx_batch_traceback(dpx_batch *b, size_t pair, char *refLine, char *relLine, char *qryLine, int32_t *len);

/* The whole batch's result text, formatted on the device exactly as c++/main.cpp prints it: per pair
 *     "<pair number> | <score>\n<reference line>\n<relation line>\n<query line>\n"
 * (three empty lines for a zero-score local alignment, c++/LinearSmithWaterman.cpp:253-257), blocks in batch order, pair
 * numbers counted from `firstPairNumber`.  Replaces the per-pair backtracking + string packing of the batched CUDA mains
 * (cuda/LNW/LinearNeedlemanWunschV15.cu:168-172,372-425: packed variable-length result strings, one D2H of the real
 * bytes; V19.cu:546-579 prints them).  _begin() is asynchronous (device traceback, block lengths, exclusive scan, packed
 * copy, D2H of the offsets on the batch's stream); _end() waits, copies exactly the bytes of the text to pinned host memory
 * and returns it: `*text` (`*bytes` long, also NUL-terminated) and `*offsets` (numPairs + 1 byte offsets of the blocks)
 * stay valid until the batch is filled again or destroyed.  Two batches can be in flight: fill of batch k+1 overlaps
 * traceback + D2H of batch k. */
int dpx_batch_output_begin(dpx_batch *b, uint64_t firstPairNumber);
int dpx_batch_output_end(dpx_batch *b, const char **text, size_t *bytes, const uint64_t **offsets);
/* Like _end(), but the caller takes the (pinned) text buffer over and the batch can be destroyed at once -- its matrix pool
 * is then free for the next batch while a printer thread is still writing the text (the reference prints batch k-1
 * from host strings while batch k runs, V19.cu:546-579).  Give the buffer back with dpx_text_free(). */
int dpx_batch_output_take(dpx_batch *b, char **text, size_t *bytes);
int dpx_text_free(char *text);

/* ---- CIGARs and alignment coordinates of the whole batch (what a mapper writes into a SAM or PAF record) -------------------
 * The traceback lines, run-length encoded on the device: one fixed-size record per pair and one packed array of ops for the batch,
 * instead of three (m + n)-byte text lines per pair.  Every algorithm, DPX_KEEP_MATRICES and DPX_KEEP_DIRECTIONS batches; a
 * DPX_SCORE_ONLY batch is DPX_ERR_NO_MATRIX.  No reference counterpart.  Added without an ABI bump: detect the three functions by
 * the exported symbol.
 *
 * Columns of the three lines are classified by their relation and query-line characters:
 *     relation '*'                      '=' (DPX_CIGAR_OP_EQ)  match, consumes both sequences
 *     relation '|'                      'X' (DPX_CIGAR_OP_X)   mismatch, consumes both
 *     relation ' ', query line '_'      'D' (DPX_CIGAR_OP_D)   consumes the reference only (the QUERY_INSERTION move)
 *     relation ' ', anything else       'I' (DPX_CIGAR_OP_I)   consumes the query only (the QUERY_DELETION move)
 * Sequences that themselves contain the byte '_' are classified by the same rule: a query '_' in a gap column of the reference reads
 * as 'D'.  Ops are in path order from the start of the alignment to its end cell (left to right along the lines); an op is
 * (length << 4) | code with BAM's code numbers; the lengths of a pair's ops sum to its alignment length.  Under DPX_CIGAR_M '=' and
 * 'X' columns merge into 'M' runs (matches and mismatches are still counted apart).
 * refEnd = the end column and qryEnd = the end row of the results call; refStart = refEnd - (matches + mismatches + deletions),
 * qryStart = qryEnd - (matches + mismatches + insertions).  An empty alignment (a zero-score local alignment, m = 0 under ASG, a BAXT
 * pair ending at (0, 0)) has numOps = 0 and start == end.  opsOffset is the exclusive prefix sum of numOps in batch order. */
typedef struct dpx_alignment {      /* 48 bytes */
    uint64_t opsOffset;             /* index of this pair's first op in the batch's ops array */
    int32_t  numOps;
    int32_t  refStart, refEnd;      /* half-open, 0-based: the alignment covers ref[refStart, refEnd) */
    int32_t  qryStart, qryEnd;      /* ... and qry[qryStart, qryEnd) */
    int32_t  matches, mismatches;   /* columns whose relation character is '*' / '|' */
    int32_t  insertions, deletions; /* columns that consume the query only / the reference only */
    int32_t  reserved;              /* 0 */
} dpx_alignment;

#define DPX_CIGAR_OP_M  0u
#define DPX_CIGAR_OP_I  1u
#define DPX_CIGAR_OP_D  2u
#define DPX_CIGAR_OP_EQ 7u
#define DPX_CIGAR_OP_X  8u          /* BAM's numbering; an op is (length << 4) | code */
#define DPX_CIGAR_EXTENDED 0x0u     /* '=' and 'X' kept apart (default) */
#define DPX_CIGAR_M        0x1u     /* '=' and 'X' columns are both M and merge into one run */

/* _begin is asynchronous on the batch's stream (behind a fill on a caller's stream it orders itself with an event): the device
 * traceback if the lines of this fill do not exist yet (the same walk the text pipeline chooses), then count, scan and write kernels
 * and the D2H of the records.  _end waits and copies exactly numPairs records and *numOps ops to pinned host memory; the pointers
 * stay valid until the batch is filled again, the next _begin, or destroy.  The text pipeline and this one may follow the same fill in
 * either order.  Unknown flag bits: DPX_ERR_INVALID; not filled, or _end without a _begin since the last fill: DPX_ERR_NOT_FILLED. */
int dpx_batch_cigars_begin(dpx_batch *b, unsigned flags);
int dpx_batch_cigars_end(dpx_batch *b, const dpx_alignment **records, const uint32_t **ops, uint64_t *numOps);
/* Host only (no device, no init needed): the SAM text of `numOps` ops ("12=1X3D", letters MID=X; "*" for none) and a terminating
 * NUL into out[0..cap); *len = its length without the NUL.  A cap too small returns DPX_ERR_INVALID with *len = the length needed;
 * an op code outside {0, 1, 2, 7, 8} returns DPX_ERR_INVALID. */
int dpx_cigar_text(const uint32_t *ops, size_t numOps, char *out, size_t cap, size_t *len);

/* ---- Difference strings of the whole batch: SAM's MD tag and minimap2's short cs tag ----------------------------------------
 * What a SAM or PAF record needs beyond the CIGAR, built on the device from the same traceback lines: one packed text buffer per
 * kind and numPairs + 1 byte offsets, instead of three (m + n)-byte lines per pair tokenised on the host.  Every algorithm and
 * storage mode the CIGAR path serves; a DPX_SCORE_ONLY batch is DPX_ERR_NO_MATRIX.  No reference counterpart.  Added without an ABI
 * bump: detect the two functions by the exported symbol.
 *
 * NM, the edit distance, has no entry point of its own: NM = mismatches + insertions + deletions of the pair's dpx_alignment record.
 *
 * Columns of a pair's three lines are classified exactly as the CIGAR section classifies them:
 *     relation '*',           any query-line byte        '='
 *     relation '|',           any query-line byte        'X'
 *     anything else,          query-line byte '_'        'D'
 *     anything else,          anything else              'I'
 * ref[c] and qry[c] are the bytes of the reference line and the query line at column c.  Columns run from the start of the alignment
 * to its end cell.  Under dpx_batch_set_reversed the lines are already in the caller's orientation when these kernels see them, so
 * the strings come out in the caller's orientation.
 *
 * MD is what `samtools calmd` writes:
 *     n = 0; prev = none
 *     for each column c:
 *         '=' : n += 1
 *         'X' : emit decimal(n), emit ref[c]; n = 0
 *         'D' : if prev != 'D': emit decimal(n), emit '^'; n = 0
 *               emit ref[c]
 *         'I' : nothing          (an insertion does not break a match run, but it does end a deletion run)
 *         prev = class of c
 *     emit decimal(n)
 * decimal(n) has no leading zeros; decimal(0) is "0".  An empty alignment gives "0".  Reference bytes are emitted as they are: there
 * is no case folding, and a reference byte that is a digit or '^' makes the string ambiguous (it is emitted all the same).
 *
 * cs is minimap2's short form.  Take the maximal runs of equal class, which are the ops of DPX_CIGAR_EXTENDED:
 *     an '=' run of length L emits ':' then decimal(L)
 *     every 'X' column emits '*', lc(ref[c]), lc(qry[c])
 *     an 'I' run emits '+' then lc(qry[c]) for each column
 *     a 'D' run emits '-' then lc(ref[c]) for each column
 * lc adds 32 to the bytes 'A'..'Z' and leaves every other byte alone.  An empty alignment gives the empty string.  The long form
 * (matched bases spelled out) is not built.
 *
 * Length bound.  A pair's MD or cs never exceeds 3 * cap bytes, where cap = (m + n + 1 + 3) & ~3 is the capacity of one of its lines
 * and len <= m + n its alignment length, so cap >= len + 1.  cs: an 'X' column emits 3 bytes, an 'I' or 'D' column 2 at the start of
 * its run and 1 inside it, and an '=' run of L >= 1 columns 1 + digits(L) <= 3 * L bytes: at most 3 bytes per column, 3 * len in
 * all.  MD: a number of d digits in front of a breaker stands for at least d '=' columns that emit nothing else, except that a "0"
 * costs one byte without any; so the densest pattern is D X D X ..., "0^" + base for a D and "0" + base for an X, 2.5 bytes per
 * column, and with the closing number MD <= (5 * len + 1) / 2 + 1 <= 3 * (len + 1) <= 3 * cap.  Hence one device text buffer of the
 * size of the batch's line buffer holds every kind's worst case, and count, scan and write run without a host round trip. */
#define DPX_DIFF_MD 0x1u
#define DPX_DIFF_CS 0x2u

/* _begin (`kinds`: one or both bits) is asynchronous on the batch's stream (behind a fill on a caller's stream it orders itself with an
 * event): the device traceback if the lines of this fill do not exist yet, so the walk runs once whichever of text, CIGARs and diffs
 * comes first; then per requested kind count, scan and write kernels and the D2H of the numPairs + 1 offsets.  _end (`kind`: exactly
 * one bit that a _begin since the last fill was given) waits and copies exactly offsets[numPairs] bytes to pinned host memory: *text
 * holds the pairs' strings back to back with no separators and one NUL after the last byte, *offsets are numPairs + 1 byte offsets,
 * *bytes is offsets[numPairs].  The pointers stay valid until the batch is filled again, the next _begin of that kind, or destroy.
 * The text pipeline, the CIGAR path and this one may follow the same fill in any order.  `kinds` 0 or with unknown bits, `kind` not
 * exactly one known bit: DPX_ERR_INVALID; not filled, or _end for a kind not begun since the last fill: DPX_ERR_NOT_FILLED.  A batch
 * of zero pairs gives *bytes = 0 and one offset of 0. */
int dpx_batch_diffs_begin(dpx_batch *b, unsigned kinds);
int dpx_batch_diffs_end(dpx_batch *b, unsigned kind, const char **text, size_t *bytes, const uint64_t **offsets);

/* ---- BAXT extension mode: z-drop termination, the query-end score and an end bonus -----------------------------------------
 * What a read mapper's extension step needs beyond DPX_ALGO_BAXT: stop once the score has fallen far enough below its best (ksw2's
 * zdrop, BWA-MEM's Z-dropoff), report the best score that reaches the END OF THE QUERY (ksw2's mqe / mqe_t, BWA's gscore / gtle),
 * and choose between the clipped and the end-to-end alignment with an end bonus (minimap2's end_bonus, BWA's pen_clip).  Modelled on
 * ksw2's extz2, NOT bit-compatible with it: the tie rules and the band definition are this library's.  No reference counterpart.
 * Added without an ABI bump: detect the two functions by the exported symbol.  dpx_align_batch cannot set the values.
 *
 * Cells, band and borders are BAXT's, unchanged.  Two per-batch values: zdrop Z and endBonus E, each -1 = off or >= 0.
 * Let pen = -gapExtend if gapExtend < 0, else 0.
 * Scan: anti-diagonals a = i + j are visited in order a = 1, 2, ..., m + n.  cells(a) = the in-band cells of the matrix on a, border
 * cells included; an empty cells(a) is skipped (every odd a when B = 1; every a past the band's reach).  dmax(a) = the maximum of H
 * on a, (ia, ja) = the cell that holds it with the smallest row.  State best = 0, (bi, bj) = (0, 0).  For each non-empty a:
 *     if dmax(a) > best:  best = dmax(a), (bi, bj) = (ia, ja)
 *     else if Z >= 0 and ia >= bi and ja >= bj and best - dmax(a) > Z + pen * |(ia - bi) - (ja - bj)|:
 *                         stop: lastDiag = a, the pair is z-dropped
 * A pair that is not dropped has lastDiag = m + n.  The COMPUTED cells are the in-band cells with i + j <= lastDiag (the dropping
 * anti-diagonal counts).  All results are taken over the computed cells only:
 *     maxScore, (maxRow, maxCol)  BAXT's rule: the maximum of H and the first cell in row-major order that holds it; 0 at (0, 0)
 *                                 when nothing is above 0.  maxScore == best; the cell may differ from (bi, bj) under ties, so
 *                                 with Z = -1 these three are BAXT's results bit for bit.
 *     qryEndScore, qryEndCol      the maximum of H[m][j] over the computed in-band cells of row m at the smallest such j (j = 0
 *                                 takes part when (m, 0) is in the band; m = 0 makes this row 0).  When row m has no computed
 *                                 in-band cell: DPX_EXT_NO_QUERY_END and -1.
 *     choice                      if E >= 0, the pair is not z-dropped, row m was reached and qryEndScore + E > maxScore (strictly),
 *                                 the pair REACHED THE END: the reported score is qryEndScore WITHOUT the bonus and the end cell is
 *                                 (m, qryEndCol).  Otherwise the reported score and end cell are maxScore / (maxRow, maxCol).
 *                                 E = 0 never flips a pair ("report only").
 * The chosen score and end cell are what dpx_batch_results, dpx_batch_device_results, dpx_batch_traceback, the text pipeline and
 * dpx_batch_cigars_* see; none of them changes otherwise (the walk from a computed cell only visits earlier anti-diagonals).  A
 * reached-end score may be negative; the text block prints it, as BANW's does.
 * dpx_batch_matrix: BAXT's export with every plane 0 where i + j > lastDiag.
 * A Z below -(gapOpen + gapExtend) drops a perfect match: the odd anti-diagonal after a match cell peaks at best + gapOpen +
 * gapExtend.  That is documented, not refused; a mapper's Z (hundreds) is far above it. */
typedef struct dpx_extension {      /* 32 bytes */
    int32_t  maxScore, maxRow, maxCol;
    int32_t  qryEndScore, qryEndCol; /* DPX_EXT_NO_QUERY_END / -1 when row m was not reached */
    int32_t  lastDiag;
    uint32_t flags;                  /* DPX_EXT_ZDROPPED | DPX_EXT_REACHED_END */
    int32_t  reserved;               /* 0 */
} dpx_extension;

#define DPX_EXT_ZDROPPED     0x1u
#define DPX_EXT_REACHED_END  0x2u
#define DPX_EXT_NO_QUERY_END INT32_MIN

/* Legal any time after create; takes effect at the next fill (dpx_batch_fill, dpx_batch_fill_timed).  A batch of another algorithm:
 * DPX_ERR_UNSUPPORTED; a value below -1 or above 1 << 30: DPX_ERR_INVALID.  (-1, -1) returns the batch to plain BAXT (k_baxt_fill).
 * While either value is >= 0 the fill runs k_zext_fill and dpx_batch_describe adds `zdrop=` and `end_bonus=`.  Matrix and
 * DPX_SCORE_ONLY batches, packed2 input, dpx_batch_create_on and a caller's stream as for BAXT.  A DPX_KEEP_BAND_DIRECTIONS batch:
 * DPX_ERR_UNSUPPORTED, the batch is left as it was (this setter keeps refusing: dpx_batch_set_direction_scoring is the way in). */
int dpx_batch_set_extension(dpx_batch *b, int32_t zdrop, int32_t endBonus);
/* numPairs records into host memory.  DPX_ERR_NOT_FILLED before a fill; DPX_ERR_UNSUPPORTED when the last fill ran without
 * extension mode. */
int dpx_batch_extensions(dpx_batch *b, dpx_extension *out);

/* ---- substitution-matrix scoring (BANW and BAXT batches) ----
 * Batches score a column by byte equality (match / mismatch) unless a table is set.  With a table, for a reference byte r and a query
 * byte q the diagonal term uses
 *       s(r, q) = scores[codeOf[r] * alphabet + codeOf[q]]
 * -- the row is the reference code, the column the query code, the matrix need not be symmetric.  Everything else in the BANW / BAXT
 * definitions is unchanged: band, borders, recurrence, tie order, score, end cell, walk rules, export form.  Only H_diag + s uses the
 * table, in the fill and in the walks; params.match / params.mismatch are ignored by both while a table is set.
 * The TEXT stays byte equality: the relation line ('*' / '|') and the CIGAR's '=' / 'X' compare bytes, as SAM defines '='.  So 'a'
 * against 'A' under a case-folding codeOf scores as a match and prints '|' / 'X'.
 * The call applies to every following fill and invalidates lines, text, CIGARs and results of an earlier fill (DPX_ERR_NOT_FILLED until
 * the next one).  scores == NULL clears it (the other arguments are ignored) and the batch runs k_banw_fill / k_baxt_fill again.  Both
 * arrays are copied at the call.  A refused call leaves the previous setting in force.
 *   DPX_ERR_INVALID      b == NULL, alphabet outside 1..32, codeOf == NULL, or a codeOf[x] >= alphabet
 *   DPX_ERR_UNSUPPORTED  an algorithm other than BANW / BAXT; a BANW batch whose band covers its matrices (it runs as ANW); a batch with
 *                        extension mode on (and dpx_batch_set_extension switching a mode on while a table is set: the two go together
 *                        through dpx_batch_set_extension_table below); a batch whose staged sequences leave no room in LDS for the table
 *   DPX_ERR_RANGE        the create-time range check of BANW / BAXT fails for a pair with the largest of the alphabet^2 entries in place
 *                        of match and the smallest in place of mismatch
 * While a table is set dpx_batch_describe reports kernel=k_subst_fill, traceback=k_subst_traceback_wave / k_subst_traceback and adds
 * ` subst=<alphabet>`.  Matrix and DPX_SCORE_ONLY batches, packed2 input, dpx_batch_create_on and a caller's stream as for BAXT.  A
 * DPX_KEEP_BAND_DIRECTIONS batch: DPX_ERR_UNSUPPORTED, the batch is left as it was (this setter keeps refusing:
 * dpx_batch_set_direction_scoring is the way in). */
int dpx_batch_set_substitution(dpx_batch *b, const int8_t *scores, int32_t alphabet, const uint8_t *codeOf /* 256 entries */);

/* ---- BAXT extension mode under a substitution table: both of the above at once ----
 * What ksw2's extz2 takes in one call: (m, mat) with a negative N score together with zdrop and end_bonus.  The two setters above refuse
 * each other's setting (extension mode under a table, a table in extension mode), and keep doing so; this function switches both on
 * together.  A new exported symbol, no ABI bump and no new flag: detect it by the symbol, as the other two.  BAXT only.
 *
 * The definition is the conjunction of the two blocks above, nothing new:
 *     Cells, band, borders    BAXT's under the table: the diagonal term is H[i-1][j-1] + scores[codeOf[r] * alphabet + codeOf[q]] for the
 *                             reference byte r and the query byte q (the row is the reference code; the table need not be symmetric).
 *                             params.match / params.mismatch are ignored.
 *     Scan and results        extension mode's, word for word, over those cells: the scan over anti-diagonals with its update-or-drop
 *                             rule, lastDiag, the computed cells, maxScore / (maxRow, maxCol), qryEndScore / qryEndCol, the end-bonus
 *                             choice and the dpx_extension record.
 *     Text                    byte equality, as under a table.
 * zdrop, endBonus: dpx_batch_set_extension's values; scores, alphabet, codeOf: dpx_batch_set_substitution's (copied at the call).
 *   DPX_ERR_INVALID      b == NULL; scores == NULL or codeOf == NULL; alphabet outside 1..32; a codeOf[x] >= alphabet; zdrop or endBonus
 *                        below -1 or above 1 << 30; both zdrop and endBonus -1 (nothing to combine: dpx_batch_set_substitution does that)
 *   DPX_ERR_UNSUPPORTED  an algorithm other than BAXT; a DPX_KEEP_BAND_DIRECTIONS batch (this setter keeps refusing:
 *                        dpx_batch_set_direction_scoring is the way in); a batch whose staged sequences leave no room in LDS for the table
 *   DPX_ERR_RANGE        dpx_batch_set_substitution's range check fails
 * A refused call leaves both settings of the batch as they were.  Legal in any state; it replaces both settings, applies to every
 * following fill and, as dpx_batch_set_substitution, invalidates lines, text, CIGARs and results of an earlier fill
 * (DPX_ERR_NOT_FILLED until the next one, dpx_batch_extensions included).
 * While both are on: the fill runs k_zsub_fill, the walks are k_subst_traceback_wave / k_subst_traceback from the chosen end cell,
 * dpx_batch_describe reports kernel=k_zsub_fill with ` zdrop=`, ` end_bonus=` and ` subst=`, dpx_batch_extensions returns the records,
 * dpx_batch_matrix is BAXT's export with every plane 0 where i + j > lastDiag, and dpx_batch_results, the text pipeline and
 * dpx_batch_cigars_* see the chosen score and end.  Matrix and DPX_SCORE_ONLY batches, packed2 input, dpx_batch_create_on, a caller's
 * stream, DPX_TIME_FILLS and repeated fills as for BAXT.
 * The two setters keep every behaviour they have, on such a batch too:
 *     dpx_batch_set_extension(b, -1, -1)        switches the mode off and keeps the table: the next fill runs k_subst_fill
 *     dpx_batch_set_substitution(b, NULL, ...)  clears the table and keeps the mode: the next fill runs k_zext_fill
 *     dpx_batch_set_extension with a value >= 0 while a table is set, dpx_batch_set_substitution with a table while the mode is on:
 *                                               DPX_ERR_UNSUPPORTED, as ever
 * To change Z, E or the table of a combined batch, call this function again. */
int dpx_batch_set_extension_table(dpx_batch *b, int32_t zdrop, int32_t endBonus,
                                  const int8_t *scores, int32_t alphabet, const uint8_t *codeOf /* 256 entries */);

/* ---- scoring of a DPX_KEEP_BAND_DIRECTIONS batch: substitution table, z-drop and end bonus ----
 * Band-direction batches are the storage mode of BANW / BAXT that runs long reads (int32 cells, no m + n limit); this function gives
 * them the other half of a mapper's extension step.  The three setters above refuse such a batch with DPX_ERR_UNSUPPORTED and keep
 * doing so; this is ONE setter for all scoring of a band-direction batch.  A new exported symbol, no ABI bump and no new flag: detect
 * it by the symbol.  It accepts a batch only when dpx_batch_describe says kernel=k_bdir_fill (or, after an earlier call, k_bdx_fill).
 *     scores == NULL           no table; alphabet and codeOf are ignored.  Otherwise dpx_batch_set_substitution's arrays, copied at the call.
 *     zdrop, endBonus          dpx_batch_set_extension's values, -1 = off (BAXT only).
 *     everything off           the batch runs plain k_bdir_fill again.
 * The call replaces all three settings at once and applies to every following fill.  If any setting changed it invalidates lines,
 * text, CIGARs and results of an earlier fill as dpx_batch_set_substitution does (DPX_ERR_NOT_FILLED until the next fill,
 * dpx_batch_extensions included).  A refused call changes nothing: dpx_batch_describe is byte-identical before and after.
 * The definitions are the blocks above, word for word, over the same cells: substitution-matrix scoring, BAXT extension mode, and
 * their conjunction.  Nothing about the scan, the record, the end-bonus choice or the text changes.
 *   DPX_ERR_INVALID      b == NULL; zdrop or endBonus below -1 or above 1 << 30; with scores != NULL: alphabet outside 1..32,
 *                        codeOf == NULL, or a codeOf[x] >= alphabet
 *   DPX_ERR_UNSUPPORTED  a batch that is not a band-direction batch (matrix and score-only batches, every other algorithm, a covering
 *                        BANW band that runs as k_affine_dir); zdrop >= 0 or endBonus >= 0 on BANW; one wave's staged strings plus the
 *                        table image exceed one workgroup's LDS
 *   DPX_ERR_RANGE        the create-time range check of a band-direction batch (bounds against 2^28) fails for a pair with the table's
 *                        largest entry in place of match and its smallest in place of mismatch.  With int8 entries and strings that
 *                        fit LDS this can only happen where the creation's own check was already at its limit.
 * While a mode is on: the fill runs k_bdx_fill (dpx_batch_describe: kernel=k_bdx_fill traceback=k_bdir_traceback matrix=banddir4,
 * with ` zdrop=` / ` end_bonus=` / ` subst=` exactly as a matrix batch prints them); with a table, where four waves' strings plus
 * table images do not fit a workgroup the fill runs one-wave workgroups (waves_per_workgroup says what will launch).
 * dpx_batch_extensions returns the records after a fill that ran the scan (zdrop or endBonus on) and DPX_ERR_UNSUPPORTED after one
 * that did not.  dpx_batch_results, dpx_batch_device_results, dpx_batch_traceback, the text pipeline and dpx_batch_cigars_* see the
 * chosen score and end cell.  dpx_batch_directions gives the enum export with every plane 0 where i + j > lastDiag; under a table the
 * H plane's MATCH / MISMATCH stays byte equality.  Repeated fills, DPX_TIME_FILLS, dpx_batch_fill_timed, a caller's stream,
 * dpx_batch_create_on and packed2 input as for a BANW band-direction batch. */
int dpx_batch_set_direction_scoring(dpx_batch *b, int32_t zdrop, int32_t endBonus,
                                    const int8_t *scores, int32_t alphabet, const uint8_t *codeOf /* 256 entries */);

/* ---- Two-piece affine gaps for DPX_KEEP_BAND_DIRECTIONS batches of BANW and BAXT ----
 * Long-read mappers score a gap of length k as the cheaper of two affine pieces: g(k) = max(o1 + k*e1, o2 + k*e2).  Piece 1,
 * (o1, e1) = params.gapOpen / params.gapExtend, prices sequencing errors; piece 2, (o2, e2) with |e2| < |e1|, prices real indels
 * (minimap2's ksw_extd2 / ksw_gg2).  A two-piece batch is created with DPX_KEEP_BAND_DIRECTIONS | DPX_TWO_PIECE_GAPS on BANW or BAXT;
 * until dpx_batch_set_second_gap is called piece 2 equals piece 1 and the batch reports exactly what the unflagged band-direction
 * batch reports.  No ABI bump: detect the feature by the symbol dpx_batch_set_second_gap.
 * Everything not named here is BANW's / BAXT's definition, unchanged: the band |i - j| <= B - 1, the anchoring, the end-cell rules,
 * the admission rule, the tails and the text.
 *   Borders.  H[0][0] = 0; in-band H[i][0] = g(i) and H[0][j] = g(j).  The four gap planes D1, D2, I1, I2 are minus infinity on every
 *     border and outside the band.
 *   Cells.  Dk = max(H_up + ok + ek, Dk_up + ek), Ik = max(H_left + ok + ek, Ik_left + ek); GAP_OPEN wins a tie in each of the four.
 *     best = H_diag + s; then, in this order, D1, D2, I1, I2: a candidate that is >= the winner so far takes the cell.  H is the final
 *     winner; there is no floor.  With (o2, e2) == (o1, e1) the geometry of every choice is the one-piece definition's: insertion holds
 *     iff max(I) >= max(D, diag), otherwise deletion holds iff max(D) >= diag.
 *   Walk.  Five states.  In SCORING the cell's winner names the move and, for a gap, the piece.  In state Dk / Ik the walk emits the gap
 *     column, stays in that state while the cell's own extend bit of that plane is set, and returns to SCORING where that plane opened.
 *     Then ANW's two tails.  The lines, the `_` convention, the relation line and the CIGAR are unchanged; a CIGAR does not say which
 *     piece paid for a gap.
 *   Empty sequences.  The one border line carries g(k), which is convex in k.  BANW's score is g(max(m, n)).  BAXT's first maximum is at
 *     k = 1 when g(1) >= g(L), else at k = L, with L = min(max(m, n), B - 1); it counts only when above 0.
 *   Extension mode on such a batch.  The scan, the record, the drop rule and the end-bonus choice stay word for word; the only change is
 *     pen = max(0, -max(e1, e2)), the flatter piece (what ksw_extd2 passes), which equals the present pen when the pieces are equal.  The
 *     value on anti-diagonal 1 is g(1).
 * The batch stores one BYTE per in-band cell (csrc/dpx_banddir2.h) and runs k_bd2_fill / k_bd2_traceback: dpx_batch_describe reports
 * kernel=k_bd2_fill traceback=k_bd2_traceback matrix=banddir8 and ` gap2=<o2>,<e2>`.  The band limit is B <= 256, covering or not
 * (DPX_ERR_UNSUPPORTED above it: eight cells per lane do not fit the register file); a BANW band that covers the matrix runs the band
 * kernel like any other band, because ANW has no second piece.  The range check is the band-direction batch's, on the componentwise
 * minimum of the two pieces and again on their componentwise maximum.
 * DPX_TWO_PIECE_GAPS without DPX_KEEP_BAND_DIRECTIONS: DPX_ERR_INVALID; with another algorithm than BANW / BAXT: DPX_ERR_UNSUPPORTED.
 * dpx_batch_set_direction_scoring accepts a two-piece batch with its present arguments, checks and semantics; the three older setters
 * keep refusing.  dpx_batch_extensions, the masking of exported planes behind lastDiag, repeated fills, DPX_TIME_FILLS,
 * dpx_batch_fill_timed, a caller's stream, dpx_batch_create_on, packed2 input, the text pipeline and dpx_batch_cigars_* work as for a
 * band-direction batch.
 * dpx_batch_directions on a two-piece batch: DPX_MAT_H is directionMain (either piece exports QUERY_INSERTION / QUERY_DELETION),
 * DPX_MAT_I / DPX_MAT_D are piece 1's planes, DPX_MAT_I2 / DPX_MAT_D2 piece 2's (GAP_OPEN / GAP_EXTEND, the same edge and border
 * conventions), DPX_MAT_H_PIECE is 0 where H took the diagonal or the cell has no code and 1 / 2 for the piece of a gap move.  On any
 * other batch selectors 3..5 answer what an out-of-range `which` answers.
 * dpx_batch_set_second_gap: legal any time after create, applies to every following fill; if a value changed it invalidates the
 * earlier fill's results, lines, text, CIGARs and records (DPX_ERR_NOT_FILLED), as dpx_batch_set_substitution does.
 *   DPX_ERR_INVALID      b == NULL
 *   DPX_ERR_UNSUPPORTED  a batch created without a two-piece flag (DPX_TWO_PIECE_GAPS, or DPX_LOCAL_TWO_PIECE_GAPS below)
 *   DPX_ERR_RANGE        a weight beyond +-2^20, or the range check fails for a pair
 * A refused call changes nothing: dpx_batch_describe is byte-identical before and after.
 * The class surface (dpx_class_main) and dpx_align_batch stay one-piece. */
#define DPX_TWO_PIECE_GAPS 0x20u /* dpx_batch_create flag, only together with DPX_KEEP_BAND_DIRECTIONS */
#define DPX_MAT_I2 3      /* dpx_batch_directions on a two-piece batch: piece 2's horizontal-gap plane */
#define DPX_MAT_D2 4      /* ... piece 2's vertical-gap plane */
#define DPX_MAT_H_PIECE 5 /* ... which piece H's gap move took (0 none, 1, 2) */
int dpx_batch_set_second_gap(dpx_batch *b, int32_t gapOpen2, int32_t gapExtend2);

/* ---- Per-pair orientation for BANW and BAXT batches: leftward extension and right-aligned gaps ----
 * A mapper extends leftward from its first anchor as often as rightward from its last, and on reverse-strand hits it wants the gaps of
 * an ambiguous run at the other end of the run (ksw2's KSW_EZ_RIGHT with KSW_EZ_REV_CIGAR).  Both are the alignment of the reversed
 * strings.  dpx_batch_set_reversed marks pairs of a batch as reversed; the reversing is done on the device, the caller keeps uploading
 * its strings once, left to right, and reads lines, CIGARs and coordinates in its own orientation.  No ABI bump: detect the feature by
 * the symbol dpx_batch_set_reversed.
 *   Definition.  With n / m the pair's reference / query length, a reversed pair is aligned exactly as the pair (reverse(ref),
 *     reverse(qry)) would be by the same batch: cells, band, borders, tie order, end-cell rule, z-drop scan, the table lookup s(r, q) and
 *     the second gap piece are unchanged.  This is the pair's REVERSED FRAME.  A pair that is not reversed reports what it reports in a
 *     batch without a mask, bit for bit.
 *   Reversed frame, unchanged: dpx_batch_results, dpx_batch_device_results, dpx_batch_extensions (every field), dpx_batch_matrix and
 *     dpx_batch_directions (row i / column j are the i-th / j-th character from the RIGHT end of the query / reference).  endRow /
 *     endCol count characters consumed from the right end of the original strings: a BAXT alignment covers ref[n - endCol, n) and
 *     qry[m - endRow, m).
 *   Original orientation: dpx_batch_traceback, the text pipeline (dpx_batch_output_*) and dpx_batch_cigars_*.  The three lines are the
 *     reversed frame's lines read back to front, so they read left to right along the original strings; the ops are in left-to-right
 *     order of the original strings (the reversed frame's ops in reverse order; under DPX_CIGAR_M merging and reversing commute);
 *     refStart = n - refEnd', refEnd = n - refStart', qryStart = m - qryEnd', qryEnd = m - qryStart' with ' the reversed frame's value,
 *     so that the alignment covers ref[refStart, refEnd) and qry[qryStart, qryEnd) of the original strings and a leftward BAXT extension
 *     ends at refEnd = n, qryEnd = m; numOps and the four counters are unchanged.  The header line of a text block (pair number,
 *     score) is unchanged.
 *   `reversed`: numPairs bytes, nonzero = reversed; NULL = no pair.  Legal any time after create, takes effect at the next fill and
 *     invalidates the earlier fill's results, lines, text, CIGARs and records (DPX_ERR_NOT_FILLED) unless there was no mask before and
 *     there is none now.  Calling it again replaces the mask; NULL or all zeros returns the batch to exactly what it reports without
 *     this call.  Admitted on matrix, DPX_SCORE_ONLY, DPX_KEEP_BAND_DIRECTIONS and DPX_TWO_PIECE_GAPS batches, on a BANW batch whose
 *     band covers the matrix, and together with dpx_batch_set_extension, _set_substitution, _set_extension_table,
 *     _set_direction_scoring and _set_second_gap in either call order; packed2 input, dpx_batch_create_on, a caller's stream, repeated
 *     fills, DPX_TIME_FILLS and dpx_batch_fill_timed work as before.
 *   Cost.  One device allocation of the batch's sequence bytes plus the reversed copies (a string that several reversed pairs share is
 *     copied once), one device-to-device copy and one kernel over the copies per call; per fill one pass over the reversed pairs' lines
 *     behind the walk.  No sequence byte crosses the bus again and the host reads none.
 *   dpx_batch_describe gains ` reversed=<count>` behind the plan's fields while count > 0, followed by `rev_addr=0x<hex> rev_bytes=<n>`
 *     (the setter's allocation) and `lines_addr=0x<hex> lines_bytes=<n>` (the traceback line buffer, 0x0 before the first walk):
 *     diagnostics like pool_addr, for tests that overwrite the blocks to show that no result depends on what they held.  With no
 *     reversed pair the text is byte for byte what it was.
 *   DPX_ERR_INVALID      b == NULL
 *   DPX_ERR_UNSUPPORTED  an algorithm other than BANW / BAXT
 *   DPX_ERR_RANGE        the copies would end beyond byte 2^31 of the device sequence buffer, where the pair table's int32 indices do not
 *                        reach (text in dpx_last_error())
 *   DPX_ERR_NOMEM / DPX_ERR_HIP  the allocation or a device call failed
 * A refused or failed call changes nothing: dpx_batch_describe is byte-identical before and after, and the batch fills as before. */
int dpx_batch_set_reversed(dpx_batch *b, const uint8_t *reversed /* numPairs bytes; nonzero = reversed; NULL = none */);

/* ---- substitution-matrix scoring of ANW, ASW and ASG direction batches ----
 * Protein local alignment under a 20-24 letter matrix, DNA with a negative N and folded lower case, transition / transversion weights, a
 * read fitted into a reference window under a 5 x 5 matrix: none of them is a banded problem.  This setter gives the three full-matrix
 * affine algorithms a table in the storage mode that carries it: a DPX_KEEP_DIRECTIONS batch computes in int32 against a 2^28 bound and
 * its walk and export read only the 4-bit codes and the two bytes of a cell.  A new exported symbol, no ABI bump and no new flag: detect
 * it by the symbol.
 *   Definition.  ANW's / ASW's / ASG's block above, word for word, with one change: the diagonal term is
 *         H[i-1][j-1] + scores[codeOf[r] * alphabet + codeOf[q]]
 *     for the reference byte r and the query byte q (the row is the reference code; the table need not be symmetric).  params.match /
 *     params.mismatch are ignored.  Borders, tie order and end-cell rules, ASW's zero floor and "move 0 where H == 0", ASG's first
 *     maximum of row m with its column-0 border, the empty-sequence results and the walk do not change.
 *   Text.  The relation line, the CIGAR's '=' / 'X' and the MATCH / MISMATCH enum of dpx_batch_directions stay byte equality, as under
 *     dpx_batch_set_substitution.
 *   Arguments.  dpx_batch_set_substitution's: both arrays are copied at the call; scores == NULL clears the table (the other arguments
 *     are ignored), is legal on every batch and changes nothing where nothing was set.
 *   Lifecycle.  dpx_batch_set_substitution's: the setting applies to every following fill; a call that changes it invalidates results,
 *     lines, text and CIGARs of an earlier fill (DPX_ERR_NOT_FILLED until the next fill); setting the same table again invalidates
 *     nothing; a refused call leaves the previous setting in force and dpx_batch_describe byte-identical.
 *   DPX_ERR_INVALID      b == NULL; with scores != NULL: alphabet outside 1..32, codeOf == NULL, or a codeOf[x] >= alphabet
 *   DPX_ERR_UNSUPPORTED  anything but a DPX_ALGO_ANW / DPX_ALGO_ASW / DPX_ALGO_ASG batch created with DPX_KEEP_DIRECTIONS: their matrix
 *                        and DPX_SCORE_ONLY batches, LNW / LSW direction batches, every banded algorithm in every storage mode (a BANW
 *                        band-direction batch whose covering band runs k_affine_dir and a BSW / BASW local band-direction batch whose
 *                        covering band runs k_linear_dir / k_asw_dir included)
 *   DPX_ERR_RANGE        the create-time range check of a direction batch (bounds against 2^28) fails for a pair with the table's largest
 *                        entry in place of match and its smallest in place of mismatch
 * While a table is set dpx_batch_describe keeps kernel=k_affine_dir / k_asw_dir / k_asg_dir and matrix=dir4 (the table is a mode of the
 * same fill, k_dirtab_fill in the library) and adds ` subst=<alphabet>`.  Every wave keeps the 1280-byte table image in LDS; where the
 * plan's waves per workgroup no longer fit with it the fill runs one-wave workgroups (waves_per_workgroup says what will launch), and
 * a one-wave workgroup always fits, so there is no "no room in LDS" refusal.  dpx_batch_set_extension, dpx_batch_set_substitution (with
 * a table), dpx_batch_set_extension_table and dpx_batch_set_direction_scoring keep refusing these batches.  Repeated fills,
 * DPX_TIME_FILLS, dpx_batch_fill_timed, a caller's stream, dpx_batch_create_on and packed2 input as for any direction batch. */
int dpx_batch_set_direction_table(dpx_batch *b, const int8_t *scores, int32_t alphabet, const uint8_t *codeOf /* 256 entries */);

/* ---- substitution-matrix scoring of ANW, ASW and ASG score-only batches ----
 * A database search -- one query scored against many sequences under BLOSUM62 -- or a read scored against many candidate windows under a
 * 5 x 5 matrix with a negative N needs scores and end cells, no traceback: score everything, keep the hits, realign those on a direction
 * batch (dpx_batch_set_direction_table).  This setter gives DPX_SCORE_ONLY batches of the three full-matrix affine algorithms a table: no
 * pool, no stores, the kernels of any score-only batch with one term changed.  A new exported symbol, no ABI bump and no new flag:
 * detect it by the symbol.
 *   Definition.  ANW's / ASW's / ASG's block above, word for word, with one change: the diagonal term is
 *         H[i-1][j-1] + scores[codeOf[r] * alphabet + codeOf[q]]
 *     for the reference byte r and the query byte q (the row is the reference code; the table need not be symmetric).  params.match /
 *     params.mismatch are ignored.  Borders, tie order, ASW's zero floor and first strict maximum in row-major order, ASG's first
 *     maximum of row m with column 0 winning a tie, and the empty-sequence results do not change.
 *   Arguments.  dpx_batch_set_substitution's: both arrays are copied at the call; scores == NULL clears the table (the other arguments
 *     are ignored), is legal on every batch and changes nothing where nothing was set.  Where a table was set through another setter
 *     (dpx_batch_set_substitution on a BANW batch, say) the NULL call clears that one, as dpx_batch_set_direction_table's NULL call
 *     does: a batch holds one table, and NULL through any of the three clears it.
 *   Lifecycle.  dpx_batch_set_substitution's: the setting applies to every following fill; a call that changes it invalidates the
 *     results of an earlier fill (DPX_ERR_NOT_FILLED until the next fill); setting the same table again invalidates nothing; a refused
 *     or failed call leaves the previous setting in force, dpx_batch_describe byte-identical and the batch filling as before.
 *   DPX_ERR_INVALID      b == NULL; with scores != NULL: alphabet outside 1..32, codeOf == NULL, or a codeOf[x] >= alphabet
 *   DPX_ERR_UNSUPPORTED  anything but a DPX_ALGO_ANW / DPX_ALGO_ASW / DPX_ALGO_ASG batch (the batch's own algorithm) created with
 *                        DPX_SCORE_ONLY: their matrix batches (a traceback under a table is the direction batch's, at a twelfth of the
 *                        bytes), their direction batches (which keep their own setter), LNW / LSW, every banded algorithm in every
 *                        storage mode (a covering BANW / BASW band that runs the ANW / ASW kernels included); and a batch where one
 *                        wave's LDS slice plus the table image does not fit a workgroup (dpx_last_error() says which; today creation
 *                        admits a batch only when FOUR plain slices fit one workgroup, so no batch that exists reaches this refusal)
 *   DPX_ERR_RANGE        the create-time range check of an int16 batch (fits_int16) fails for a pair with the table's largest entry in
 *                        place of match and its smallest in place of mismatch.  Score-only batches stay on the int16 bound because
 *                        these kernels keep their stripe edge rows as int16 in LDS and their ASW / ASG running maxima as 16-bit
 *                        (score, column) keys; the bounds carry over by the argument given for dpx_batch_set_substitution (a diagonal
 *                        step scores at least the smallest entry and at most the largest).  Longer pairs belong on a direction batch.
 * While a table is set dpx_batch_describe keeps kernel= (k_affine_fill, k_asw_lanes, ...: the table is a mode of the same fills,
 * k_scoretab_fill / k_scoretab_lanes in the library) and store=0, and adds ` subst=<alphabet>`.  Every wave keeps the 1280-byte table
 * image in LDS; where the plan's waves per workgroup no longer fit with it the one-wave-per-pair fill runs one-wave workgroups
 * (waves_per_workgroup says what will launch; the lane-packed kernels are one-wave workgroups already).  dpx_batch_set_extension,
 * dpx_batch_set_substitution (with a table), dpx_batch_set_extension_table, dpx_batch_set_direction_scoring and
 * dpx_batch_set_direction_table keep refusing these batches; matrix requests stay DPX_ERR_NO_MATRIX.  Repeated fills, DPX_TIME_FILLS,
 * dpx_batch_fill_timed, a caller's stream, dpx_batch_create_on, packed2 input and pairs that share bytes as for any score-only batch. */
int dpx_batch_set_score_table(dpx_batch *b, const int8_t *scores, int32_t alphabet, const uint8_t *codeOf /* 256 entries */);

/* ---- substitution-matrix scoring of BSW and BASW local band-direction batches ----
 * A DPX_KEEP_LOCAL_BAND_DIRECTIONS batch is the only local alignment that runs past ~10-16 kb: a long noisy read aligned locally against
 * a window, where N must not match N and soft-masked lower case must fold; transition / transversion weights; a banded local protein
 * alignment under a 20-24 letter matrix that realigns the hits a score-only table batch found.  This setter gives those batches a table.
 * A new exported symbol, no ABI bump and no new flag: detect it by the symbol.
 *   Definition.  BSW's / BASW's block above as a DPX_KEEP_LOCAL_BAND_DIRECTIONS batch computes it, word for word, with one change: the
 *     diagonal term of every in-band cell is
 *         H[i-1][j-1] + scores[codeOf[r] * alphabet + codeOf[q]]
 *     for the reference byte r and the query byte q (the row is the reference code; the table need not be symmetric).  params.match /
 *     params.mismatch are ignored.  The zero floor, the H = 0 read from every neighbour without a cell, the tie orders, the codes, the
 *     end-cell rule (first maximum in row-major order, (0, 0) when every H is 0) and the walk that stops where H == 0 do not change.
 *   Text.  The relation line, the CIGAR's '=' / 'X', MD / cs and the MATCH / MISMATCH enum of dpx_batch_directions stay byte equality,
 *     as under dpx_batch_set_substitution.
 *   Arguments.  dpx_batch_set_substitution's: entries are int8, 1 <= alphabet <= 32, codeOf has 256 entries, each < alphabet; both arrays
 *     are copied at the call; scores == NULL clears the table (the other arguments are ignored), is legal on every batch and changes
 *     nothing where nothing was set.  A batch holds one table, and NULL through any table setter clears it.
 *   Lifecycle.  dpx_batch_set_substitution's: the setting applies to every following fill; a call that changes it invalidates results,
 *     lines, text, CIGARs and difference strings of an earlier fill (DPX_ERR_NOT_FILLED until the next fill);
 *     setting the same table again invalidates nothing; a refused call leaves the previous setting in force and dpx_batch_describe
 *     byte-identical.
 *   Statuses, in this order, every check before the first change:
 *   DPX_ERR_INVALID      b == NULL; with scores != NULL: alphabet outside 1..32, codeOf == NULL, or a codeOf[x] >= alphabet
 *   DPX_ERR_UNSUPPORTED  anything but a DPX_ALGO_BSW / DPX_ALGO_BASW batch created with DPX_KEEP_LOCAL_BAND_DIRECTIONS whose band does not
 *                        cover the matrix: matrix and DPX_SCORE_ONLY batches, every other algorithm, BANW / BAXT band-direction batches
 *                        (dpx_batch_set_direction_scoring is theirs), and a covering BSW / BASW band, which runs k_linear_dir / k_asw_dir
 *   DPX_ERR_UNSUPPORTED  one wave's staged strings leave no room in LDS for the 1280-byte table image
 *   DPX_ERR_RANGE        the create-time range check of the batch (LSW's / ASW's bounds against 2^28) fails for a pair with the table's
 *                        largest entry in place of match and its smallest in place of mismatch
 * While a table is set dpx_batch_describe says kernel=k_bdlt_fill, keeps traceback=k_bdl_traceback and matrix=banddir4 and adds
 * ` subst=<alphabet>` between them.  Every wave keeps the table image in LDS behind its staged strings; where four waves' strings and
 * images no longer fit a workgroup the fill runs one-wave workgroups (waves_per_workgroup says what will launch).  The seven other
 * setters (dpx_batch_set_extension, dpx_batch_set_substitution with a table, dpx_batch_set_extension_table, dpx_batch_set_second_gap,
 * dpx_batch_set_direction_scoring, dpx_batch_set_direction_table, dpx_batch_set_score_table with a table; dpx_batch_set_reversed too)
 * keep refusing these batches, table set or not (dpx_batch_set_second_gap admits the DPX_LOCAL_TWO_PIECE_GAPS batches of BASW, below).
 * Not built: covering bands, reversed pairs and extension settings on local batches, a table through dpx_align_batch.  Repeated fills, DPX_TIME_FILLS, dpx_batch_fill_timed, a caller's stream,
 * dpx_batch_create_on, packed2 input, the output pipeline, dpx_batch_cigars_* and dpx_batch_diffs_* as for any local band-direction batch. */
int dpx_batch_set_local_direction_table(dpx_batch *b, const int8_t *scores, int32_t alphabet, const uint8_t *codeOf /* 256 entries */);

/* ---- A second gap piece for BASW local band-direction batches ----
 * The pairs that need a DPX_KEEP_LOCAL_BAND_DIRECTIONS batch are long noisy reads against a window, and every long-read scoring scheme
 * prices them with two gap pieces: a gap of length k scores max(o1 + k*e1, o2 + k*e2), so a 100-base deletion does not cost a hundred
 * sequencing errors.  New create flag DPX_LOCAL_TWO_PIECE_GAPS, legal only together with DPX_KEEP_LOCAL_BAND_DIRECTIONS, on
 * DPX_ALGO_BASW (BSW has one linear gap weight and no second piece).  Piece 1 is params.gapOpen / gapExtend.  Piece 2 starts equal to
 * piece 1 and is set with dpx_batch_set_second_gap(b, o2, e2), whose rule "a batch created without DPX_TWO_PIECE_GAPS ->
 * DPX_ERR_UNSUPPORTED" reads "without a two-piece flag".  There is no new symbol and no ABI bump.
 * Everything not named below is BASW's definition under DPX_KEEP_LOCAL_BAND_DIRECTIONS, unchanged: the band |i - j| <= B - 1 over cells
 * with i, j >= 1, the end-cell rule, the text block, and "no tails".
 *   Neighbours.  A neighbour that is a border cell, lies outside the band or lies outside the matrix reads H = 0 and D1 = D2 = I1 = I2 =
 *     minus infinity: BASW's rule with four gap planes.
 *   Cells.  Dk = max(H_up + ok + ek, Dk_up + ek) and Ik = max(H_left + ok + ek, Ik_left + ek); GAP_OPEN wins a tie in each of the four.
 *     best = H_diag + s; then, in this order, D1, D2, I1, I2: a candidate that is >= the winner so far takes the cell (k_bd2_fill's
 *     order).  H = max(0, winner); the move is NONE where H == 0.  With (o2, e2) == (o1, e1), every score, end cell, line, CIGAR and the
 *     H / I / D planes equal the one-piece local batch's; piece 2's planes equal piece 1's.
 *   Score / end cell.  BASW's rule: the first maximum in row-major order, or 0 at (0, 0) when every H is 0.  Empty sequences give 0 at
 *     (0, 0).
 *   Walk.  Five states, from the end cell in SCORING.  In SCORING the walk stops on the first cell whose H is 0: move 0, or a cell
 *     without a code (a border cell or a cell outside the band).  In state Dk / Ik the walk emits the gap column, stays in that state
 *     while the cell's own extend bit of that plane is set, and returns to SCORING where that plane opened.  An edge cell always opens,
 *     so the walk cannot extend out of the band.  The lines, the `_` convention, the relation line, the CIGAR, MD / cs and the
 *     dpx_alignment records are as for the one-piece batch; a CIGAR does not say which piece paid.
 *   dpx_batch_directions takes the six selectors of a two-piece batch.  DPX_MAT_H is NONE_MAIN where H == 0; either piece exports
 *     QUERY_INSERTION / QUERY_DELETION.  DPX_MAT_I / _D / _I2 / _D2 are GAP_OPEN / GAP_EXTEND for every in-band cell.  DPX_MAT_H_PIECE is
 *     0 / 1 / 2.  Every plane is 0 on the borders and outside the band (the local export's rule).
 *   Storage.  One byte per in-band cell in csrc/dpx_banddir2.h's layout, unchanged.  dpx_batch_describe shows kernel=k_lb2_fill
 *     traceback=k_lb2_traceback matrix=banddir8 gap2=<o2>,<e2>.
 *   Band.  B <= 256, covering or not; 257 and above is DPX_ERR_UNSUPPORTED.  A covering band runs the band kernel, because ASW has no
 *     second piece (as for DPX_TWO_PIECE_GAPS).
 *   Range.  The local batch's check (ASW's bounds against 2^28, no m + n limit) on the componentwise minimum of the two pieces and again
 *     on their maximum; under a table, with the table's extremes.
 *   Flags.  DPX_LOCAL_TWO_PIECE_GAPS without DPX_KEEP_LOCAL_BAND_DIRECTIONS: DPX_ERR_INVALID; with DPX_SCORE_ONLY,
 *     DPX_KEEP_BAND_DIRECTIONS or DPX_TWO_PIECE_GAPS: DPX_ERR_INVALID; on any algorithm but BASW: DPX_ERR_UNSUPPORTED, BSW included; with
 *     DPX_KEEP_DIRECTIONS: DPX_ERR_UNSUPPORTED.
 *   Setters.  dpx_batch_set_second_gap has its present argument checks and invalidates the earlier fill only when a value changed.
 *     dpx_batch_set_local_direction_table is admitted, with its lifecycle, its LDS-fit refusal and its one-wave workgroups where four
 *     waves' strings plus images pass 160 KiB; describe then adds ` subst=<alphabet>` and keeps kernel=k_lb2_fill.  Every other setter
 *     refuses as on a one-piece local batch (extension, substitution, extension_table, direction_scoring, direction_table, score_table,
 *     reversed).  A refused call leaves dpx_batch_describe byte-identical.
 *   Detecting it.  An older library ignores the bit and builds the one-piece batch: describe then says kernel=k_bdl_fill
 *     matrix=banddir4, and dpx_batch_set_second_gap returns DPX_ERR_UNSUPPORTED.
 * Not built: bands 257..512 under two pieces, z-drop / end bonus and reversed pairs on local batches, the class surface and
 * dpx_align_batch, BSW. */
#define DPX_LOCAL_TWO_PIECE_GAPS 0x80u /* dpx_batch_create flag, only together with DPX_KEEP_LOCAL_BAND_DIRECTIONS, on DPX_ALGO_BASW */

/* Sizes: numPairs, total cells (sum refLen*queryLen, the reference's numCells, c++/parseInput.cpp:100),
 * bytes of HBM the matrices occupy, algorithmic bytes of one fill. */
int dpx_batch_info(dpx_batch *b, size_t *numPairs, uint64_t *cells, uint64_t *matrixBytes, uint64_t *algorithmicBytes);

/* One line of text about how the batch will be (was) filled: `algo=LSW kernel_algo=LSW kernel=k_linear_fill_pk dtype=int16
 * rows_per_lane=16 store=1 couples=5000 lane_pairs=0 waves=0 singles=0 streams=0 row_tags=1 pool=vmm pool_bytes=22263365632
 * pool_chunk_mb=1024 pool_kept=0 pool_memset_ms=3.290` (pool_*: how the matrix pool was allocated -- `vmm` = a virtual range
 * backed by physical chunks, `malloc` = one hipMalloc -- and the hipMemset time of every candidate allocation that was timed,
 * `untimed` if none was; pool_kept indexes the one in use).  `pool_addr=0x<hex>` follows pool_bytes: the device address of
 * the block of pool_bytes bytes that holds the batch's matrices (a diagnostic: tests overwrite exactly that range between
 * fills to show that no result depends on what it held); a batch without a pool (DPX_SCORE_ONLY) reports only
 * `pool_addr=0x0`.  The longest line (a tuned pool's five candidates) stays below 1 KiB.  The reference prints its launch
 * geometry the same way (cuda/LNW/LinearNeedlemanWunschV19.cu:398-409); tests and bench.py read the kernel and the
 * arithmetic type from here instead of guessing the host's choice. */
int dpx_batch_describe(dpx_batch *b, char *buf, size_t cap);

int dpx_batch_destroy(dpx_batch *b);

/* ---- one-shot path (what the SequenceAligner-derived classes call from score_matrix()) ------------- */

/* create + fill + results [+ matrices of pair 0..numPairs-1 into caller buffers] + destroy.
 * H/I/D may be NULL; otherwise they are arrays of numPairs host pointers, each (m+1)*(n+1) int16. */
int dpx_align_batch(const dpx_params *params, const char *sequences, size_t numBytes, const dpx_seq_pair *pairs,
                    size_t numPairs, int32_t *scores, int32_t *endRow, int32_t *endCol, int16_t **H, int16_t **I,
                    int16_t **D);

/* ---- DPX primitive probe (a5: FakeDPX, c++/FakeDPX.hpp:19-126) ----------------------------------- */

/* Evaluate `count` DPX primitives on the device with the CDNA4 instruction mapping used by the kernels
 * (v_max3_i32 / v_pk_max_i16 / v_pk_add_i16 ...).  op numbering follows c++/FakeDPX.hpp declaration order
 * (0 = __vimax3_s32 ... 35 = __viaddmin_s16x2_relu).  pred bit0 = pred / pred_lo, bit1 = pred_hi. */
int dpx_prim_eval(const int32_t *op, const uint32_t *a, const uint32_t *b, const uint32_t *c, size_t count,
                  uint32_t *result, uint32_t *pred);

#ifdef __cplusplus
}
#endif
#endif /* DPX_ALIGN_H */
