/* dpx_plan.h -- the host-only half of dpx_batch_create: what a batch decides before it touches the device, as a pure function of the
 * parameters, the pairs' sizes and indices, the flags and a Knobs snapshot.  No sequence byte is read and no HIP function called
 * (dpx_kernels.h: the argument structs only), so hostcpp/plan_tool runs it without a GPU.  dpx_capi.cpp, dpx_settings.cpp and
 * dpx_output.cpp do the device work. */
#ifndef DPX_PLAN_H
#define DPX_PLAN_H

#include <string>
#include <vector>

#include "../../include/dpx_align.h"
#include "dpx_dir.h" /* (first: it brings dpx_kernels.h, whose hip_runtime.h the layout headers need under hipcc) */
#include "dpx_banddir.h"
#include "dpx_banddir2.h"

#pragma GCC visibility push(hidden) /* (internal to libdpxalign.so: not part of its ABI) */

/* Development and test knobs.  The environment is read in ONE place (dpx_host.cpp: refresh_knobs), when dpx_init() binds a device and
 * again at the start of every dpx_batch_create*() (the tests flip a knob between two batches of one process); everything else reads this
 * snapshot.  -1 / 0 = not set.  None of them changes a result: they force or forbid a kernel family, change the launch shape or trace
 * the runtime. */
struct Knobs {
    int rowsPerLane = 0;   /* DPX_R=2|4|8|16 */
    int packed = -1;       /* DPX_PACKED=0|1: the two-pairs-per-wave int16 kernels */
    int lanes = -1;        /* DPX_LANES=0|1: the lane-packed (several pairs per wave) kernels */
    int lanesPk = -1;      /* DPX_LANES_PK=0: keep the lane-packed batches on the int32 kernels */
    int split = -1;        /* DPX_SPLIT=0|1: one wave per stripe */
    int rowTags = -1;      /* DPX_ROW_TAGS=0: per-row start-cell keys in the packed SW kernel */
    int rampLines = -1;    /* DPX_RAMP_LINES=0|1: skew ramps store lines / whole chunks */
    int wavesPerBlock = 0; /* DPX_WPB=1|4 */
    int group = 0;         /* DPX_GROUP: pairs per interleaved block of the matrix layout */
    int tbWalk = -1;       /* DPX_TB_WALK=0|1|2 */
    int poolProbe = -1;    /* DPX_POOL_PROBE=0|1|2: nothing / time the pool / time + shop, whatever DPX_TUNE_PLACEMENT says */
    bool poolMalloc = false;  /* DPX_POOL=malloc: one hipMalloc instead of the chunked virtual range */
    size_t poolChunkBytes = 0; /* DPX_POOL_CHUNK_MB */
    int poolGuard = 0;     /* DPX_POOL_GUARD: 1 = pattern band behind the matrices, 2 = "selftest" (the band is born damaged) */
    bool trace = false, traceVmm = false; /* DPX_TRACE / DPX_TRACE_VMM: phase timings / pool mapping calls on stderr */
};

/* What dpx_plan_batch decides.  dpx_batch (dpx_batch.h) takes it over by move and fills in the device pointers. */
struct dpx_plan {
    dpx_params prm{}; unsigned flags = 0; size_t numPairs = 0;
    bool packed2 = false;  /* the sequences arrive as 2-bit codes (dpx_batch_create_packed2) */
    int kernelAlgo = 0;    /* algorithm the kernel runs (BSW with a covering band runs as LSW) */
    int R = 8;             /* rows per lane (full-matrix kernels) or cells per lane (band kernels) */
    int planes = 1;
    bool store = true;
    bool dirs = false;     /* DPX_KEEP_DIRECTIONS: 4-bit codes in the pool (matElems counts them in int16 units, dpx_dir.h), k_linear_dir / k_affine_dir */
    bool bandDirs = false; /* DPX_KEEP_BAND_DIRECTIONS on a BANW / BAXT band kernel: codes in dpx_banddir.h's layout, k_bdir_fill through `args`
                              (a covering BANW band is a `dirs` batch of ANW instead) */
    bool bandLocal = false; /* DPX_KEEP_LOCAL_BAND_DIRECTIONS on a BSW / BASW band kernel: a bandDirs plan in the same layout whose kernels are k_bdl_fill,
                              k_bdl_traceback and k_bdl_export (a covering band is a `dirs` batch of LSW / ASW instead); under a table
                              (dpx_batch_set_local_direction_table) the fill is k_bdlt_fill, walk and export stay */
    bool twoPiece = false; /* ... with DPX_TWO_PIECE_GAPS: 8-bit codes in dpx_banddir2.h's layout, k_bd2_fill; every band <= 256 runs the band kernel.
                              On a bandLocal plan (DPX_LOCAL_TWO_PIECE_GAPS, BASW): the same codes and layout, k_lb2_fill / k_lb2_traceback / k_lb2_export */
    bool bandScores = false; /* DPX_LONG_SCORES on a bandDirs (0x10) or bandLocal (0x40) plan: that plan's geometry -- C, parity, ldsPerWave, ldsRefOff, waves
                              per workgroup, the range check against 2^28 -- with store = false: no pool, no line offsets, k_bscore_fill / k_lscore_fill.
                              Every band <= 512 runs the band kernel, covering or not */
    int32_t gapOpen2 = 0, gapExtend2 = 0; /* twoPiece: the second gap piece (dpx_batch_set_second_gap; piece 1 until then) */
    bool packed = false;     /* LNW / LSW / BSW with matrices: couples of equal-shaped pairs, two per wave + leftover singles */
    bool split = false;      /* small batch: one workgroup per pair, one wave per stripe (k_linear_split) */
    bool lanePacked = false; /* short queries: several pairs per wave (k_linear_lanes / k_affine_lanes, 8 x 8 tile layout) */
    bool lanesPk = false;    /* lane-packed batch on k_linear_lanes_pk (two row blocks of a pair in the halves of every register) */
    int splitWaves = 0, maxM = 0, maxN = 0;
    size_t splitLds = 0;
    uint64_t cells = 0, matElems = 0, algBytes = 0, bandCells = 0;
    std::vector<dpx_pair_dev> pairs; /* the device pair table, indices relative to seqLo */
    std::vector<int32_t> singles;     /* launch order of the one-wave-per-pair kernel (longest first); empty: pair order */
    std::vector<int32_t> couples;     /* packed kernels: two adjacent entries per wave */
    std::vector<dpx_wave_desc> waves; /* lane-packed kernels: one descriptor per wave */
    std::vector<uint64_t> tbOff;      /* where k_traceback puts a pair's three lines (numPairs + 1 entries; empty when score-only) */
    size_t seqLo = 0, seqHi = 0;      /* the bytes (bases) of the caller's buffer that the pairs touch: only these are uploaded */
    size_t packedDwords = 0, packedCopy = 0; /* 2-bit input: dwords k_unpack2 expands, bytes of the caller's packed buffer to copy */
    size_t dirScratch = 0; /* direction batches whose edge rows do not fit LDS: bytes of the per-wave areas behind the codes (0: LDS) */
    dpx_fill_args args{};   /* the one-wave-per-pair / split kernel; every pointer null */
    dpx_fill_args pkArgs{}; /* the packed or lane-packed kernel; every pointer null */
    dpx_dir_args dirArgs{}; /* the direction kernels; every pointer null */
    size_t ldsBytes = 0, pkLdsBytes = 0;
    size_t nSingles = 0, nCouples = 0, nLanePairs = 0, nWaves = 0; /* launch-list sizes (dpx_batch_describe) */
};

bool is_affine(int algo), is_banded(int algo), is_banded_affine(int algo), is_banw_layout(int algo);
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
int validate_params(const dpx_params *p);
bool fits_int16(const dpx_params &p, long long m, long long n), fits_dir(const dpx_params &p, long long m, long long n);
bool packed_safe(const dpx_params &p, long long m, long long n);

/* The status dpx_batch_create*() returns for this input once validate_params, the flag checks and the device have passed, and on DPX_OK the
 * plan.  `numBytes`: bytes (2-bit input: bases) of the caller's buffer.  `err` receives the text for dpx_last_error(). */
int dpx_plan_batch(const dpx_params &params, const dpx_seq_pair *pairs, size_t firstPair, size_t numPairs, size_t numBytes, bool packed2Input,
                   unsigned flags, const Knobs &knobs, dpx_plan &out, std::string &err);

/* Which kernels a batch runs: the one place that decides it.  A fill, a traceback, a matrix export and dpx_batch_describe() each compute
 * the route again and read their part of it (plain data, no allocation; nothing is cached, so a setter has nothing to invalidate). */
enum dpx_fill_kernel { /* the kernel that fills (most of) the batch: describe's kernel= */
    DPX_K_LINEAR_FILL, DPX_K_LINEAR_FILL_PK, DPX_K_LINEAR_LANES, DPX_K_LINEAR_LANES_PK, DPX_K_LINEAR_SPLIT,
    DPX_K_AFFINE_FILL, DPX_K_ASW_FILL, DPX_K_ASG_FILL, DPX_K_AFFINE_LANES, DPX_K_ASW_LANES, DPX_K_ASG_LANES,
    DPX_K_BANDED_FILL, DPX_K_BANDED_FILL_PK, DPX_K_BASW_FILL, DPX_K_BANW_FILL, DPX_K_BAXT_FILL,
    DPX_K_ZEXT_FILL, DPX_K_SUBST_FILL, DPX_K_ZSUB_FILL, DPX_K_BDIR_FILL, DPX_K_BDX_FILL, DPX_K_BD2_FILL,
    DPX_K_LINEAR_DIR, DPX_K_AFFINE_DIR, DPX_K_ASW_DIR, DPX_K_ASG_DIR, DPX_K_BDL_FILL, DPX_K_BDLT_FILL, DPX_K_COUNT
};
enum dpx_main_launch { DPX_MAIN_NONE, DPX_MAIN_FILL, DPX_MAIN_BASW, DPX_MAIN_BANW, DPX_MAIN_BAXT, DPX_MAIN_ZEXT, DPX_MAIN_SUBST, DPX_MAIN_ZSUB, DPX_MAIN_BDIR, DPX_MAIN_BDX, DPX_MAIN_BD2, DPX_MAIN_BDL, DPX_MAIN_BDLT };
/* The two-piece local band-direction batches (DPX_LOCAL_TWO_PIECE_GAPS, dpx_lb2_kernels.hip).  Values of the two enums above, declared
 * behind them: tests/test_bdlt_constants.py holds both enumerator lists to the last name they had, and DPX_K_COUNT stays the size of
 * dpx_route_kernel_name's table of create-time kernels.  Both values lie inside the enums' ranges (5 and 4 bits). */
constexpr dpx_fill_kernel DPX_K_LB2_FILL = static_cast<dpx_fill_kernel>(DPX_K_COUNT + 1);
constexpr dpx_main_launch DPX_MAIN_LB2 = static_cast<dpx_main_launch>(DPX_MAIN_BDLT + 1);
/* DPX_LONG_SCORES (dpx_bscore_kernels.hip, dpx_lscore_kernels.hip): appended the same way, behind the values above (31 and 15: still
 * inside the ranges) */
constexpr dpx_fill_kernel DPX_K_BSCORE_FILL = static_cast<dpx_fill_kernel>(DPX_K_COUNT + 2);
constexpr dpx_fill_kernel DPX_K_LSCORE_FILL = static_cast<dpx_fill_kernel>(DPX_K_COUNT + 3);
constexpr dpx_main_launch DPX_MAIN_BSCORE = static_cast<dpx_main_launch>(DPX_MAIN_BDLT + 2);
constexpr dpx_main_launch DPX_MAIN_LSCORE = static_cast<dpx_main_launch>(DPX_MAIN_BDLT + 3);
enum dpx_second_launch { DPX_SECOND_NONE, DPX_SECOND_PACKED, DPX_SECOND_BANDED_PACKED, DPX_SECOND_LANES, DPX_SECOND_LANES_PK };
enum dpx_walk_family { DPX_WALK_PLAIN, DPX_WALK_DIR, DPX_WALK_BASW, DPX_WALK_BANW, DPX_WALK_SUBST, DPX_WALK_BDIR, DPX_WALK_BD2, DPX_WALK_BDL, DPX_WALK_LB2 };
enum dpx_export_kind { DPX_EXPORT_PLAIN, DPX_EXPORT_BASW, DPX_EXPORT_BANW };
struct dpx_route {
    dpx_fill_kernel kernel;
    /* the launches of one fill: a direction batch, or the split kernel, or the secondary kernel (if any) beside the one-wave-per-pair
     * kernel of the pairs it leaves over (if any) */
    bool dirs, split;
    bool dirTable;   /* ... a direction batch of ANW / ASW / ASG under a table (dpx_batch_set_direction_table): k_dirtab_fill, a mode of the same three kernel= names */
    bool scoreTable; /* ... a DPX_SCORE_ONLY batch of ANW / ASW / ASG under a table (dpx_batch_set_score_table): main and second are the plain batch's, each launched
                        through its table twin (k_scoretab_fill / k_scoretab_lanes); a mode of the same six kernel= names */
    dpx_second_launch second;
    dpx_main_launch main;
    bool ext;        /* the band kernel (BDIR, SUBST) runs BAXT's end-cell rule, not BANW's */
    bool extRecords; /* the fill writes a dpx_extension record per pair (k_zext_fill, k_zsub_fill, k_bdx_fill with its scan on) */
    dpx_walk_family walk;
    int walkMode;    /* 0 / 1: one lane per pair, cell by cell / through cached column vectors; 2: one wave per pair (DIR, BDIR, BD2 and BDL have one walk: 0) */
    dpx_export_kind exportKind;
};
/* What a batch can change after its creation comes as arguments: the traceback walk knob, BAXT's extension mode (-1, -1: off) and the
 * substitution alphabet (0: none).  On a bandDirs plan either of the two (dpx_batch_set_direction_scoring) turns k_bdir_fill into
 * k_bdx_fill; the walk stays k_bdir_traceback.  On a bandLocal plan the alphabet (dpx_batch_set_local_direction_table) turns k_bdl_fill
 * into k_bdlt_fill; the walk stays k_bdl_traceback.  On a dirs plan of ANW / ASW / ASG the alphabet
 * (dpx_batch_set_direction_table) sets dirTable and nothing else; on a score-only plan of the three (dpx_batch_set_score_table) it sets
 * scoreTable and nothing else.  A twoPiece plan runs k_bd2_fill and k_bd2_traceback in every mode (bandLocal as well: k_lb2_fill and
 * k_lb2_traceback, with or without the alphabet); its second piece is
 * the plan's own (the batch IS the plan), so the signatures here do not know it.  A bandScores plan (DPX_LONG_SCORES) runs k_bscore_fill
 * (0x10) or k_lscore_fill (0x40) in every mode its setters bring; it has no walk and no export. */
dpx_route dpx_plan_route(const dpx_plan &p, int tbWalk, int zdrop, int endBonus, int substAlphabet);
/* Waves per workgroup of a bandDirs plan's fill: the plan's own without a table; with one (DPX_SUBST_IMAGE_BYTES more per wave) the
 * plan's own when four waves' strings and images fit one workgroup's LDS, else 1, and 0 when not even one wave's fit (the setter
 * refuses).  The plan's own is 1 or 4 (fill_waves_per_block: DPX_WPB takes no other value), so "four do not fit" and "the plan's own do
 * not fit" are the same test wherever it matters.  A pure function of the plan, which is not changed. */
unsigned dpx_plan_bdx_waves(const dpx_plan &p, bool table);
/* Waves per workgroup of a dirs plan's fill under a table (dpx_batch_set_direction_table): the plan's own when that many waves' edge
 * rows, staged references and images fit one workgroup's LDS, else 1.  One wave always fits (edge rows in LDS: dirArgs.ldsPerWave <= 64
 * KiB; edge rows in the scratch: the image alone, and the plan's own is 1), so this setter has no "no room in LDS" refusal.  A pure
 * function of the plan, which is not changed. */
unsigned dpx_plan_dirtab_waves(const dpx_plan &p);
/* A score-only plan of ANW / ASW / ASG under a table (dpx_batch_set_score_table).  _lds: one wave's slice of the one-wave-per-pair kernel
 * with the image behind it; _lanes_lds: the lane-packed kernel's per wave (its workgroups are one wave), 0 when the plan is not
 * lane-packed.  _waves: waves per workgroup of the one-wave-per-pair fill -- the plan's own when that many slices with their images fit
 * one workgroup's LDS, else 1, and 0 when not even one fits.  _fits: every launch of the plan finds room (the setter refuses otherwise,
 * with `err` for dpx_last_error()).  Pure functions of the plan, which is not changed.  launch_scalars admits a plan only when four plain
 * slices of its longest reference fit one workgroup (lane-packed plans included), so a plan that dpx_plan_batch made always fits: the
 * 0 and the refusal guard against a planner that one day admits longer references (tests/scoretab_fits_main.cpp drives them directly). */
size_t dpx_plan_scoretab_lds(const dpx_plan &p), dpx_plan_scoretab_lanes_lds(const dpx_plan &p);
unsigned dpx_plan_scoretab_waves(const dpx_plan &p);
bool dpx_plan_scoretab_fits(const dpx_plan &p, std::string &err);
const char *dpx_route_kernel_name(dpx_fill_kernel k);
const char *dpx_route_walk_name(dpx_walk_family walk, int walkMode);

/* dpx_batch_describe()'s text up to the pool fields, with dpx_plan_route's arguments.  Returns the length written (snprintf's rules). */
int dpx_plan_describe(const dpx_plan &p, int tbWalk, int zdrop, int endBonus, int substAlphabet, char *buf, size_t cap);

#pragma GCC visibility pop
#endif
