// dpx_main.cpp -- batched GPU driver of the MI355X engine, shaped like the reference's CUDA mains
// (cuda/LNW/LinearNeedlemanWunschV19.cu:357-680, cuda/LinearSmithWaterman.cu:172-435): parse the pairs file,
// fill batch after batch, trace back on the device, and print "<pair> | <score>" + three lines per pair in input order.
// Two batches are in flight on two streams (the copy/compute overlap of cuda/LNW/LinearNeedlemanWunschV13.cu:414-495):
// while the device fills batch k+1, batch k's traceback, packing and D2H run on the other stream and batch k-1 is
// being written to stdout by the printer thread (the software pipeline of V19.cu:546-579).  The device formats every
// pair's block itself (packed variable-length result strings, V15.cu:168-172,372-425), so printing a batch is one fwrite.
// stdout keeps the reference's lines so logs stay diff-able.
// -cigar [M]: instead of the four-line block, one tab-separated line per pair from the engine's alignment records and CIGAR ops
// (dpx_batch_cigars_begin / _end): pair, score, qryLen, qryStart, qryEnd, refLen, refStart, refEnd, matches, alnLen, cigar -- PAF's
// coordinates and the SAM CIGAR ('=' / 'X' ops; "-cigar M" merges them into 'M').  The lines are formatted on the host.
// -md / -cs (only with -cigar): every line gains the fields NM:i:<mismatches + insertions + deletions>, then MD:Z:<text> under -md and
// cs:Z:<text> under -cs, the strings built on the device (dpx_batch_diffs_begin / _end).
//
//   dpx_main -pairs <file> [-match 3] [-mismatch -1] [-open -2 | -gap -2] [-extend -1]
//            [-algo LSW|LNW|ANW|BSW|ASW|BASW|ASG|BANW|BAXT] [-band 128] [-batch N | -pool-gb 4] [-inflight K] [-tune 0|1] [-device 0] [-noprint] [-pack2] [-directions] [-cigar [M] [-md] [-cs]] [-zdrop Z] [-endbonus E] [-matrix FILE] [-localmatrix FILE] [-open2 O2 -extend2 E2] [-localopen2 O2 -localextend2 E2] [-reverse] [-longscores] [-producer P] [-rank r -world w]
//
// -matrix FILE (BANW / BAXT, not with -zdrop / -endbonus): score columns by a substitution matrix (dpx_batch_set_substitution) instead of
// -match / -mismatch.  NCBI text format: '#' lines are comments; one header row of 1..32 single-character column letters; then one row
// per letter: the letter, then that many integers in -128..127.  The row letter is the REFERENCE's.  A lower-case byte takes its
// upper-case letter's code, every other unlisted byte the last letter's ('*' in NCBI files, 'N' in a DNA file).
// -directions with -algo BSW|BASW keeps band direction codes too (DPX_KEEP_LOCAL_BAND_DIRECTIONS, k_bdl_fill): int32 scores, so pairs run that
// the int16 matrices refuse, and the output is what the run without -directions prints.
// -localmatrix FILE (only with -algo BSW|BASW -directions): a -matrix file for those batches, through dpx_batch_set_local_direction_table
// (k_bdlt_fill); composes with -cigar [M] -md -cs.  -matrix itself stays a usage error there.
// -directions with -algo BANW|BAXT keeps band direction codes (DPX_KEEP_BAND_DIRECTIONS); -zdrop / -endbonus / -matrix then go through
// dpx_batch_set_direction_scoring (k_bdx_fill) and print what the run without -directions prints.
// -directions with -algo ANW|ASW|ASG takes -matrix too: the table goes through dpx_batch_set_direction_table (k_dirtab_fill: int32 scores
// against 2^28, so a protein matrix with entries up to 127 runs on long pairs), and the text and CIGARs stay byte equality.
// -scores (any -algo): score-only batches (DPX_SCORE_ONLY: no matrix pool, no traceback); one line per pair, "<number> | <score> | <endRow>
// <endCol>", formatted on the host from dpx_batch_results.  With -algo ANW|ASW|ASG it takes -matrix FILE: the table goes through
// dpx_batch_set_score_table (k_scoretab_fill / k_scoretab_lanes) -- the scoring pass of a database search.  Not with -directions, -cigar,
// -zdrop, -endbonus, -open2 / -extend2 or -reverse, and for the other algorithms not with -matrix.  Without -batch N a -scores run takes
// batches of 20000 pairs, the cap of the budgeted batches (there is no matrix pool to size them by).
// -longscores (only with -algo BANW|BAXT|BSW|BASW, which take -band B): the scoring pass of long banded pairs, DPX_LONG_SCORES on the band-direction
// batch of the algorithm (k_bscore_fill / k_lscore_fill: int32 scores, no pool, no traceback), so pairs run that -scores refuses.  It prints
// -scores' lines and takes -scores' batch sizing.  With -zdrop / -endbonus / -matrix FILE (BANW / BAXT, through
// dpx_batch_set_direction_scoring), -localmatrix FILE (BSW / BASW), -reverse and -pack2.  Not with -scores, -directions, -cigar, -open2 /
// -extend2 or -localopen2 / -localextend2.
// -open2 O2 -extend2 E2 (both or neither; only with -directions and -algo BANW|BAXT): two-piece affine gaps, a gap of length k scores
// max(open + k * extend, O2 + k * E2) (DPX_TWO_PIECE_GAPS and dpx_batch_set_second_gap, k_bd2_fill; bands up to 256).  They combine with
// -zdrop / -endbonus / -matrix through dpx_batch_set_direction_scoring.
// -localopen2 O2 -localextend2 E2 (both or neither; only with -directions and -algo BASW): the same two-piece gaps on the local band-direction
// batches (DPX_LOCAL_TWO_PIECE_GAPS and dpx_batch_set_second_gap, k_lb2_fill; bands up to 256, covering or not).  They combine with
// -localmatrix, -cigar [M] -md -cs, -pack2 and -band.
// -reverse (only with -algo BANW|BAXT, and with every flag those take): every pair is aligned as (reverse(ref), reverse(qry)) on the
// device (dpx_batch_set_reversed) -- a leftward extension, or a global alignment with its gaps at the right end of every ambiguous run.
// Score and, for BAXT, the end cell behind it are the reversed frame's; lines, CIGARs and coordinates are printed along the strings as
// they stand in the file.
//
// Batch size: by default from a matrix-pool BUDGET (-pool-gb, 4 GiB): as many pairs as fit the budget, at most 20000 (the
// reference sizes its buffers once for BATCH_SIZE = 10000 reads of 150 bases, cuda/LNW/LinearNeedlemanWunschV9.cu:26-46,
// V14.cu:144-213 -- 10000 pairs of 1024 x 1024 would be a 22 GB pool whose allocation costs 50 times the fill).  -inflight such
// pools (default 3, at most 8) are built on a helper thread while the file is being parsed and then recycled by every batch: that many
// batches are on the device at a time.  Round 4 (profiles/r04/e2e_*.txt): a batch of 1700 pairs of 1024 x 1024 is a chain fill -> traceback
// -> text -> copy of ~1.5 ms; with two in flight the device idles while this thread creates the next batch (7.1 - 7.9 ms for 10 000 pairs),
// with three the next fill is already queued (6.6 - 7.4 ms); deeper pipelines only add fills that share the same HBM (4 ... 8: slower again).
//
// Multi-GPU: pairs are independent, so every GPU gets one process with its own contiguous shard of the file:
// `-rank r -world w` aligns only pairs [ceil(N/w)*r, ceil(N/w)*(r+1)) (the same split as shard.py / bench.py) and
// prints them with their global pair numbers; tools/run_multi_gpu.sh starts one rank per device and concatenates
// the outputs in rank order, which is input order.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <map>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/dpx_align.h"
#include "parseInput.h"
#include "timing.h"

namespace {

[[noreturn]] void die(const char *what, int rc) {
    printf("%s\nDPX ERROR: %s (%s)\n", what, dpx_strerror(rc), dpx_last_error());
    exit(1);
}

struct InFlight { // one batch between dpx_batch_create and dpx_batch_destroy
    dpx_batch *b = nullptr;
    size_t first = 0, count = 0;
};

// -matrix: the file into an alphabet x alphabet table and the 256-entry byte -> code map; false (with a reason) when it is malformed
bool read_matrix(const char *path, std::vector<int8_t> &scores, int &alphabet, uint8_t (&codeOf)[256], std::string &why) {
    FILE *f = fopen(path, "r");
    if (!f) { why = "cannot open it"; return false; }
    std::string letters;
    std::vector<std::string> rows;
    char line[4096];
    while (fgets(line, sizeof line, f)) {
        std::string t(line);
        if (t.find('\n') == std::string::npos && !feof(f)) { fclose(f); why = "a line is too long"; return false; }
        const size_t a = t.find_first_not_of(" \t\r\n");
        if (a == std::string::npos || t[a] == '#') continue;
        rows.push_back(t);
    }
    fclose(f);
    if (rows.empty()) { why = "no header row"; return false; }
    auto tokens = [](const std::string &t) {
        std::vector<std::string> out;
        size_t at = 0;
        while ((at = t.find_first_not_of(" \t\r\n", at)) != std::string::npos) {
            const size_t end = t.find_first_of(" \t\r\n", at);
            out.push_back(t.substr(at, end == std::string::npos ? end : end - at));
            at = end;
        }
        return out;
    };
    for (const std::string &tok : tokens(rows[0])) {
        if (tok.size() != 1) { why = "a column letter is not a single character"; return false; }
        if (letters.find(tok[0]) != std::string::npos) { why = "a column letter appears twice"; return false; }
        letters += tok[0];
    }
    alphabet = (int)letters.size();
    if (alphabet < 1 || alphabet > 32) { why = "1..32 column letters are allowed"; return false; }
    if ((int)rows.size() != alphabet + 1) { why = "one row per column letter is needed"; return false; }
    scores.assign((size_t)alphabet * alphabet, 0);
    std::vector<bool> seen((size_t)alphabet, false);
    for (int r = 1; r <= alphabet; r++) {
        const std::vector<std::string> tok = tokens(rows[(size_t)r]);
        if ((int)tok.size() != alphabet + 1 || tok[0].size() != 1) { why = "a row needs its letter and one integer per column"; return false; }
        const size_t row = letters.find(tok[0][0]);
        if (row == std::string::npos || seen[row]) { why = "a row letter is unknown or appears twice"; return false; }
        seen[row] = true;
        for (int c = 0; c < alphabet; c++) {
            char *end = nullptr;
            const long v = strtol(tok[(size_t)c + 1].c_str(), &end, 10);
            if (end == tok[(size_t)c + 1].c_str() || *end || v < -128 || v > 127) { why = "an entry is not an integer in -128..127"; return false; }
            scores[row * (size_t)alphabet + (size_t)c] = (int8_t)v;
        }
    }
    for (int x = 0; x < 256; x++) codeOf[x] = (uint8_t)(alphabet - 1);
    for (int k = 0; k < alphabet; k++) codeOf[(unsigned char)letters[(size_t)k]] = (uint8_t)k;
    for (int lo = 'a'; lo <= 'z'; lo++)
        if (letters.find((char)lo) == std::string::npos && letters.find((char)(lo - 32)) != std::string::npos) codeOf[lo] = codeOf[lo - 32];
    return true;
}

} // namespace

static void usage() {
    fprintf(stderr, "usage: dpx_main -pairs <InSeqFile> -match <matchWeight> -mismatch <mismatchWeight> -open <gapWeight> "
                    "[-extend <gapExtend>] [-algo LSW|LNW|ANW|BSW|ASW|BASW|ASG|BANW|BAXT] [-band <B>] [-batch <N>] [-device <D>] [-noprint] [-cigar [M]] [-md] [-cs] (only with -cigar: NM:i:, MD:Z: and cs:Z: fields behind the CIGAR) "
                    "[-zdrop <Z>] [-endbonus <E>] (BAXT only) [-matrix <file>] (BANW / BAXT, not with -zdrop / -endbonus; ANW / ASW / ASG only with -directions) "
                    "[-directions] (direction codes instead of score matrices; -algo BSW|BASW -directions: one code per in-band cell, long pairs run; BANW / BAXT: with -zdrop / -endbonus / -matrix too; -algo ANW|ASW|ASG -directions -matrix <file>: full-matrix affine alignment under a substitution matrix) "
                    "[-localmatrix <file>] (a -matrix file for the local band-direction batches: only with -algo BSW|BASW -directions, not with -matrix) "
                    "[-open2 <O2> -extend2 <E2>] (two-piece gaps: both together, only with -directions and -algo BANW|BAXT) "
                    "[-localopen2 <O2> -localextend2 <E2>] (two-piece gaps on local band-direction batches: both together, only with -directions and -algo BASW) "
                    "[-scores] (score-only batches: one line '<number> | <score> | <endRow> <endCol>' per pair; not with -directions / -cigar / -zdrop / -endbonus / -open2 / -extend2 / -reverse; -matrix <file> with it only for -algo ANW|ASW|ASG; batches of 20000 pairs unless -batch says otherwise) "
                    "[-longscores] (the scoring pass of long banded pairs: -scores' lines from int32 band fills without a pool; only with -algo BANW|BAXT|BSW|BASW, with -zdrop / -endbonus / -matrix <file> (BANW / BAXT), -localmatrix <file> (BSW / BASW), -reverse, -pack2; not with -scores / -directions / -cigar / -open2 / -extend2 / -localopen2 / -localextend2) "
                    "[-reverse] (align every pair right to left on the device, output in the file's orientation; only with -algo BANW|BAXT)\n");
    exit(EXIT_FAILURE);
}

int main(int argc, char *argv[]) {
    if (argc < 3) usage();
    const char *pairFileName = nullptr;
    int match = 3, mismatch = -1, gapOpen = -2, gapExtend = -1, band = 128, device = 0, rank = 0, world = 1;
    size_t batchSize = 0;     // 0: from the pool budget (the reference's BATCH_SIZE, V19.cu:9, assumes short reads)
    double poolGb = 4.0;
    bool print = true, pack2 = false;
    int producerFlag = -1; // producer threads; -1: by batch size (2 for batches of many short pairs, none for few long ones)
    bool cigar = false;      // -cigar: records + CIGAR ops instead of the text pipeline
    unsigned cigarFlags = DPX_CIGAR_EXTENDED;
    unsigned diffKinds = 0;  // -md / -cs (only with -cigar): every line gains NM:i:, then MD:Z: and / or cs:Z: from dpx_batch_diffs_begin / _end
    bool directions = false; // -directions: batches keep 4-bit direction codes (DPX_KEEP_DIRECTIONS): int32 scores, a quarter of the pool per pair
                             // (-algo BANW | BAXT: DPX_KEEP_BAND_DIRECTIONS, -algo BSW | BASW: DPX_KEEP_LOCAL_BAND_DIRECTIONS, one code per in-band cell)
    int zdrop = -1, endBonus = -1; // -zdrop / -endbonus: BAXT's extension mode (dpx_batch_set_extension) on every batch; -1 = off
    bool haveOpen2 = false, haveExtend2 = false; // -open2 / -extend2: the second gap piece (dpx_batch_set_second_gap) on every batch
    int gapOpen2 = 0, gapExtend2 = 0;
    bool haveLocalOpen2 = false, haveLocalExtend2 = false; // -localopen2 / -localextend2: the same on BASW's local band-direction batches (DPX_LOCAL_TWO_PIECE_GAPS)
    bool scoresOnly = false; // -scores: score-only batches (DPX_SCORE_ONLY), one "<number> | <score> | <endRow> <endCol>" line per pair from dpx_batch_results
    bool longScores = false; // -longscores: DPX_LONG_SCORES on the algorithm's band-direction batch, -scores' lines from dpx_batch_results
    bool reverse = false;    // -reverse: every pair of every batch is reversed on the device (dpx_batch_set_reversed)
    const char *matrixFile = nullptr; // -matrix: a substitution table (dpx_batch_set_substitution) on every batch
    const char *localMatrixFile = nullptr; // -localmatrix: a substitution table (dpx_batch_set_local_direction_table) on every BSW / BASW band-direction batch
    int inflight = 3;      // batches on the device at a time (= matrix pools reserved)
    int tuneFlag = -1;     // -1: by the length of the job
    std::string algoName = "LSW";
    for (int i = 1; i < argc; i++) {
        auto next = [&](const char *flag) -> const char * {
            if (i + 1 >= argc) { fprintf(stderr, "missing value for %s\n", flag); exit(EXIT_FAILURE); }
            return argv[++i];
        };
        if (!strcmp(argv[i], "-pairs")) pairFileName = next("-pairs");
        else if (!strcmp(argv[i], "-match")) match = atoi(next("-match"));
        else if (!strcmp(argv[i], "-mismatch")) mismatch = atoi(next("-mismatch"));
        else if (!strcmp(argv[i], "-open") || !strcmp(argv[i], "-gap")) gapOpen = atoi(next("-open"));
        else if (!strcmp(argv[i], "-extend")) gapExtend = atoi(next("-extend"));
        else if (!strcmp(argv[i], "-algo")) algoName = next("-algo");
        else if (!strcmp(argv[i], "-band")) band = atoi(next("-band"));
        else if (!strcmp(argv[i], "-batch")) batchSize = (size_t)atoll(next("-batch"));
        else if (!strcmp(argv[i], "-pool-gb")) poolGb = atof(next("-pool-gb"));
        else if (!strcmp(argv[i], "-device")) device = atoi(next("-device"));
        else if (!strcmp(argv[i], "-noprint")) print = false;
        else if (!strcmp(argv[i], "-pack2")) pack2 = true;
        else if (!strcmp(argv[i], "-directions")) directions = true;
        else if (!strcmp(argv[i], "-cigar")) {
            cigar = true;
            if (i + 1 < argc && !strcmp(argv[i + 1], "M")) { cigarFlags = DPX_CIGAR_M; i++; }
        }
        else if (!strcmp(argv[i], "-md")) diffKinds |= DPX_DIFF_MD;
        else if (!strcmp(argv[i], "-cs")) diffKinds |= DPX_DIFF_CS;
        else if (!strcmp(argv[i], "-zdrop")) zdrop = atoi(next("-zdrop"));
        else if (!strcmp(argv[i], "-endbonus")) endBonus = atoi(next("-endbonus"));
        else if (!strcmp(argv[i], "-matrix")) matrixFile = next("-matrix");
        else if (!strcmp(argv[i], "-localmatrix")) localMatrixFile = next("-localmatrix");
        else if (!strcmp(argv[i], "-open2")) { gapOpen2 = atoi(next("-open2")); haveOpen2 = true; }
        else if (!strcmp(argv[i], "-extend2")) { gapExtend2 = atoi(next("-extend2")); haveExtend2 = true; }
        else if (!strcmp(argv[i], "-localopen2")) { gapOpen2 = atoi(next("-localopen2")); haveLocalOpen2 = true; }
        else if (!strcmp(argv[i], "-localextend2")) { gapExtend2 = atoi(next("-localextend2")); haveLocalExtend2 = true; }
        else if (!strcmp(argv[i], "-reverse")) reverse = true;
        else if (!strcmp(argv[i], "-scores")) scoresOnly = true;
        else if (!strcmp(argv[i], "-longscores")) longScores = true;
        else if (!strcmp(argv[i], "-producer")) producerFlag = atoi(next("-producer"));
        else if (!strcmp(argv[i], "-inflight")) inflight = atoi(next("-inflight"));
        else if (!strcmp(argv[i], "-tune")) tuneFlag = atoi(next("-tune"));
        else if (!strcmp(argv[i], "-rank")) rank = atoi(next("-rank"));
        else if (!strcmp(argv[i], "-world")) world = atoi(next("-world"));
        else { fprintf(stderr, "unknown argument: %s\n", argv[i]); exit(EXIT_FAILURE); }
    }
    if (!pairFileName) { fprintf(stderr, "need -pairs <file>\n"); exit(EXIT_FAILURE); }
    if (poolGb < 0.0625 || poolGb > 200) { fprintf(stderr, "bad -pool-gb\n"); exit(EXIT_FAILURE); }
    if (world < 1 || rank < 0 || rank >= world) { fprintf(stderr, "bad -rank/-world\n"); exit(EXIT_FAILURE); }
    if (inflight < 1 || inflight > 8) { fprintf(stderr, "bad -inflight (1..8)\n"); exit(EXIT_FAILURE); }
    const int algo = algoName == "LNW" ? DPX_ALGO_LNW : algoName == "LSW" ? DPX_ALGO_LSW : algoName == "ANW" ? DPX_ALGO_ANW
                     : algoName == "BSW" ? DPX_ALGO_BSW : algoName == "ASW" ? DPX_ALGO_ASW : algoName == "BASW" ? DPX_ALGO_BASW : algoName == "ASG" ? DPX_ALGO_ASG : algoName == "BANW" ? DPX_ALGO_BANW : algoName == "BAXT" ? DPX_ALGO_BAXT : -1;
    if (algo < 0) { fprintf(stderr, "unknown -algo %s\n", algoName.c_str()); exit(EXIT_FAILURE); }
    if ((zdrop != -1 || endBonus != -1) && algo != DPX_ALGO_BAXT) usage();
    const bool twoPiece = haveOpen2 || haveExtend2;
    if (twoPiece && (!(haveOpen2 && haveExtend2) || !directions || (algo != DPX_ALGO_BANW && algo != DPX_ALGO_BAXT))) usage();
    const bool localTwoPiece = haveLocalOpen2 || haveLocalExtend2;
    if (localTwoPiece && (!(haveLocalOpen2 && haveLocalExtend2) || twoPiece || !directions || algo != DPX_ALGO_BASW)) usage();
    if (reverse && algo != DPX_ALGO_BANW && algo != DPX_ALGO_BAXT) usage();
    if (diffKinds && !cigar) usage();
    if (scoresOnly && (directions || cigar || zdrop != -1 || endBonus != -1 || twoPiece || localTwoPiece || reverse)) usage();
    const bool bandedAlgo = algo == DPX_ALGO_BSW || algo == DPX_ALGO_BASW || algo == DPX_ALGO_BANW || algo == DPX_ALGO_BAXT;
    if (longScores && (scoresOnly || directions || cigar || twoPiece || localTwoPiece || !bandedAlgo)) usage();
    const bool resultLines = scoresOnly || longScores; // one "<number> | <score> | <endRow> <endCol>" line per pair, no pool, no text
    std::vector<int8_t> substScores;
    int substAlphabet = 0;
    uint8_t substCode[256];
    // -matrix on a direction batch of the three full-matrix affine algorithms (dpx_batch_set_direction_table)
    const bool directionTable = matrixFile && directions && (algo == DPX_ALGO_ANW || algo == DPX_ALGO_ASW || algo == DPX_ALGO_ASG);
    // -matrix on a score-only batch of the same three (dpx_batch_set_score_table); the other algorithms have no score-only table kernel
    const bool scoreTable = matrixFile && scoresOnly && (algo == DPX_ALGO_ANW || algo == DPX_ALGO_ASW || algo == DPX_ALGO_ASG);
    if (matrixFile) {
        if (scoresOnly && !scoreTable) usage();
        if (((algo != DPX_ALGO_BANW && algo != DPX_ALGO_BAXT) && !directionTable && !scoreTable) || zdrop != -1 || endBonus != -1) usage();
        std::string why;
        if (!read_matrix(matrixFile, substScores, substAlphabet, substCode, why)) {
            fprintf(stderr, "-matrix %s: %s\n", matrixFile, why.c_str());
            usage();
        }
    }
    if (localMatrixFile) {
        if (matrixFile || !(directions || longScores) || (algo != DPX_ALGO_BSW && algo != DPX_ALGO_BASW)) usage();
        std::string why;
        if (!read_matrix(localMatrixFile, substScores, substAlphabet, substCode, why)) {
            fprintf(stderr, "-localmatrix %s: %s\n", localMatrixFile, why.c_str());
            usage();
        }
    }

    printf("[Device Details]\n");
    int deviceCount = 0;
    int rc = dpx_device_count(&deviceCount);
    if (rc != DPX_OK || deviceCount == 0) die("FAILED TO GET DEVICE COUNT", rc != DPX_OK ? rc : DPX_ERR_NO_DEVICE);
    printf("Device count: %d\n", deviceCount);
    if ((rc = dpx_init(device)) != DPX_OK) die("FAILED TO BIND DEVICE", rc);
    char name[256];
    int cus = 0;
    size_t hbm = 0;
    if ((rc = dpx_device_info(name, sizeof name, &cus, &hbm)) != DPX_OK) die("FAILED TO GET DEVICE PROPERTIES", rc);
    printf("Device %d is%s with %d compute units, %.0f GB.\n\n", device, name, cus, (double)hbm / 1e9);

    // the two matrix pools of the pipeline are built while the file is parsed (nothing else needs the device yet)
    // (the budget is per score plane: the three planes of the affine algorithm get three times the bytes, so that a batch holds
    // as many pairs -- and fills the chip as well -- as a linear-gap batch of the same shapes)
    // (-directions: one 4-bit code per cell whatever the algorithm, so the budget stays per batch and holds 4x -- ANW 12x -- the pairs)
    const bool threePlanes = algo == DPX_ALGO_ANW || algo == DPX_ALGO_ASW || algo == DPX_ALGO_BASW || algo == DPX_ALGO_ASG || algo == DPX_ALGO_BANW || algo == DPX_ALGO_BAXT; // H, I, D
    const bool bandAlgo = algo == DPX_ALGO_BSW || algo == DPX_ALGO_BASW || algo == DPX_ALGO_BANW || algo == DPX_ALGO_BAXT; // band layout: 2 * band + 8 columns per row
    const size_t poolBudget = (size_t)(poolGb * (double)(1ull << 30)) * (threePlanes && !directions ? 3 : 1);
    std::thread reserve;
    // (and pinned text buffers: one being printed, one per batch in flight, two spare)
    const bool budgetedBatches = batchSize == 0 && !resultLines; // (-scores / -longscores: the batches have no pool and no text)
    if (batchSize == 0 && resultLines) batchSize = 20000; // no pool to budget against: the cap the budgeted batches have below (enough waves for the chip, small enough to pipeline)
    if (budgetedBatches) reserve = std::thread([poolBudget, print, inflight]() { (void)dpx_pool_reserve(poolBudget, inflight); if (print) (void)dpx_text_reserve((size_t)16 << 20, inflight + 3); });

    printf("Parsing input file: %s\n", pairFileName);
    seqPair *sequenceIdxs;
    char *sequences;
    // one process per GPU: every rank maps the file and materialises only its own contiguous ceil(N/world)-sized shard
    size_t shardFirst = 0, totalPairs = 0;
    inputInfo fileInfo = world > 1 ? parseInputShard(pairFileName, rank, world, sequenceIdxs, sequences, shardFirst, totalPairs)
                                   : parseInput(pairFileName, sequenceIdxs, sequences);
    if (world == 1) totalPairs = fileInfo.numPairs;
    printf("Num Pairs: %zu\n\n", totalPairs);
    const size_t shardLo = 0, shardHi = fileInfo.numPairs; // indices into this rank's own records
    if (world > 1) printf("Rank %d of %d: pairs [%zu, %zu)\n\n", rank, world, shardFirst, shardFirst + fileInfo.numPairs);

    if (batchSize == 0) { // pairs per batch from the pool budget: 2 bytes per cell and plane, rows / columns padded as the layouts pad them
        const double cols = (bandAlgo && 2.0 * band < (double)fileInfo.maxReferenceLength) ? 2.0 * band + 8 : (double)fileInfo.maxReferenceLength + 128;
        // (-directions: half a byte per cell; rows rounded up to whole stripes of 64 * R, every stripe n + 63 steps rounded up to 32 / R --
        // the code layout of csrc/dpx_dir.h, R picked from the longest query as dpx_batch_create picks it)
        const long long mq = fileInfo.maxQueryLength, dR = mq <= 128 ? 2 : mq <= 256 ? 4 : (mq <= 512 || algo != DPX_ALGO_LNW) ? 8 : 16;
        const double dirRows = (double)((mq + 64 * dR - 1) / (64 * dR) * 64 * dR);
        const double dirCols = (double)(((long long)fileInfo.maxReferenceLength + 63 + 32 / dR - 1) / (32 / dR) * (32 / dR));
        // (-directions on a banded algorithm: ceil((m + n - 1) / Gd) chunks of 1 KiB, Gd = 32 / C steps per chunk, C = cells per lane of the
        // band -- the layout of csrc/dpx_banddir.h)
        // (BSW / BASW under a covering band run as LSW / ASW direction batches: the estimate above)
        const bool localAlgo = algo == DPX_ALGO_BSW || algo == DPX_ALGO_BASW;
        const bool bandDirections = directions && bandAlgo && (!localAlgo || localTwoPiece || (long long)band < std::max<long long>(mq, fileInfo.maxReferenceLength)); // (two local pieces: the band kernel, covering or not)
        const long long bC0 = ((long long)band + 63) / 64, bC = bC0 <= 1 ? 1 : bC0 <= 2 ? 2 : bC0 <= 4 ? 4 : 8, bGd = ((twoPiece || localTwoPiece) ? 16 : 32) / bC; // (two-piece: a byte per cell, csrc/dpx_banddir2.h)
        const double bandDirChunks = (double)((mq + (long long)fileInfo.maxReferenceLength - 1 + bGd - 1) / bGd);
        const double perPair = bandDirections ? 1024.0 * bandDirChunks + 1024.0
                             : directions ? 0.5 * dirRows * dirCols + 1024.0
                                          : 2.0 * (threePlanes ? 3 : 1) * ((double)fileInfo.maxQueryLength + 64) * cols;
        const double fit = (double)poolBudget / (perPair > 0 ? perPair : 1);
        batchSize = (size_t)std::min(20000.0, std::max(64.0, fit));
        batchSize &= ~(size_t)1; // even: the packed kernels fill COUPLES of equal-shaped pairs, an odd batch leaves one pair to a second kernel
                                 // of one wave (0.4 ms of latency on 1024 x 1024, and on a shared hardware queue the couples' kernel waits for it)
    }
    // -pack2: the parse step emits four bases per byte (alphabets of up to four symbols); the batches then move a quarter of the
    // sequence bytes to the device, which expands them (dpx_batch_create_packed2).  Like parsing, outside the timer.
    std::vector<uint8_t> packed;
    uint8_t alphabet[4] = {0, 0, 0, 0};
    if (pack2) {
        packed.resize((fileInfo.numBytes + 3) / 4 + 1);
        rc = dpx_pack2(sequences, fileInfo.numBytes, reinterpret_cast<const dpx_seq_pair *>(sequenceIdxs), fileInfo.numPairs, alphabet, packed.data());
        if (rc == DPX_ERR_UNSUPPORTED) { fprintf(stderr, "-pack2: more than four distinct symbols, keeping bytes\n"); pack2 = false; }
        else if (rc != DPX_OK) die("FAILED TO PACK THE SEQUENCES", rc);
    }
    if (reserve.joinable()) reserve.join();
    // Producer threads (below) keep one batch more alive than -inflight says; without a pool of its own that batch would build one inside
    // the timed region (a 4-GiB pool: 100 - 450 ms, seen with -producer 2 on long pairs; a short-read pool: a few ms of the job's six).
    const int producers = producerFlag >= 0 ? std::min(producerFlag, 8) : (batchSize >= 8192 ? 2 : 0);
    if (budgetedBatches && producers > 0 && producers + 1 > inflight) {
        (void)dpx_pool_reserve(poolBudget, std::min(8, producers + 1));
        if (print) (void)dpx_text_reserve((size_t)16 << 20, std::min(9, producers + 1 + 3));
    }
    start_timer();
    uint64_t kernel_time = 0, memalloc_time = 0, backtracking_time = 0, printing_time = 0; // usec, as V19.cu:411-415
    uint64_t traceback_kernel_time = 0; // device time of the traceback + text kernels (backtracking_time is the host's wait for them)
    printf("Pair # | Score\n");
    const dpx_params prm{algo, match, mismatch, gapOpen, gapExtend, band};
    static_assert(sizeof(seqPair) == sizeof(dpx_seq_pair), "seqPair must stay layout-compatible with the C ABI");

    // pipeline of three host threads: the producer issues [create + fill + output_begin] of batch k+1 while this thread waits
    // for batch k and takes its text; the printer thread writes batch k-1 meanwhile from the text buffer it took over, so batch
    // k-1 itself is destroyed (its matrix pool parked for batch k+1) as soon as its text is on the host.
    std::thread printer;
    char *printingText = nullptr;
    InFlight filling; // issued to the device, not yet waited for
    auto retire_printed = [&]() {
        if (printer.joinable()) { const uint64_t t0 = get_time(); printer.join(); printing_time += get_time() - t0; }
        if (printingText) { dpx_text_free(printingText); printingText = nullptr; }
    };
    auto finish = [&](InFlight &f) { // wait for batch f, account its kernel time, hand its text to the printer
        uint64_t t0 = get_time();
        char *text = nullptr;
        size_t bytes = 0;
        std::string lines; // -cigar: the batch's lines, formatted here while the batch (which owns the records and ops) is alive
        if (print && resultLines) { // no device text: the three result arrays, formatted here
            std::vector<int32_t> scores(f.count), endRow(f.count), endCol(f.count);
            if ((rc = dpx_batch_results(f.b, scores.data(), endRow.data(), endCol.data())) != DPX_OK) die("RESULTS FAILED", rc);
            char line[96];
            for (size_t k = 0; k < f.count; k++)
                lines.append(line, (size_t)snprintf(line, sizeof line, "%zu | %d | %d %d\n", shardFirst + f.first + k, scores[k], endRow[k], endCol[k]));
        } else if (print && cigar) {
            const dpx_alignment *recs = nullptr;
            const uint32_t *ops = nullptr;
            uint64_t numOps = 0;
            if ((rc = dpx_batch_cigars_end(f.b, &recs, &ops, &numOps)) != DPX_OK) die("TRACEBACK FAILED", rc);
            std::vector<int32_t> scores(f.count);
            if ((rc = dpx_batch_results(f.b, scores.data(), nullptr, nullptr)) != DPX_OK) die("RESULTS FAILED", rc);
            const char *diffText[2] = {nullptr, nullptr}; // MD, cs: the batch's strings back to back, cut at the offsets
            const uint64_t *diffOff[2] = {nullptr, nullptr};
            if ((diffKinds & DPX_DIFF_MD) && (rc = dpx_batch_diffs_end(f.b, DPX_DIFF_MD, &diffText[0], nullptr, &diffOff[0])) != DPX_OK) die("MD FAILED", rc);
            if ((diffKinds & DPX_DIFF_CS) && (rc = dpx_batch_diffs_end(f.b, DPX_DIFF_CS, &diffText[1], nullptr, &diffOff[1])) != DPX_OK) die("CS FAILED", rc);
            std::vector<char> cg;
            for (size_t k = 0; k < f.count; k++) {
                const dpx_alignment &r = recs[k];
                const seqPair &sp = sequenceIdxs[f.first + k];
                size_t need = 0;
                cg.resize((size_t)r.numOps * 11 + 2); // at most ten digits and a letter per op
                if ((rc = dpx_cigar_text(ops + r.opsOffset, (size_t)r.numOps, cg.data(), cg.size(), &need)) != DPX_OK) die("CIGAR TEXT FAILED", rc);
                char head[256];
                const int h = snprintf(head, sizeof head, "%zu\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t", shardFirst + f.first + k, scores[k],
                                       (int)sp.querySize, r.qryStart, r.qryEnd, (int)sp.referenceSize, r.refStart, r.refEnd, r.matches,
                                       r.matches + r.mismatches + r.insertions + r.deletions);
                lines.append(head, (size_t)h);
                lines.append(cg.data(), need);
                if (diffKinds) {
                    lines.append(head, (size_t)snprintf(head, sizeof head, "\tNM:i:%d", r.mismatches + r.insertions + r.deletions));
                    for (int d = 0; d < 2; d++)
                        if (diffText[d]) {
                            lines.append(d == 0 ? "\tMD:Z:" : "\tcs:Z:");
                            lines.append(diffText[d] + diffOff[d][k], (size_t)(diffOff[d][k + 1] - diffOff[d][k]));
                        }
                }
                lines.push_back('\n');
            }
        } else if (print) {
            if ((rc = dpx_batch_output_take(f.b, &text, &bytes)) != DPX_OK) die("TRACEBACK FAILED", rc);
        } else if ((rc = dpx_batch_sync(f.b)) != DPX_OK) die("KERNEL FAILED", rc);
        double usec = 0;
        if ((rc = dpx_batch_last_fill_usec(f.b, &usec)) != DPX_OK) die("KERNEL TIMING FAILED", rc);
        kernel_time += (uint64_t)usec;
        if (print && !resultLines && dpx_batch_last_output_usec(f.b, &usec) == DPX_OK) traceback_kernel_time += (uint64_t)usec;
        backtracking_time += get_time() - t0;
        t0 = get_time();
        dpx_batch_destroy(f.b);
        f = InFlight{};
        memalloc_time += get_time() - t0;
        retire_printed();
        printingText = text;
        if (print && (cigar || resultLines)) printer = std::thread([s = std::move(lines)]() { fwrite(s.data(), 1, s.size(), stdout); });
        else if (print) printer = std::thread([text, bytes]() { fwrite(text, 1, bytes, stdout); });
    };
    size_t shardCells = 0;
    for (size_t i = shardLo; i < shardHi; i++) shardCells += (size_t)sequenceIdxs[i].referenceSize * (size_t)sequenceIdxs[i].querySize;
    fflush(stdout); // the printer thread writes with fwrite from here on
    // One batch: create, fill, start the output.  Two batches alive need two matrix pools.  Allocating tens of GB costs hundreds of
    // ms (more than the overlap of one batch's traceback with the next batch's fill can ever win back), so batches with pools of
    // 16 GiB or more (an explicit -batch) run one after the other and share ONE parked pool; the printer thread still overlaps.
    size_t maxAlive = (size_t)inflight;
    // Pool placement: the same fill runs up to 27 % apart on two allocations of one pool (ANW 1000 x 1024^2: 0.94 vs 1.20 ms;
    // no address pattern of the fill moves it, profiles/r04/anw_group_sweep_on_fixed_allocations.txt).  A job of 256 batches or more lets the engine shop
    // for its pools with the first batch that uses each of them (DPX_TUNE_PLACEMENT: five candidate allocations, four fills each -- ~35 ms per pool,
    // once); shorter jobs would not earn that back.  -tune 0|1 overrides.
    const size_t jobBatches = (shardHi - shardLo + batchSize - 1) / batchSize;
    const bool tunePools = tuneFlag >= 0 ? tuneFlag != 0 : jobBatches >= 256;
    std::atomic<int> tuned{0}; // batches created with the flag so far (one per pool in flight)
    std::atomic<uint64_t> create_time{0}; // summed over the threads that produce
    auto produce = [&](size_t first) -> InFlight {
        InFlight next;
        next.first = first;
        next.count = std::min(batchSize, shardHi - first);
        const uint64_t t0 = get_time();
        const bool bandDirections = (directions || longScores) && (algo == DPX_ALGO_BANW || algo == DPX_ALGO_BAXT);
        const bool localDirections = (directions || longScores) && (algo == DPX_ALGO_BSW || algo == DPX_ALGO_BASW);
        const unsigned flags = (longScores ? DPX_LONG_SCORES : 0u) | (twoPiece ? DPX_TWO_PIECE_GAPS : localTwoPiece ? DPX_LOCAL_TWO_PIECE_GAPS : 0u) | (bandDirections ? DPX_KEEP_BAND_DIRECTIONS : localDirections ? DPX_KEEP_LOCAL_BAND_DIRECTIONS : directions ? DPX_KEEP_DIRECTIONS : scoresOnly ? DPX_SCORE_ONLY : DPX_KEEP_MATRICES) | DPX_TIME_FILLS | ((tunePools && !resultLines && tuned.fetch_add(1) < inflight) ? DPX_TUNE_PLACEMENT : 0u);
        int prc = pack2 ? dpx_batch_create_packed2(-1, &prm, packed.data(), fileInfo.numBytes, alphabet, reinterpret_cast<const dpx_seq_pair *>(sequenceIdxs),
                                                   first, next.count, flags, &next.b)
                        : dpx_batch_create(&prm, sequences, fileInfo.numBytes, reinterpret_cast<const dpx_seq_pair *>(sequenceIdxs), first, next.count,
                                           flags, &next.b);
        if (prc != DPX_OK) die("FAILED TO CREATE DEVICE BATCH", prc);
        if ((twoPiece || localTwoPiece) && (prc = dpx_batch_set_second_gap(next.b, gapOpen2, gapExtend2)) != DPX_OK) die("FAILED TO SET THE SECOND GAP PIECE", prc);
        if (bandDirections) { // the one setter of a band-direction batch: the two below refuse it
            if ((zdrop != -1 || endBonus != -1 || matrixFile) &&
                (prc = dpx_batch_set_direction_scoring(next.b, zdrop, endBonus, matrixFile ? substScores.data() : nullptr, substAlphabet, substCode)) != DPX_OK)
                die(matrixFile ? "FAILED TO SET THE SUBSTITUTION MATRIX" : "FAILED TO SET THE EXTENSION MODE", prc);
        } else if (localMatrixFile) { // (a covering band is refused here: it runs k_linear_dir / k_asw_dir, which take no table)
            if ((prc = dpx_batch_set_local_direction_table(next.b, substScores.data(), substAlphabet, substCode)) != DPX_OK) die("FAILED TO SET THE SUBSTITUTION MATRIX", prc);
        } else if (directionTable) {
            if ((prc = dpx_batch_set_direction_table(next.b, substScores.data(), substAlphabet, substCode)) != DPX_OK) die("FAILED TO SET THE SUBSTITUTION MATRIX", prc);
        } else if (scoreTable) {
            if ((prc = dpx_batch_set_score_table(next.b, substScores.data(), substAlphabet, substCode)) != DPX_OK) die("FAILED TO SET THE SUBSTITUTION MATRIX", prc);
        } else {
            if ((zdrop != -1 || endBonus != -1) && (prc = dpx_batch_set_extension(next.b, zdrop, endBonus)) != DPX_OK) die("FAILED TO SET THE EXTENSION MODE", prc);
            if (matrixFile && (prc = dpx_batch_set_substitution(next.b, substScores.data(), substAlphabet, substCode)) != DPX_OK) die("FAILED TO SET THE SUBSTITUTION MATRIX", prc);
        }
        if (reverse) {
            const std::vector<uint8_t> all(next.count, 1);
            if ((prc = dpx_batch_set_reversed(next.b, all.data())) != DPX_OK) die("FAILED TO SET THE ORIENTATION", prc);
        }
        create_time += get_time() - t0;
        if ((prc = dpx_batch_fill(next.b, nullptr)) != DPX_OK) die("KERNEL LAUNCH FAILED", prc);
        // global pair numbers: shardFirst + index inside the shard
        if (print && resultLines) { /* (nothing to start: finish reads the results) */ }
        else if (print && cigar) { if ((prc = dpx_batch_cigars_begin(next.b, cigarFlags)) != DPX_OK) die("TRACEBACK LAUNCH FAILED", prc);
            if (diffKinds && (prc = dpx_batch_diffs_begin(next.b, diffKinds)) != DPX_OK) die("MD / CS LAUNCH FAILED", prc); }
        else if (print && (prc = dpx_batch_output_begin(next.b, shardFirst + first)) != DPX_OK) die("TRACEBACK LAUNCH FAILED", prc);
        return next;
    };
    auto pool_is_huge = [](const InFlight &f) { uint64_t mb = 0; dpx_batch_info(f.b, nullptr, nullptr, &mb, nullptr); return mb >= (16ull << 30); };
    // Batches of many short pairs are bound by the HOST (dpx_batch_create: 1.1-1.4 ms per 20000 pairs for validation, two counting
    // sorts, the wave packing and the H2D copies, against 0.15 + 0.3 ms of kernels).  Round 3 moved that onto ONE producer thread
    // (100k short reads: 12 -> 7.5 ms, of which 5.9 ms were still that thread creating five batches one after the other); batches are
    // independent, so round 4 creates them on several threads (-producer P, default 2: 100k short reads 6.3 -> 5.9 ms LSW, 9.2 -> 8.1 ANW; three or four threads contend and lose again, profiles/r04/e2e_producers.txt): every thread takes the next batch index, creates
    // and fills the batch and starts its output, this thread finishes the batches in input order.  At most -inflight batches exist
    // between the one being finished and the newest one being created.  Batches of few long pairs are bound by the device, and there one
    // issuing thread is as fast or faster (10000 x 1024^2: 8.1-8.9 vs 8.4-9.3 ms).  -producer 0 turns the threads off.
    if (producers > 0) {
        const size_t numBatches = (shardHi - shardLo + batchSize - 1) / batchSize;
        if ((size_t)producers + 1 > maxAlive) maxAlive = std::min<size_t>(8, (size_t)producers + 1); // (every producer needs a slot of its own)
        std::mutex qm;
        std::condition_variable qcv;
        std::map<size_t, InFlight> ready; // created, filling, not yet finished; by batch index
        std::atomic<size_t> nextBatch{0};
        size_t consumed = 0; // batches finished (and destroyed) so far
        std::vector<std::thread> pool;
        for (int t = 0; t < producers; t++)
            pool.emplace_back([&]() {
                (void)dpx_init(device); // (binds the device for this thread)
                for (;;) {
                    const size_t k = nextBatch.fetch_add(1);
                    if (k >= numBatches) return;
                    {
                        std::unique_lock<std::mutex> lk(qm);
                        qcv.wait(lk, [&]() { return k < consumed + maxAlive; });
                    }
                    const InFlight next = produce(shardLo + k * batchSize);
                    std::lock_guard<std::mutex> lk(qm);
                    if (pool_is_huge(next)) maxAlive = 1;
                    ready[k] = next;
                    qcv.notify_all();
                }
            });
        for (size_t k = 0; k < numBatches; k++) {
            {
                std::unique_lock<std::mutex> lk(qm);
                qcv.wait(lk, [&]() { return ready.count(k) != 0; });
                filling = ready[k];
                ready.erase(k);
            }
            finish(filling); // (destroys the batch: its pool is parked for the batches still to be created)
            std::lock_guard<std::mutex> lk(qm);
            consumed = k + 1;
            qcv.notify_all();
        }
        for (std::thread &t : pool) t.join();
    } else {
        std::deque<InFlight> alive; // issued to the device, oldest first
        for (size_t first = shardLo; first < shardHi; first += batchSize) {
            if (alive.size() >= maxAlive) { finish(alive.front()); alive.pop_front(); } // (its pool is parked for the batch produced next)
            alive.push_back(produce(first));
            if (pool_is_huge(alive.back())) maxAlive = 1;
        }
        while (!alive.empty()) { finish(alive.front()); alive.pop_front(); }
    }
    memalloc_time += create_time.load();
    retire_printed();
    fflush(stdout);

    const uint64_t elapsed_time = get_elapsed_time();
    printf("Elapsed time (usec): %llu\n", (unsigned long long)elapsed_time);
    printf("Num Pairs: %zu\n", totalPairs);
    printf("Num Cells: %zu\n", fileInfo.numCells);
    printf("Reference length min/avg/max: %zu / %.1f / %zu\n", fileInfo.minReferenceLength, fileInfo.avgReferenceLength, fileInfo.maxReferenceLength);
    printf("Query length min/avg/max: %zu / %.1f / %zu\n", fileInfo.minQueryLength, fileInfo.avgQueryLength, fileInfo.maxQueryLength);
    printf("Kernel time (usec): %llu\n", (unsigned long long)kernel_time);
    printf("Memory management time (usec): %llu\n", (unsigned long long)memalloc_time);
    printf("Backtracking time (usec): %llu\n", (unsigned long long)backtracking_time);
    printf("Traceback kernel time (usec): %llu\n", (unsigned long long)traceback_kernel_time);
    printf("Printing wait time (usec): %llu\n", (unsigned long long)printing_time);
    // GCUPS exactly as the reference computes it (V12.cu:487-491): numCells / kernel seconds / 1e9
    printf("GCUPS: %f\n", kernel_time ? (double)shardCells / ((double)kernel_time * 1e-6) / 1e9 : 0.0);

    printf("Cleaning up\n");
    cleanupParsedFile(sequenceIdxs, sequences);
    return 0;
}
