/* dpx_output.cpp -- what a filled batch hands out besides scores: result text, CIGARs and difference strings, all three from one device
 * traceback (host side of libdpxalign.so; the dpx_batch_output_*, _traceback, _cigars_*, _diffs_* entry points of include/dpx_align.h). */
#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "dpx_batch.h"
#include "dpx_cigar.h"
#include "dpx_diff.h"
#include "dpx_reverse.h"

extern "C" {

/* ---- result text: device traceback -> per-pair block lengths -> exclusive scan -> packed blocks -> D2H of the real bytes ----
 * (the reference's V15 packed variable-length strings, cuda/LNW/LinearNeedlemanWunschV15.cu:168-172,372-425; the blocks are
 * already formatted as c++/main.cpp prints them, so a driver writes a batch with one fwrite) */

/* The traceback lines of the last fill, on the batch's stream: the one place that orders the stream behind a fill on a caller's stream
 * (without blocking the host) and launches the walk, for the text pipeline, the CIGAR path and the difference strings alike.  b->dTb must
 * exist.  `started` (output_begin's timing) is recorded between the two; the walk is skipped when the lines of this fill are there already. */
static int lines_behind_fill(dpx_batch *b, hipEvent_t started = nullptr) {
    if (b->lastStream && b->lastStream != b->stream) {
        if (!b->evOrder) HIP_TRY(hipEventCreateWithFlags(&b->evOrder, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(b->evOrder, b->lastStream));
        HIP_TRY(hipStreamWaitEvent(b->stream, b->evOrder, 0));
    }
    if (started) HIP_TRY(hipEventRecord(started, b->stream));
    if (b->tbLinesValid) return DPX_OK;
    const dpx_route r = route_of(b); /* (which walk, and why: dpx_plan.cpp) */
    const int n = (int)b->numPairs, walk = r.walkMode;
    switch (r.walk) {
    case DPX_WALK_PLAIN: HIP_TRY(dpx_launch_traceback(b->args, n, b->kernelAlgo, b->R, b->planes, walk, b->dTbOff, b->dTb.get(), b->dTbLen, b->stream)); break;
    case DPX_WALK_DIR: HIP_TRY(dpx_launch_traceback_dir(b->dirArgs, n, b->kernelAlgo, b->R, b->dTbOff, b->dTb.get(), b->dTbLen, b->stream)); break;
    case DPX_WALK_BASW: HIP_TRY(dpx_launch_basw_traceback(b->args, n, walk, b->dTbOff, b->dTb.get(), b->dTbLen, b->stream)); break;
    case DPX_WALK_BANW: HIP_TRY(dpx_launch_banw_traceback(b->args, n, walk, b->dTbOff, b->dTb.get(), b->dTbLen, b->stream)); break;
    case DPX_WALK_SUBST: HIP_TRY(dpx_launch_subst_traceback(subst_args(b), n, walk, b->dTbOff, b->dTb.get(), b->dTbLen, b->stream)); break;
    case DPX_WALK_BDIR: HIP_TRY(dpx_launch_bdir_traceback(b->args, n, b->dTbOff, b->dTb.get(), b->dTbLen, b->stream)); break;
    case DPX_WALK_BD2: HIP_TRY(dpx_launch_bd2_traceback(b->args, n, b->dTbOff, b->dTb.get(), b->dTbLen, b->stream)); break;
    case DPX_WALK_BDL: HIP_TRY(dpx_launch_bdl_traceback(b->args, n, b->prm.algo == DPX_ALGO_BASW, b->dTbOff, b->dTb.get(), b->dTbLen, b->stream)); break;
    case DPX_WALK_LB2: HIP_TRY(dpx_launch_lb2_traceback(b->args, n, b->dTbOff, b->dTb.get(), b->dTbLen, b->stream)); break;
    }
    /* reversed pairs (dpx_batch_set_reversed): their lines come out of the walk in the reversed frame and are turned round here, once */
    if (b->revCount) HIP_TRY(dpx_launch_flip_lines(b->dPairs, b->dFlagged, (int)b->revCount, b->dTbLen, b->dTbOff, b->dTb.get(), b->stream));
    b->tbLinesValid = true;
    return DPX_OK;
}

/* what every *_begin asks of the batch once its own arguments have passed: matrices, a fill, and the batch's device bound */
static int ready_for_output(const dpx_batch *b) {
    if (!b->store) return DPX_ERR_NO_MATRIX;
    if (!b->filled) return DPX_ERR_NOT_FILLED;
    return bind_device(b->device);
}

/* stage 1, asynchronous on the batch's stream: kernels + D2H of the offsets / lengths */

static int output_begin(dpx_batch *b, uint64_t firstNumber) {
    PhaseTrace trace;
    const size_t np = b->numPairs;
    if (b->outState == 2 && b->outFirst == firstNumber) return DPX_OK; /* already on the host */
    if (b->outState == 1 && b->outFirst == firstNumber) return DPX_OK; /* already in flight */
    if (b->outState == 1) HIP_TRY(hipStreamSynchronize(b->stream));    /* a run with another numbering is in flight: let it finish */
    if (!b->dTb || !b->dOut || !b->hMeta) { /* buffers of the output path, on first use (a failed attempt is simply repeated) */
        const uint64_t lines = b->tbOff[np];
        HIP_TRY(b->dTb.ensure((size_t)std::max<uint64_t>(lines, 16)));
        /* packed text, worst case: every alignment m + n long, 20 digits of pair number, 11 of score */
        HIP_TRY(b->dOut.ensure((size_t)(lines + 40ull * np + 16)));
        HIP_TRY(b->hMeta.ensure((np + 1) * sizeof(uint64_t) + np * sizeof(int32_t) + 16 + kSmallResultBytes));
        trace.mark("output: buffers");
    }
    uint64_t *hOff = reinterpret_cast<uint64_t *>(b->hMeta.get());
    int32_t *hLen = reinterpret_cast<int32_t *>(hOff + np + 1);
    const bool timeOut = (b->flags & DPX_TIME_FILLS) != 0;
    if (timeOut) {
        if (!b->evOut0) HIP_TRY(hipEventCreate(&b->evOut0));
        if (!b->evOut1) HIP_TRY(hipEventCreate(&b->evOut1));
    }
    { const int rc = lines_behind_fill(b, timeOut ? b->evOut0 : nullptr); if (rc != DPX_OK) return rc; }
    HIP_TRY(dpx_launch_output(b->dPairs, b->dScore, b->dTbLen, b->dTbOff, b->dTb.get(), (int)np, (unsigned long long)firstNumber,
                              reinterpret_cast<unsigned long long *>(b->dOutScratch), reinterpret_cast<unsigned long long *>(b->dOutOff), b->dOut.get(),
                              false, false, b->stream));
    if (timeOut) { HIP_TRY(hipEventRecord(b->evOut1, b->stream)); b->outTimed = true; }
    b->textCopied = false;
    b->resultsCopied = false;
    if (np) {
        HIP_TRY(hipMemcpyAsync(hOff, b->dOutOff, (np + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipMemcpyAsync(hLen, b->dTbLen, np * sizeof(int32_t), hipMemcpyDeviceToHost, b->stream));
        /* small batches: the text follows at once, at its worst-case size -- dpx_batch_output_end() then waits once instead of waiting,
         * reading the real size and copying (a second round trip of ~15 us; the class-per-pair drivers pay it 200 times per 4000 pairs) */
        const size_t worst = (size_t)(b->tbOff[np] + 40ull * np + 16);
        if (worst <= ((size_t)256 << 10)) {
            HIP_TRY(b->hOut.grow(worst + 1));
            HIP_TRY(hipMemcpyAsync(b->hOut.get(), b->dOut.get(), worst, hipMemcpyDeviceToHost, b->stream));
            b->textCopied = true;
            /* ... and so do score / end row / end column (they lie side by side in the arena): dpx_batch_results() after this call is a
             * wait and three memcpy instead of a wait and a synchronous copy of its own */
            const size_t stride = (size_t)((const char *)b->dEndRow - (const char *)b->dScore), bytes = np * sizeof(int32_t);
            if ((const char *)b->dEndCol - (const char *)b->dEndRow == (ptrdiff_t)stride && 2 * stride + bytes <= kSmallResultBytes &&
                (!b->lastStream || b->lastStream == b->stream)) {
                char *tail = b->hMeta.get() + (np + 1) * sizeof(uint64_t) + np * sizeof(int32_t) + 16;
                HIP_TRY(hipMemcpyAsync(tail, b->dScore, 2 * stride + bytes, hipMemcpyDeviceToHost, b->stream));
                b->resultsCopied = true;
            }
        }
    } else {
        hOff[0] = 0;
    }
    b->outState = 1;
    b->outFirst = firstNumber;
    trace.mark("output: launches");
    return DPX_OK;
}

/* stage 2: wait, then copy exactly the bytes the blocks occupy */
static int output_end(dpx_batch *b) {
    if (b->outState == 2) return DPX_OK;
    if (b->outState != 1) return DPX_ERR_INVALID;
    PhaseTrace trace;
    HIP_TRY(hipStreamSynchronize(b->stream));
    trace.mark("output: wait for device");
    const uint64_t total = reinterpret_cast<const uint64_t *>(b->hMeta.get())[b->numPairs];
    if (b->textCopied) { /* (the text came with the offsets) */
        b->hOut.get()[total] = 0;
        b->hOutBytes = (size_t)total;
        b->outState = 2;
        trace.mark("output: D2H text");
        return DPX_OK;
    }
    if (b->hOut.cap() < total + 1) {
        HIP_TRY(b->hOut.grow((size_t)total + 1));
        trace.mark("output: pinned text buffer");
    }
    if (total) {
        HIP_TRY(hipMemcpyAsync(b->hOut.get(), b->dOut.get(), (size_t)total, hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));
    }
    b->hOut.get()[total] = 0;
    b->hOutBytes = (size_t)total;
    b->outState = 2;
    trace.mark("output: D2H text");
    return DPX_OK;
}

int dpx_batch_output_begin(dpx_batch *b, uint64_t firstPairNumber) {
    if (!b) return DPX_ERR_INVALID;
    int rc = ready_for_output(b);
    if (rc != DPX_OK) return rc;
    return output_begin(b, firstPairNumber);
}

int dpx_batch_output_end(dpx_batch *b, const char **text, size_t *bytes, const uint64_t **offsets) {
    if (!b) return DPX_ERR_INVALID;
    if (b->outState == 0) return DPX_ERR_NOT_FILLED; /* no dpx_batch_output_begin() since the last fill */
    int rc = bind_device(b->device);
    if (rc != DPX_OK) return rc;
    rc = output_end(b);
    if (rc != DPX_OK) return rc;
    if (text) *text = b->hOut.get();
    if (bytes) *bytes = b->hOutBytes;
    if (offsets) *offsets = reinterpret_cast<const uint64_t *>(b->hMeta.get());
    return DPX_OK;
}

/* pinned text buffers handed to the caller by dpx_batch_output_take(): pointer -> capacity, for dpx_text_free() */
namespace { struct Taken { void *ptr; size_t cap; int device; }; std::mutex g_takenMu; std::vector<Taken> g_taken; }

int dpx_batch_output_take(dpx_batch *b, char **text, size_t *bytes) {
    if (!b || !text) return DPX_ERR_INVALID;
    if (b->outState == 0) return DPX_ERR_NOT_FILLED;
    int rc = bind_device(b->device);
    if (rc != DPX_OK) return rc;
    rc = output_end(b);
    if (rc != DPX_OK) return rc;
    size_t cap = 0;
    *text = b->hOut.release(&cap); /* the batch no longer owns it; a later dpx_batch_traceback() / _output_end() rebuilds the text */
    { std::lock_guard<std::mutex> lk(g_takenMu); g_taken.push_back(Taken{(void *)*text, cap, b->device}); }
    if (bytes) *bytes = b->hOutBytes;
    b->outState = 0;
    return DPX_OK;
}

int dpx_text_free(char *text) {
    if (!text) return DPX_OK;
    size_t cap = 0;
    int dev = -1;
    {
        std::lock_guard<std::mutex> lk(g_takenMu);
        for (size_t i = 0; i < g_taken.size(); i++)
            if (g_taken[i].ptr == (void *)text) { cap = g_taken[i].cap; dev = g_taken[i].device; g_taken.erase(g_taken.begin() + (long)i); break; }
    }
    if (!cap) return DPX_ERR_INVALID; /* not a buffer dpx_batch_output_take() handed out */
    if (dev >= 0) { (void)hipSetDevice(dev); t_device = dev; }
    g_tbHostCache.park(text, cap);
    return DPX_OK;
}

int dpx_batch_traceback(dpx_batch *b, size_t pair, char *refLine, char *relLine, char *qryLine, int32_t *len) {
    if (!b || pair >= b->numPairs) return DPX_ERR_INVALID;
    if (!b->store) return DPX_ERR_NO_MATRIX;
    if (!b->filled) return DPX_ERR_NOT_FILLED;
    if (b->outState != 2) { /* first call after a fill walks every pair of the batch on the device; later calls only copy lines */
        int rc = bind_device(b->device);
        if (rc != DPX_OK) return rc;
        rc = output_begin(b, b->outState == 1 ? b->outFirst : 0);
        if (rc == DPX_OK) rc = output_end(b);
        if (rc != DPX_OK) return rc;
    }
    const uint64_t *hOff = reinterpret_cast<const uint64_t *>(b->hMeta.get());
    const int32_t *hLen = reinterpret_cast<const int32_t *>(hOff + b->numPairs + 1);
    const int k = hLen[pair];
    /* the pair's block ends with its three lines, each k characters + '\n' */
    const char *lines = b->hOut.get() + hOff[pair + 1] - 3 * (size_t)(k + 1);
    char *dst[3] = {refLine, relLine, qryLine};
    for (int l = 0; l < 3; l++)
        if (dst[l]) { memcpy(dst[l], lines + (size_t)l * (size_t)(k + 1), (size_t)k); dst[l][k] = 0; }
    if (len) *len = k;
    return DPX_OK;
}

/* ---- CIGARs: the same traceback lines, run-length encoded on the device (dpx_cigar_kernels.hip) -> D2H of one record per pair,
 * then of exactly the ops.  Buffers of its own, so the text pipeline and this one may follow the same fill in either order. */

int dpx_batch_cigars_begin(dpx_batch *b, unsigned flags) {
    if (!b || (flags & ~DPX_CIGAR_M) != 0) return DPX_ERR_INVALID;
    int rc = ready_for_output(b);
    if (rc != DPX_OK) return rc;
    const size_t np = b->numPairs, recBytes = np * sizeof(dpx_alignment);
    const uint64_t lines = b->tbOff[np];
    /* buffers, on first use (a failed attempt is simply repeated); ops, worst case: one per column of every line capacity */
    HIP_TRY(b->dTb.ensure((size_t)std::max<uint64_t>(lines, 16)));
    HIP_TRY(b->dCigar.ensure(recBytes + (1 + dpx_cigar_scan_tiles(np)) * sizeof(uint64_t) + 16));
    HIP_TRY(b->dCigarOps.ensure((size_t)(lines / 3) * sizeof(uint32_t) + 16));
    HIP_TRY(b->hCigar.ensure(recBytes + sizeof(uint64_t) + 16));
    unsigned long long *dTotal = reinterpret_cast<unsigned long long *>(b->dCigar.get() + recBytes); /* (48 bytes per record: 8-byte aligned) */
    if (np) {
        rc = lines_behind_fill(b);
        if (rc != DPX_OK) return rc;
        HIP_TRY(dpx_launch_cigars(b->dPairs, b->dEndRow, b->dEndCol, b->dTbLen, b->dTbOff, b->dTb.get(), (int)np, flags,
                                  reinterpret_cast<dpx_alignment *>(b->dCigar.get()), dTotal + 1, dTotal, b->dCigarOps.get(), b->stream));
        if (b->revCount) HIP_TRY(dpx_launch_map_records(b->dPairs, b->dFlagged, (int)b->revCount, reinterpret_cast<dpx_alignment *>(b->dCigar.get()), b->stream));
        HIP_TRY(hipMemcpyAsync(b->hCigar.get(), b->dCigar.get(), recBytes + sizeof(uint64_t), hipMemcpyDeviceToHost, b->stream));
    } else {
        memset(b->hCigar.get(), 0, sizeof(uint64_t)); /* a batch without pairs: no records, no ops */
    }
    b->cigarFlags = flags;
    b->cigarState = 1;
    return DPX_OK;
}

int dpx_batch_cigars_end(dpx_batch *b, const dpx_alignment **records, const uint32_t **ops, uint64_t *numOps) {
    if (!b) return DPX_ERR_INVALID;
    if (b->cigarState == 0) return DPX_ERR_NOT_FILLED; /* no dpx_batch_cigars_begin() since the last fill */
    int rc = bind_device(b->device);
    if (rc != DPX_OK) return rc;
    if (b->cigarState == 1) {
        HIP_TRY(hipStreamSynchronize(b->stream));
        uint64_t total = 0;
        memcpy(&total, b->hCigar.get() + b->numPairs * sizeof(dpx_alignment), sizeof total);
        const size_t bytes = (size_t)total * sizeof(uint32_t);
        HIP_TRY(b->hCigarOps.grow(bytes + 16));
        if (bytes) {
            HIP_TRY(hipMemcpyAsync(b->hCigarOps.get(), b->dCigarOps.get(), bytes, hipMemcpyDeviceToHost, b->stream));
            HIP_TRY(hipStreamSynchronize(b->stream));
        }
        b->cigarOps = total;
        b->cigarState = 2;
    }
    if (records) *records = reinterpret_cast<const dpx_alignment *>(b->hCigar.get());
    if (ops) *ops = b->hCigarOps.get();
    if (numOps) *numOps = b->cigarOps;
    return DPX_OK;
}

/* ---- difference strings: the same traceback lines once more, as MD or cs text per pair (dpx_diff_kernels.hip) -> D2H of the
 * numPairs + 1 offsets, then of exactly the bytes.  Buffers of their own per kind, so text, CIGARs and these may follow the same fill
 * in any order. */

int dpx_batch_diffs_begin(dpx_batch *b, unsigned kinds) {
    if (!b || kinds == 0 || (kinds & ~(DPX_DIFF_MD | DPX_DIFF_CS)) != 0) return DPX_ERR_INVALID;
    int rc = ready_for_output(b);
    if (rc != DPX_OK) return rc;
    const size_t np = b->numPairs, offBytes = (np + 1) * sizeof(uint64_t);
    const uint64_t lines = b->tbOff[np];
    HIP_TRY(b->dTb.ensure((size_t)std::max<uint64_t>(lines, 16)));
    if (np) {
        rc = lines_behind_fill(b);
        if (rc != DPX_OK) return rc;
    }
    for (int k = 0; k < 2; k++) {
        const unsigned kind = k == 0 ? DPX_DIFF_MD : DPX_DIFF_CS;
        if (!(kinds & kind)) continue;
        /* buffers, on first use (a failed attempt is simply repeated); text, worst case: three bytes per column of every line capacity */
        HIP_TRY(b->dDiffOff[k].ensure(offBytes + dpx_diff_scan_tiles(np) * sizeof(uint64_t) + 16));
        HIP_TRY(b->dDiffText[k].ensure((size_t)lines + 16));
        HIP_TRY(b->hDiffOff[k].ensure(offBytes + 16));
        if (np) {
            unsigned long long *dOff = reinterpret_cast<unsigned long long *>(b->dDiffOff[k].get());
            HIP_TRY(dpx_launch_diffs(kind, b->dPairs, b->dTbLen, b->dTbOff, b->dTb.get(), (int)np, dOff, dOff + np + 1, b->dDiffText[k].get(), b->stream));
            HIP_TRY(hipMemcpyAsync(b->hDiffOff[k].get(), b->dDiffOff[k].get(), offBytes, hipMemcpyDeviceToHost, b->stream));
        } else {
            memset(b->hDiffOff[k].get(), 0, sizeof(uint64_t)); /* a batch without pairs: one offset of 0, no bytes */
        }
        b->diffState[k] = 1;
    }
    return DPX_OK;
}

int dpx_batch_diffs_end(dpx_batch *b, unsigned kind, const char **text, size_t *bytes, const uint64_t **offsets) {
    if (!b || (kind != DPX_DIFF_MD && kind != DPX_DIFF_CS)) return DPX_ERR_INVALID;
    const int k = kind == DPX_DIFF_MD ? 0 : 1;
    if (b->diffState[k] == 0) return DPX_ERR_NOT_FILLED; /* no dpx_batch_diffs_begin() of this kind since the last fill */
    int rc = bind_device(b->device);
    if (rc != DPX_OK) return rc;
    const uint64_t *hOff = reinterpret_cast<const uint64_t *>(b->hDiffOff[k].get());
    if (b->diffState[k] == 1) {
        HIP_TRY(hipStreamSynchronize(b->stream));
        const size_t total = (size_t)hOff[b->numPairs];
        HIP_TRY(b->hDiffText[k].grow(total + 1 + 16));
        if (total) {
            HIP_TRY(hipMemcpyAsync(b->hDiffText[k].get(), b->dDiffText[k].get(), total, hipMemcpyDeviceToHost, b->stream));
            HIP_TRY(hipStreamSynchronize(b->stream));
        }
        b->hDiffText[k].get()[total] = 0;
        b->diffState[k] = 2;
    }
    if (text) *text = b->hDiffText[k].get();
    if (bytes) *bytes = (size_t)hOff[b->numPairs];
    if (offsets) *offsets = hOff;
    return DPX_OK;
}

int dpx_cigar_text(const uint32_t *ops, size_t numOps, char *out, size_t cap, size_t *len) {
    if ((!ops && numOps) || (!out && cap)) return DPX_ERR_INVALID;
    static const char letters[] = "MID....=X"; /* BAM's numbering; 3..6 (N S H P) never come out of the engine */
    size_t need = numOps ? 0 : 1; /* "*" */
    for (size_t k = 0; k < numOps; k++) {
        const uint32_t code = ops[k] & 0xFu;
        if (code > 8u || letters[code] == '.') return DPX_ERR_INVALID;
        uint32_t v = ops[k] >> 4;
        do { need++; v /= 10u; } while (v);
        need++;
    }
    if (len) *len = need;
    if (cap < need + 1) return DPX_ERR_INVALID;
    char *q = out;
    if (!numOps) *q++ = '*';
    for (size_t k = 0; k < numOps; k++) {
        char digits[10];
        int d = 0;
        uint32_t v = ops[k] >> 4;
        do { digits[d++] = (char)('0' + (int)(v % 10u)); v /= 10u; } while (v);
        while (d) *q++ = digits[--d];
        *q++ = letters[ops[k] & 0xFu];
    }
    *q = 0;
    return DPX_OK;
}

} /* extern "C" */
