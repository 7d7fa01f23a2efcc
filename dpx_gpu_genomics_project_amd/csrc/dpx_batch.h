/* dpx_batch.h -- struct dpx_batch and what more than one host unit of libdpxalign.so does with it (dpx_capi.cpp: create, fill, results,
 * destroy; dpx_settings.cpp: the setters; dpx_output.cpp: text, CIGARs, difference strings). */
#ifndef DPX_BATCH_H
#define DPX_BATCH_H

#include <vector>

#include "dpx_mem.h"

#pragma GCC visibility push(hidden) /* (internal to libdpxalign.so: not part of its ABI) */
using namespace dpx_host; /* (an internal header: whoever includes it is a host unit of the library) */

constexpr size_t kSmallResultBytes = 12288; /* score / end row / end column of a small batch, as they lie in the arena (dpx_batch_output_begin) */

/* Every buffer the batch owns is a Buf on the cache it comes from: taken at first use, parked by ~dpx_batch (dpx_batch_destroy
 * binds the device and waits for the streams first). */
/* A batch is its plan (dpx_plan.h: what was decided, the pair table, the launch arguments) plus everything that lives on the device. */
struct dpx_batch : dpx_plan {
    int device = -1; /* the device the batch lives on */
    bool filled = false;
    size_t guardBytes = 0;   /* DPX_POOL_GUARD: pattern bytes behind the matrices, checked by dpx_batch_sync() */
    bool guardSelfTest = false;
    char *dSeq = nullptr;
    dpx_pair_dev *dPairs = nullptr;
    int32_t *dOrder = nullptr;
    Buf<char> arena{g_arenaCache}; /* one device allocation behind dSeq, dPairs, dScore/dEndRow/dEndCol, dOrder, dCouples, dTbOff, dTbLen
                                (parked and reused across batches like the matrix pool: 9 hipMalloc/hipFree pairs per batch otherwise) */
    Buf<int16_t> dMat{g_matCache}; /* the matrix pool (cap() may exceed matElems*2 when a parked pool was reused) */
    int32_t *dScore = nullptr, *dEndRow = nullptr, *dEndCol = nullptr;
    hipStream_t stream = nullptr;     /* the batch's own stream */
    hipStream_t sideStream = nullptr; /* secondary kernels of a fill run here, concurrently with the main one (launch_all) */
    hipEvent_t evFork = nullptr, evJoin = nullptr;
    hipEvent_t evT0 = nullptr, evT1 = nullptr; /* DPX_TIME_FILLS: recorded around every dpx_batch_fill() */
    hipEvent_t evOrder = nullptr;              /* orders the output path behind a fill that ran on a caller's stream */
    hipEvent_t evOut0 = nullptr, evOut1 = nullptr; /* DPX_TIME_FILLS: around the traceback + text kernels of dpx_batch_output_begin() */
    bool outTimed = false;
    bool fillTimed = false;
    hipStream_t lastStream = nullptr; /* stream of the most recent fill (caller's or own) */
    int32_t *dCouples = nullptr; /* the couples of the packed kernels, or the wave descriptors of the lane-packed ones */
    /* result text (lazy): device line buffers of k_traceback, the packed blocks built from them, pinned host mirrors */
    uint64_t *dTbOff = nullptr;
    Buf<char> dTb{g_tbDevCache};
    int32_t *dTbLen = nullptr;
    uint64_t *dOutOff = nullptr, *dOutScratch = nullptr; /* per-pair byte offsets of the blocks (+ total), scan scratch */
    Buf<char> dOut{g_tbDevCache};
    Buf<char> hStage{g_stageCache}; /* pinned image of the arena's uploaded front (small batches), alive until the batch is destroyed */
    bool resultsCopied = false; /* ... and of score / end row / end column, into the tail of hMeta */
    bool textCopied = false;    /* dpx_batch_output_begin() has queued the text's D2H itself (small batches) */
    bool uploadPending = false; /* ... and its one asynchronous H2D on b->stream has not been waited for by anybody yet */
    Buf<char> hMeta{g_tbHostCache}; /* pinned: uint64 offsets[numPairs + 1], then int32 alignment lengths[numPairs] */
    Buf<char> hOut{g_tbHostCache};  /* pinned: the packed text */
    size_t hOutBytes = 0;
    bool tbLinesValid = false; /* k_traceback has run since the last fill */
    int outState = 0;          /* 0 none, 1 dpx_batch_output_begin() in flight, 2 text on the host */
    uint64_t outFirst = 0;     /* pair number of the batch's first pair in the text */
    /* CIGARs (dpx_batch_cigars_begin / _end): built from the same traceback lines as the text, with buffers of their own so that the
     * two output paths may follow one fill in either order */
    int cigarState = 0;        /* 0 none, 1 dpx_batch_cigars_begin() in flight, 2 records and ops on the host */
    unsigned cigarFlags = 0;
    Buf<char> dCigar{g_tbDevCache};    /* device: dpx_alignment[numPairs], uint64 total, uint64 tile sums of the scan */
    Buf<uint32_t> dCigarOps{g_tbDevCache}; /* device: one op per column at worst */
    Buf<char> hCigar{g_tbHostCache};    /* pinned: dpx_alignment[numPairs], uint64 total */
    Buf<uint32_t> hCigarOps{g_tbHostCache}; /* pinned: exactly the ops */
    uint64_t cigarOps = 0;     /* total number of ops (state 2) */
    /* difference strings (dpx_batch_diffs_begin / _end), index 0: MD, 1: cs -- from the same lines again, with buffers of their own per kind */
    int diffState[2] = {0, 0};             /* 0 none, 1 dpx_batch_diffs_begin() in flight, 2 text on the host */
    Buf<char> dDiffOff[2] = {Buf<char>(g_tbDevCache), Buf<char>(g_tbDevCache)};  /* device: uint64 offsets[numPairs + 1], uint64 tile sums of the scan */
    Buf<char> dDiffText[2] = {Buf<char>(g_tbDevCache), Buf<char>(g_tbDevCache)}; /* device: the size of the line buffer (three times the line capacity per pair at worst) */
    Buf<char> hDiffOff[2] = {Buf<char>(g_tbHostCache), Buf<char>(g_tbHostCache)};  /* pinned: uint64 offsets[numPairs + 1] */
    Buf<char> hDiffText[2] = {Buf<char>(g_tbHostCache), Buf<char>(g_tbHostCache)}; /* pinned: exactly the strings and one NUL */
    /* BAXT's extension mode (dpx_batch_set_extension): the next fill runs k_zext_fill while either value is >= 0 */
    int32_t zdrop = -1, endBonus = -1;
    bool extFilled = false;    /* the last fill ran the extension scan (k_zext_fill, k_zsub_fill, k_bdx_fill with zdrop or endBonus on): dExt holds its
                                  records, and dpx_batch_matrix / dpx_batch_directions mask behind lastDiag */
    Buf<int32_t> dExt{g_tbDevCache};   /* device: dpx_extension[numPairs] */
    /* substitution table (dpx_batch_set_substitution): while substAlphabet > 0 the fills run k_subst_fill and the walks k_subst_traceback*
     * (band-direction batches: k_bdx_fill; local band-direction batches, dpx_batch_set_local_direction_table: k_bdlt_fill, the walk stays; ANW / ASW / ASG direction batches, dpx_batch_set_direction_table: k_dirtab_fill, the walk stays;
     * their score-only batches, dpx_batch_set_score_table: k_scoretab_fill / k_scoretab_lanes) */
    int substAlphabet = 0;
    Buf<unsigned char> dSubst{g_tbDevCache}; /* device: the table at row stride 32 (DPX_SUBST_TABLE_BYTES), then codeOf[256] */
    std::vector<unsigned char> tableImage; /* the image dSubst holds while substAlphabet != 0 (every table setter keeps it, every clear drops it) */
    /* orientation (dpx_batch_set_reversed): while revCount > 0 dSeq points at dRev, the setter's own allocation -- [the arena's sequence
     * bytes][reversed copies of the flagged pairs' strings][the kernel's job list][the flagged pairs' numbers] -- and the flagged pairs'
     * indices in `pairs` / dPairs at the copies.  The fills, walks and exports know nothing of it. */
    char *dSeqOwn = nullptr;     /* the arena's sequence bytes (== dSeq while no mask is set) */
    size_t seqBytes = 0;         /* ... and their padded size */
    Buf<char> dRev{g_arenaCache};
    const int32_t *dFlagged = nullptr; /* inside dRev: revCount pair numbers, ascending */
    size_t revCount = 0;
    struct RevSaved { int32_t pair, refIdx, qryIdx; };
    std::vector<RevSaved> revSaved;    /* the flagged pairs' own indices, for the next call of the setter */
    PoolRecord poolRec;    /* how the matrix pool behind dMat was built / timed */
    bool tunePool = false, tuneShop = false; /* DPX_TUNE_PLACEMENT: the pool is timed / shopped for at the end of dpx_batch_create */
};

inline bool extension_on(const dpx_batch *b) { return b->zdrop >= 0 || b->endBonus >= 0; }

/* which kernels the batch runs under its present settings (dpx_plan.h: computed at every use, never kept) */
inline dpx_route route_of(const dpx_batch *b) { return dpx_plan_route(*b, knobs().tbWalk, b->zdrop, b->endBonus, b->substAlphabet); }

/* what a refill does to lines, text and CIGARs; the results go with them until the next fill */
inline void invalidate_fill(dpx_batch *b) {
    b->filled = false; b->extFilled = false; b->tbLinesValid = false; b->outState = 0; b->cigarState = 0; b->diffState[0] = b->diffState[1] = 0;
}
/* ... and that next fill, queued on `s` along route `r` */
inline void mark_filled(dpx_batch *b, const dpx_route &r, hipStream_t s) {
    invalidate_fill(b);
    b->filled = true; b->extFilled = r.extRecords; b->lastStream = s;
}

/* the batch's table on the device (dpx_kernels.h: the map behind the table, one allocation) */
inline dpx_table_ref table_ref(const dpx_batch *b) { return {reinterpret_cast<const int8_t *>(b->dSubst.get()), b->dSubst.get() + DPX_SUBST_TABLE_BYTES}; }

/* the batch's launch arguments under its substitution table: every wave's LDS slice grows by the table image */
inline dpx_subst_args subst_args(const dpx_batch *b) {
    dpx_subst_args sa = {b->args, table_ref(b)};
    sa.f.ldsPerWave += DPX_SUBST_IMAGE_BYTES;
    return sa;
}
inline size_t subst_lds_bytes(const dpx_batch *b) { return b->ldsBytes + (size_t)DPX_SUBST_IMAGE_BYTES * (DPX_FILL_THREADS / 64); }

/* the last fill ran on a caller's stream: the host waits for it here (the batch's own stream is waited for by whoever needs that too) */
inline hipError_t wait_for_fill(const dpx_batch *b) {
    return b->lastStream && b->lastStream != b->stream ? hipStreamSynchronize(b->lastStream) : hipSuccess;
}

#pragma GCC visibility pop
#endif
