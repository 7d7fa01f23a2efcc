/* dpx_settings.cpp -- what a batch can change after its creation: the dpx_batch_set_* entry points of include/dpx_align.h (host side of
 * libdpxalign.so).  Every setter makes all of its checks before its first change. */
#include <algorithm>
#include <cstring>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "dpx_batch.h"
#include "dpx_reverse.h"

extern "C" {

/* ---- substitution tables and BAXT's extension mode: what the setters below share ----
 * One copy of every check and of every step that changes the batch.  A setter is its own admission rule, the shared checks in its
 * documented order, then ensure_ext_records / install_table / clear_table: every check comes before the first change. */
static bool ext_bounds_ok(int32_t zdrop, int32_t endBonus) { return zdrop >= -1 && zdrop <= (1 << 30) && endBonus >= -1 && endBonus <= (1 << 30); }
static bool table_args_ok(int32_t alphabet, const uint8_t *codeOf) {
    if (alphabet < 1 || alphabet > 32 || !codeOf) return false;
    for (int x = 0; x < 256; x++) if ((int)codeOf[x] >= alphabet) return false;
    return true;
}
/* the batch's parameters with the table's largest entry in place of match and its smallest in place of mismatch; `entries` is the
 * caller's array (stride = alphabet) or the host image (stride 32) */
static dpx_params table_extremes(const dpx_batch *b, const void *entries, int32_t alphabet, int32_t stride) {
    dpx_params q = b->prm;
    q.match = -128; q.mismatch = 127;
    for (int r = 0; r < alphabet; r++)
        for (int c = 0; c < alphabet; c++) {
            const int32_t v = static_cast<const int8_t *>(entries)[r * stride + c];
            q.match = std::max(q.match, v); q.mismatch = std::min(q.mismatch, v);
        }
    return q;
}
/* the range check of the batch's storage mode (`fits`: fits_int16, fits_dir or a two-piece wrapper of it) over every pair */
static bool pairs_in_range(const dpx_batch *b, const dpx_params &q, const std::function<bool(const dpx_params &, long long, long long)> &fits) {
    for (const dpx_pair_dev &pd : b->pairs) if (!fits(q, pd.m, pd.n)) return false;
    return true;
}
/* fits_dir for a band-direction batch under two gap pieces: on their componentwise minimum and again on their componentwise maximum,
 * valid lower and upper bounds of every cell (equal pieces: fits_dir itself) */
static bool fits_dir_pieces(dpx_params q, int32_t o2, int32_t e2, long long m, long long n) {
    const int32_t o1 = q.gapOpen, e1 = q.gapExtend;
    q.gapOpen = std::min(o1, o2); q.gapExtend = std::min(e1, e2);
    if (!fits_dir(q, m, n)) return false;
    q.gapOpen = std::max(o1, o2); q.gapExtend = std::max(e1, e2);
    return fits_dir(q, m, n);
}
/* the image of dpx_kernels.h: rows of 32, the 256-byte map behind them */
static void build_table_image(unsigned char (&image)[DPX_SUBST_IMAGE_BYTES], const int8_t *scores, int32_t alphabet, const uint8_t *codeOf) {
    memset(image, 0, sizeof image);
    for (int r = 0; r < alphabet; r++) memcpy(image + r * 32, scores + r * alphabet, (size_t)alphabet);
    memcpy(image + DPX_SUBST_TABLE_BYTES, codeOf, 256);
}
/* the batch's device is bound and, with the scan on, its per-pair records exist */
static int ensure_ext_records(dpx_batch *b, bool scan) {
    int rc = bind_device(b->device);
    if (rc != DPX_OK) return rc;
    if (scan && b->numPairs) HIP_TRY(b->dExt.ensure(b->numPairs * sizeof(dpx_extension)));
    return DPX_OK;
}
/* the checked table becomes the batch's, on the device and -- to tell a changed table from the same one, and for
 * dpx_batch_set_second_gap's range check -- on the host.  keepIfSame: the same table again invalidates nothing. */
static int install_table(dpx_batch *b, const unsigned char (&image)[DPX_SUBST_IMAGE_BYTES], int32_t alphabet, bool keepIfSame) {
    if (keepIfSame && b->substAlphabet == alphabet && !memcmp(b->tableImage.data(), image, sizeof image)) return DPX_OK;
    int rc = bind_device(b->device);
    if (rc != DPX_OK) return rc;
    HIP_TRY(b->dSubst.ensure(sizeof image));
    /* a fill or a walk in flight may still read the previous table */
    HIP_TRY(wait_for_fill(b));
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipMemcpy(b->dSubst.get(), image, sizeof image, hipMemcpyHostToDevice));
    b->tableImage.assign(image, image + sizeof image);
    b->substAlphabet = alphabet;
    invalidate_fill(b);
    return DPX_OK;
}
/* scores == NULL: whatever table the batch holds goes, through whichever setter it came (legal on every batch); the batch runs its
 * plain kernels again */
static int clear_table(dpx_batch *b) {
    if (b->substAlphabet) invalidate_fill(b);
    b->substAlphabet = 0;
    b->tableImage.clear();
    return DPX_OK;
}

int dpx_batch_set_extension(dpx_batch *b, int32_t zdrop, int32_t endBonus) {
    if (!b || !ext_bounds_ok(zdrop, endBonus)) return DPX_ERR_INVALID;
    if (b->prm.algo != DPX_ALGO_BAXT) return DPX_ERR_UNSUPPORTED;
    if (b->bandDirs) return DPX_ERR_UNSUPPORTED; /* refused by design (tests pin it): dpx_batch_set_direction_scoring is a band-direction batch's setter */
    if ((zdrop >= 0 || endBonus >= 0) && b->substAlphabet) return DPX_ERR_UNSUPPORTED; /* (the two go together through dpx_batch_set_extension_table only) */
    int rc = ensure_ext_records(b, zdrop >= 0 || endBonus >= 0);
    if (rc != DPX_OK) return rc;
    b->zdrop = zdrop;
    b->endBonus = endBonus;
    return DPX_OK;
}

/* dpx_batch_set_substitution's and dpx_batch_set_extension_table's batches: BANW / BAXT with matrices or score-only.  Band directions are
 * refused by design (dpx_batch_set_direction_scoring is their setter); a covering BANW band runs as ANW, which has no table kernel */
static bool admits_band_table(const dpx_batch *b) {
    return (b->prm.algo == DPX_ALGO_BANW || b->prm.algo == DPX_ALGO_BAXT) && b->kernelAlgo == b->prm.algo && !b->dirs && !b->bandDirs;
}
/* ... and what both check behind it: the image fits beside the staged strings, and fits_int16's BANW / BAXT bounds hold under the table */
static int check_band_table_fit(const dpx_batch *b, const int8_t *scores, int32_t alphabet) {
    if (subst_lds_bytes(b) > 160u * 1024u) return DPX_ERR_UNSUPPORTED;
    return pairs_in_range(b, table_extremes(b, scores, alphabet, alphabet), fits_int16) ? DPX_OK : DPX_ERR_RANGE;
}

int dpx_batch_set_substitution(dpx_batch *b, const int8_t *scores, int32_t alphabet, const uint8_t *codeOf) {
    if (!b) return DPX_ERR_INVALID;
    if (!scores) return clear_table(b);
    if (!table_args_ok(alphabet, codeOf)) return DPX_ERR_INVALID;
    if (!admits_band_table(b) || extension_on(b)) return DPX_ERR_UNSUPPORTED;
    int rc = check_band_table_fit(b, scores, alphabet);
    if (rc != DPX_OK) return rc;
    unsigned char image[DPX_SUBST_IMAGE_BYTES];
    build_table_image(image, scores, alphabet, codeOf);
    return install_table(b, image, alphabet, false);
}

/* both settings at once, the one way to have both */
int dpx_batch_set_extension_table(dpx_batch *b, int32_t zdrop, int32_t endBonus, const int8_t *scores, int32_t alphabet, const uint8_t *codeOf) {
    if (!b || !scores || !codeOf) return DPX_ERR_INVALID;
    if (!ext_bounds_ok(zdrop, endBonus) || (zdrop < 0 && endBonus < 0)) return DPX_ERR_INVALID;
    if (!table_args_ok(alphabet, codeOf)) return DPX_ERR_INVALID;
    if (!admits_band_table(b) || b->prm.algo != DPX_ALGO_BAXT) return DPX_ERR_UNSUPPORTED;
    int rc = check_band_table_fit(b, scores, alphabet);
    if (rc != DPX_OK) return rc;
    unsigned char image[DPX_SUBST_IMAGE_BYTES];
    build_table_image(image, scores, alphabet, codeOf);
    rc = ensure_ext_records(b, true);
    if (rc == DPX_OK) rc = install_table(b, image, alphabet, false);
    if (rc != DPX_OK) return rc;
    b->zdrop = zdrop;
    b->endBonus = endBonus;
    return DPX_OK;
}

/* the second gap piece of a two-piece batch (DPX_TWO_PIECE_GAPS on BANW / BAXT, DPX_LOCAL_TWO_PIECE_GAPS on BASW) */
int dpx_batch_set_second_gap(dpx_batch *b, int32_t gapOpen2, int32_t gapExtend2) {
    if (!b) return DPX_ERR_INVALID;
    if (!b->twoPiece) return DPX_ERR_UNSUPPORTED; /* (a batch created without a two-piece flag) */
    const int32_t lim = 1 << 20; /* validate_params' rule */
    if (gapOpen2 > lim || gapOpen2 < -lim || gapExtend2 > lim || gapExtend2 < -lim) return DPX_ERR_RANGE;
    /* under a table: its largest and smallest entries, as its setter checks */
    const dpx_params q = b->substAlphabet ? table_extremes(b, b->tableImage.data(), b->substAlphabet, 32) : b->prm;
    if (!pairs_in_range(b, q, [&](const dpx_params &qq, long long m, long long n) { return fits_dir_pieces(qq, gapOpen2, gapExtend2, m, n); })) return DPX_ERR_RANGE;
    if (gapOpen2 != b->gapOpen2 || gapExtend2 != b->gapExtend2) invalidate_fill(b);
    b->gapOpen2 = gapOpen2;
    b->gapExtend2 = gapExtend2;
    return DPX_OK;
}

/* all scoring of a band-direction batch, the three settings at once */
int dpx_batch_set_direction_scoring(dpx_batch *b, int32_t zdrop, int32_t endBonus, const int8_t *scores, int32_t alphabet, const uint8_t *codeOf) {
    if (!b || !ext_bounds_ok(zdrop, endBonus)) return DPX_ERR_INVALID;
    if (scores && !table_args_ok(alphabet, codeOf)) return DPX_ERR_INVALID;
    if (!b->bandDirs || b->bandLocal) return DPX_ERR_UNSUPPORTED; /* matrix and score-only batches, the other algorithms (BSW / BASW direction batches included), a covering BANW band (k_affine_dir) */
    const bool scan = zdrop >= 0 || endBonus >= 0;
    if (scan && b->prm.algo != DPX_ALGO_BAXT) return DPX_ERR_UNSUPPORTED;
    unsigned char image[DPX_SUBST_IMAGE_BYTES];
    if (scores) {
        if (!dpx_plan_bdx_waves(*b, true)) return DPX_ERR_UNSUPPORTED; /* one wave's staged strings leave no room in LDS for the table image */
        /* fits_dir under the table and the batch's gap pieces.  (With int8 entries and strings that fit LDS this can only refuse a batch
         * that its creation's own check admitted at its very limit.) */
        const int32_t o2 = b->twoPiece ? b->gapOpen2 : b->prm.gapOpen, e2 = b->twoPiece ? b->gapExtend2 : b->prm.gapExtend;
        if (!pairs_in_range(b, table_extremes(b, scores, alphabet, alphabet),
                            [&](const dpx_params &q, long long m, long long n) { return fits_dir_pieces(q, o2, e2, m, n); })) return DPX_ERR_RANGE;
        build_table_image(image, scores, alphabet, codeOf);
    }
    int rc = ensure_ext_records(b, scan);
    if (rc == DPX_OK) rc = scores ? install_table(b, image, alphabet, true) : clear_table(b);
    if (rc != DPX_OK) return rc;
    if (zdrop != b->zdrop || endBonus != b->endBonus) invalidate_fill(b);
    b->zdrop = zdrop;
    b->endBonus = endBonus;
    return DPX_OK;
}

/* dpx_batch_set_direction_table's and dpx_batch_set_score_table's algorithms: the batch's own, not the kernel's -- a covering BANW / BASW
 * band that runs the ANW / ASW kernels is not admitted */
static bool one_of_anw_asw_asg(const dpx_batch *b) { return b->prm.algo == DPX_ALGO_ANW || b->prm.algo == DPX_ALGO_ASW || b->prm.algo == DPX_ALGO_ASG; }

/* the table of an ANW / ASW / ASG direction batch (k_dirtab_fill) */
int dpx_batch_set_direction_table(dpx_batch *b, const int8_t *scores, int32_t alphabet, const uint8_t *codeOf) {
    if (!b) return DPX_ERR_INVALID;
    if (!scores) return clear_table(b);
    if (!table_args_ok(alphabet, codeOf)) return DPX_ERR_INVALID;
    if (!one_of_anw_asw_asg(b) || !b->dirs || !(b->flags & DPX_KEEP_DIRECTIONS)) return DPX_ERR_UNSUPPORTED;
    if (!pairs_in_range(b, table_extremes(b, scores, alphabet, alphabet), fits_dir)) return DPX_ERR_RANGE;
    unsigned char image[DPX_SUBST_IMAGE_BYTES];
    build_table_image(image, scores, alphabet, codeOf);
    return install_table(b, image, alphabet, true);
}

/* the table of an ANW / ASW / ASG score-only batch (k_scoretab_fill / k_scoretab_lanes) */
int dpx_batch_set_score_table(dpx_batch *b, const int8_t *scores, int32_t alphabet, const uint8_t *codeOf) {
    if (!b) return DPX_ERR_INVALID;
    if (!scores) return clear_table(b);
    if (!table_args_ok(alphabet, codeOf)) return DPX_ERR_INVALID;
    if (!one_of_anw_asw_asg(b) || b->store || b->dirs || !(b->flags & DPX_SCORE_ONLY)) return DPX_ERR_UNSUPPORTED;
    if (!dpx_plan_scoretab_fits(*b, t_err)) return DPX_ERR_UNSUPPORTED;
    if (!pairs_in_range(b, table_extremes(b, scores, alphabet, alphabet), fits_int16)) return DPX_ERR_RANGE;
    unsigned char image[DPX_SUBST_IMAGE_BYTES];
    build_table_image(image, scores, alphabet, codeOf);
    return install_table(b, image, alphabet, true);
}

/* the table of a BSW / BASW local band-direction batch (k_bdlt_fill; two pieces: k_lb2_fill, whose band never falls back); a covering band runs k_linear_dir / k_asw_dir and is not admitted */
int dpx_batch_set_local_direction_table(dpx_batch *b, const int8_t *scores, int32_t alphabet, const uint8_t *codeOf) {
    if (!b) return DPX_ERR_INVALID;
    if (!scores) return clear_table(b);
    if (!table_args_ok(alphabet, codeOf)) return DPX_ERR_INVALID;
    if (!b->bandLocal) return DPX_ERR_UNSUPPORTED;
    if (!dpx_plan_bdx_waves(*b, true)) return DPX_ERR_UNSUPPORTED; /* one wave's staged strings leave no room in LDS for the table image */
    /* fits_dir under the table and the batch's gap pieces (DPX_LOCAL_TWO_PIECE_GAPS; one piece: fits_dir itself) */
    const int32_t o2 = b->twoPiece ? b->gapOpen2 : b->prm.gapOpen, e2 = b->twoPiece ? b->gapExtend2 : b->prm.gapExtend;
    if (!pairs_in_range(b, table_extremes(b, scores, alphabet, alphabet),
                        [&](const dpx_params &q, long long m, long long n) { return fits_dir_pieces(q, o2, e2, m, n); })) return DPX_ERR_RANGE;
    unsigned char image[DPX_SUBST_IMAGE_BYTES];
    build_table_image(image, scores, alphabet, codeOf);
    return install_table(b, image, alphabet, true);
}

/* ---- orientation: dpx_batch_set_reversed ----
 * The kernels find a pair's strings through the pair table, so the setter builds reversed copies of the flagged pairs' strings on the
 * device (k_reverse_strings) behind a device copy of the batch's bytes, points the flagged pairs at them and the launch arguments'
 * `seq` at the new allocation.  Nothing is reversed in place (pairs share bytes), no sequence byte crosses PCIe and the host reads
 * none.  The plan is a function of sizes and stays. */
static void set_seq_pointer(dpx_batch *b, char *seq) {
    b->dSeq = seq;
    b->args.seq = seq;
    if (b->pkArgs.seq) b->pkArgs.seq = seq;
    if (b->dirs) b->dirArgs.seq = seq;
}

int dpx_batch_set_reversed(dpx_batch *b, const uint8_t *reversed) {
    if (!b) return DPX_ERR_INVALID;
    if (b->prm.algo != DPX_ALGO_BANW && b->prm.algo != DPX_ALGO_BAXT) return DPX_ERR_UNSUPPORTED;
    const size_t np = b->numPairs;
    std::vector<int32_t> flagged;
    for (size_t i = 0; reversed && i < np; i++) if (reversed[i]) flagged.push_back((int32_t)i);
    if (flagged.empty() && !b->revCount) return DPX_OK; /* no mask before, none now */
    PhaseTrace trace;
    /* the layout, from the pairs' own indices (a flagged pair's are in revSaved); every check comes before the first change */
    std::vector<dpx_pair_dev> table = b->pairs;
    for (const dpx_batch::RevSaved &sv : b->revSaved) { table[(size_t)sv.pair].refIdx = sv.refIdx; table[(size_t)sv.pair].qryIdx = sv.qryIdx; }
    std::vector<dpx_rev_job> jobs;
    std::vector<dpx_batch::RevSaved> saved;
    jobs.reserve(2 * flagged.size());
    saved.reserve(flagged.size());
    /* (index, length) -> the job that copies it: a string that many pairs share is copied once.  Open addressing, at most half full. */
    size_t slots = 16;
    while (slots < 4 * flagged.size()) slots <<= 1;
    std::vector<int32_t> jobOf(slots, -1);
    size_t off = b->seqBytes;
    for (const int32_t p : flagged) {
        dpx_pair_dev &pd = table[(size_t)p];
        saved.push_back({p, pd.refIdx, pd.qryIdx});
        for (int side = 0; side < 2; side++) {
            int32_t &idx = side ? pd.qryIdx : pd.refIdx;
            const int32_t len = side ? pd.m : pd.n;
            if (len <= 0) continue; /* (an empty string is never read: its index stays) */
            size_t h = (size_t)((((uint64_t)(uint32_t)idx << 32) | (uint32_t)len) * 0x9E3779B97F4A7C15ull >> 32) & (slots - 1);
            while (jobOf[h] >= 0 && (jobs[(size_t)jobOf[h]].src != idx || jobs[(size_t)jobOf[h]].len != len)) h = (h + 1) & (slots - 1);
            if (jobOf[h] < 0) {
                if (off + dpx_rev_slot_bytes((size_t)len) > (size_t)0x7fffffff) {
                    t_err = "dpx_batch_set_reversed: the reversed copies end beyond byte 2^31 of the sequence buffer (pair " + std::to_string(p) + "), int32 offsets cannot reach them";
                    return DPX_ERR_RANGE;
                }
                jobOf[h] = (int32_t)jobs.size();
                jobs.push_back({idx, (int32_t)off, len, 0});
                off += dpx_rev_slot_bytes((size_t)len);
            }
            idx = jobs[(size_t)jobOf[h]].dst;
        }
    }
    trace.mark("set_reversed: layout");
    const size_t jobsAt = align_up(off, 256), flaggedAt = jobsAt + align_up(jobs.size() * sizeof(dpx_rev_job), 256);
    const size_t need = flaggedAt + align_up(flagged.size() * sizeof(int32_t), 256);
    int rc = bind_device(b->device);
    if (rc != DPX_OK) return rc;
    /* a fill, a walk or an export in flight may still read the present strings and table */
    HIP_TRY(wait_for_fill(b));
    HIP_TRY(hipStreamSynchronize(b->stream));
    Buf<char> built(g_arenaCache); /* built aside: the batch keeps its present mask until every step has succeeded */
    char *fresh = nullptr;
    if (!flagged.empty()) {
        HIP_TRY(built.ensure(need));
        fresh = built.get();
        trace.mark("set_reversed: allocation");
        hipError_t e = hipMemcpyAsync(fresh, b->dSeqOwn, b->seqBytes, hipMemcpyDeviceToDevice, b->stream);
        if (e == hipSuccess && !jobs.empty()) e = hipMemcpy(fresh + jobsAt, jobs.data(), jobs.size() * sizeof(dpx_rev_job), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(fresh + flaggedAt, flagged.data(), flagged.size() * sizeof(int32_t), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = dpx_launch_reverse_strings(fresh, reinterpret_cast<const dpx_rev_job *>(fresh + jobsAt), (int)jobs.size(), b->stream);
        if (e == hipSuccess && np) e = hipMemcpy(b->dPairs, table.data(), np * sizeof(dpx_pair_dev), hipMemcpyHostToDevice);
        if (e != hipSuccess) { /* (the batch keeps its present mask) */
            (void)hipStreamSynchronize(b->stream);
            if (np) (void)hipMemcpy(b->dPairs, b->pairs.data(), np * sizeof(dpx_pair_dev), hipMemcpyHostToDevice);
            return hip_fail(e, "dpx_batch_set_reversed");
        }
    } else if (np) HIP_TRY(hipMemcpy(b->dPairs, table.data(), np * sizeof(dpx_pair_dev), hipMemcpyHostToDevice));
    b->dRev = std::move(built); /* (the old one parks: idle, both streams were waited for) */
    b->dFlagged = fresh ? reinterpret_cast<const int32_t *>(fresh + flaggedAt) : nullptr;
    b->revCount = flagged.size();
    b->revSaved = std::move(saved);
    b->pairs = std::move(table);
    set_seq_pointer(b, fresh ? fresh : b->dSeqOwn);
    if (fresh) b->uploadPending = true; /* the copies are being written on b->stream: a fill on a caller's stream waits for it once */
    invalidate_fill(b);
    trace.mark("set_reversed: uploads+launch");
    return DPX_OK;
}

} /* extern "C" */
