/* dpx_plan.cpp -- what a batch decides before it touches the device (dpx_plan.h).  Host code only: no HIP call, no sequence byte. */
#include "dpx_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <utility>


/* LDS request that caps residency at 16 fill waves per CU (9 KiB per wave of the workgroup) */
constexpr size_t kLdsFloor = 36u * 1024u * (DPX_FILL_THREADS / 64) / 4;

/* the three-plane Gotoh algorithms: ANW (global), ASW (local), BASW (local, banded), ASG (semi-global), BANW (global, banded) and BAXT
 * (extension, banded) */
bool is_affine(int algo) {
    return algo == DPX_ALGO_ANW || algo == DPX_ALGO_ASW || algo == DPX_ALGO_BASW || algo == DPX_ALGO_ASG || algo == DPX_ALGO_BANW ||
           algo == DPX_ALGO_BAXT;
}
/* the algorithms with a band parameter (and, unless the band covers the matrix, the anti-diagonal band kernels and layout) */
bool is_banded(int algo) { return algo == DPX_ALGO_BSW || algo == DPX_ALGO_BASW || algo == DPX_ALGO_BANW || algo == DPX_ALGO_BAXT; }
/* ... of which the three-plane ones (dpx_basw_kernels.hip, dpx_banw_kernels.hip, dpx_baxt_kernels.hip: chunks of three planes, no
 * packed-int16 variant) */
bool is_banded_affine(int algo) { return algo == DPX_ALGO_BASW || algo == DPX_ALGO_BANW || algo == DPX_ALGO_BAXT; }
/* ... of which the ones whose stored planes follow BANW's rules (in-band borders carry H, edge I / D and everything without storage is
 * minus infinity): k_banw_export and the k_banw_traceback walks read them */
bool is_banw_layout(int algo) { return algo == DPX_ALGO_BANW || algo == DPX_ALGO_BAXT; }

int validate_params(const dpx_params *p) {
    if (!p) return DPX_ERR_INVALID;
    if ((p->algo < DPX_ALGO_LNW || p->algo > DPX_ALGO_BANW) && p->algo != DPX_ALGO_BAXT) return DPX_ERR_INVALID; /* (8 and 9 are unassigned) */
    if (is_banded(p->algo) && p->band < 1) return DPX_ERR_INVALID;
    /* the int32 kernels add a weight to a cell value (|H| <= 32767 after fits_int16) and to the affine kernels' virtual
     * -2^29 borders: weights beyond +-2^20 could wrap those sums (and no int16 matrix could hold what they produce) */
    const long long lim = 1ll << 20;
    for (long long w : {(long long)p->match, (long long)p->mismatch, (long long)p->gapOpen,
                        is_affine(p->algo) ? (long long)p->gapExtend : 0ll})
        if (w > lim || w < -lim) return DPX_ERR_RANGE;
    return DPX_OK;
}

/* Can every value the algorithm stores for an (m x n) pair be held in an int16 cell?  Rigorous bounds: every H cell is
 * the maximum over alignment paths, so it is >= the score of the all-gap path and <= the sum of the positive
 * contributions any path can collect; the affine gap matrices are one open/extension away from an H cell. */
bool fits_int16(const dpx_params &p, long long m, long long n) {
    auto pos = [](long long v) { return v > 0 ? v : 0; };
    auto neg = [](long long v) { return v < 0 ? v : 0; };
    const long long lim = 32767, diag = pos(std::max<long long>(p.match, p.mismatch)) * std::min(m, n);
    if (p.algo == DPX_ALGO_LSW || p.algo == DPX_ALGO_BSW) {
        /* 0 <= H <= best diagonal run (+ positive gaps); the kernels also pack a column / step index into 16 bits */
        const long long top = diag + pos(p.gapOpen) * (m + n);
        return top <= lim && n <= 65000 && (m + n) <= 65000;
    }
    if (p.algo == DPX_ALGO_ASW || p.algo == DPX_ALGO_BASW) { /* (BASW: a band only removes paths, and its kernel packs the step index m + n into 16 bits as BSW's does) */
        /* 0 <= H <= hiH as for ANW; I, D >= o + e (an open from H >= 0, then extensions never below it: D = max(H + o + e, ...));
         * I, D <= hiH + o + e * max(m, n); the 16-bit column keys as for LSW */
        const long long o = p.gapOpen, e = p.gapExtend;
        const long long hiH = diag + (pos(o) + pos(e)) * (m + n);
        return neg(o + e) >= -lim && hiH + pos(o) + pos(e) * std::max(m, n) <= lim && n <= 65000 && (m + n) <= 65000;
    }
    if (p.algo == DPX_ALGO_LNW) {
        const long long lo = neg(p.gapOpen) * (m + n), hi = diag + pos(p.gapOpen) * (m + n);
        return lo >= -lim && hi <= lim;
    }
    if (p.algo == DPX_ALGO_BANW || p.algo == DPX_ALGO_BAXT) {
        /* hiH is ANW's: a band only removes paths, and hiH sums the positive contributions any path can collect.
         * loH: ANW's "every cell can fall back on the all-gap path" does not hold inside a band (that path leaves it).  A path that
         * does stay in the band reaches every in-band cell (i, j): the diagonal from (0, 0) to (k, k), k = min(i, j), whose cells have
         * i - j = 0, then ONE gap of |i - j| <= min(B - 1, max(m, n)) steps along row or column k, whose cells have |i' - j'| <= |i - j|.
         * H is the maximum over in-band paths, so with w = min(match, mismatch) and g = that gap bound
         *       H[i][j] >= k * w + (i != j ? o + |i - j| * e : 0) >= neg(w) * min(m, n) + neg(o) + neg(e) * g = loH
         * (the in-band border cells are the case k = 0).  The diagonal term the fill and the walks form, H[i-1][j-1] + s, is >= loH by
         * the same path with one diagonal step fewer and s in its place.  A finite I (D) is >= its open term H_left + o + e (H_up + o + e)
         * >= loH + (o + e), and <= hiH + pos(o) + pos(e) * max(m, n) as for ANW.  So every finite stored value is >= lo >= -32767, and
         * -32768 is free to stand for minus infinity in dpx_batch_matrix and in the walks' windows.  No m + n <= 65000: the kernel keeps
         * no step key.
         * BAXT: its cells are BANW's recurrence on the same band without the admission rule, and nothing above uses |m - n| <= B - 1:
         * the path (diagonal to (k, k), then one gap of |i - j| <= B - 1 steps) reaches every in-band cell of any m x n matrix and stays
         * in the band, and hiH holds for every path.  So the same bounds hold for every in-band H, I and D, and the score, a maximum of
         * H values and the 0 of (0, 0), lies in [0, hiH].  k_baxt_fill keeps a signed (H << 16 | 0xFFFF - step) key per slot: H inside
         * int16 is this check, and the step index m + n must fit 16 bits (the same 65000 as BASW's keys).
         * Under a substitution table (dpx_batch_set_substitution) the caller passes the largest table entry as `match` and the smallest
         * as `mismatch`, and the proofs carry over word for word: a diagonal step scores at least the minimum entry and at most the
         * maximum, which is all that w and `diag` use. */
        const long long o = p.gapOpen, e = p.gapExtend, g = std::min<long long>(std::max<long long>(p.band - 1, 0), std::max(m, n));
        const long long loH = neg(std::min<long long>(p.match, p.mismatch)) * std::min(m, n) + neg(o) + neg(e) * g;
        const long long hiH = diag + (pos(o) + pos(e)) * (m + n);
        if (p.algo == DPX_ALGO_BAXT && m + n > 65000) return false;
        return loH + neg(o + e) >= -lim && hiH + pos(o) + pos(e) * std::max(m, n) <= lim;
    }
    /* ANW, and ASG: every ASG cell H[i][j] is the best score of an alignment path between a reference substring ref[a:j] and the query
     * prefix qry[0:i] (the free row 0 chooses a), or the column-0 border, an all-gap path.  Such a path has at most m + n steps and at
     * most min(m, n) diagonal ones, so ANW's bounds hold for it: hiH sums the positive contributions a path can collect, loH is below
     * the all-gap path every cell can fall back on (o + i*e after a free row 0, or ANW's own).  I and D are one open / extension away
     * as for ANW.  ASG's fills also keep ((H + 32768) << 16 | 65535 - j) keys for row m: H inside int16 is this check, and the column
     * must fit 16 bits (the same 65000 as LSW's and ASW's keys). */
    const long long o = p.gapOpen, e = p.gapExtend;
    const long long loH = 2 * neg(o) + neg(e) * (m + n), hiH = diag + (pos(o) + pos(e)) * (m + n);
    const long long lo = loH + neg(o + e), hi = hiH + pos(o) + pos(e) * std::max(m, n);
    if (p.algo == DPX_ALGO_ASG && n > 65000) return false;
    return lo >= -lim && hi <= lim;
}

/* The same rigorous bounds for a DPX_KEEP_DIRECTIONS batch: int32 arithmetic, checked against 2^28 so that every value stays clear
 * of the affine kernels' -2^29 virtual borders; no column limit (no 16-bit column keys). */
bool fits_dir(const dpx_params &p, long long m, long long n) {
    auto pos = [](long long v) { return v > 0 ? v : 0; };
    auto neg = [](long long v) { return v < 0 ? v : 0; };
    const long long lim = 1ll << 28, diag = pos(std::max<long long>(p.match, p.mismatch)) * std::min(m, n);
    /* (BSW / BASW, DPX_KEEP_LOCAL_BAND_DIRECTIONS: LSW's and ASW's bounds -- a band only removes paths -- and no m + n limit: k_bdl_fill keeps
     * the value and the position of its running maximum in separate registers) */
    if (p.algo == DPX_ALGO_LSW || p.algo == DPX_ALGO_BSW) return diag + pos(p.gapOpen) * (m + n) <= lim;
    if (p.algo == DPX_ALGO_ASW || p.algo == DPX_ALGO_BASW) { /* fits_int16's ASW bounds without the column keys (the direction fill keeps an int32 column per row) */
        const long long o = p.gapOpen, e = p.gapExtend;
        const long long hiH = diag + (pos(o) + pos(e)) * (m + n);
        return neg(o + e) >= -lim && hiH + pos(o) + pos(e) * std::max(m, n) <= lim;
    }
    if (p.algo == DPX_ALGO_LNW) return neg(p.gapOpen) * (m + n) >= -lim && diag + pos(p.gapOpen) * (m + n) <= lim;
    if (p.algo == DPX_ALGO_BANW || p.algo == DPX_ALGO_BAXT) {
        /* DPX_KEEP_BAND_DIRECTIONS: fits_int16's loH / hiH argument for the band (the all-gap path leaves it; the diagonal to (k, k) and
         * one gap of at most min(B - 1, max(m, n)) steps does not), in int32.  No m + n limit for BAXT: k_bdir_fill keeps the value and
         * the position of its running maximum in separate registers. */
        const long long o = p.gapOpen, e = p.gapExtend, g = std::min<long long>(std::max<long long>(p.band - 1, 0), std::max(m, n));
        const long long loH = neg(std::min<long long>(p.match, p.mismatch)) * std::min(m, n) + neg(o) + neg(e) * g;
        const long long hiH = diag + (pos(o) + pos(e)) * (m + n);
        return loH + neg(o + e) >= -lim && hiH + pos(o) + pos(e) * std::max(m, n) <= lim;
    }
    /* ANW, and ASG by the argument in fits_int16 (its direction fill keeps row m's first maximum as an int32 value and column: no key, no column limit) */
    const long long o = p.gapOpen, e = p.gapExtend;
    const long long loH = 2 * neg(o) + neg(e) * (m + n), hiH = diag + (pos(o) + pos(e)) * (m + n);
    return loH + neg(o + e) >= -lim && hiH + pos(o) + pos(e) * std::max(m, n) <= lim;
}

/* The "+Opt" packed kernel (k_linear_fill_pk) does EVERY add in wrapping 16-bit halves (v_pk_add_i16 / v_pk_mad_i16), so
 * not only the stored H values but the weights themselves and the intermediates `diag + s` and `max(up, left) + gap`
 * must stay inside int16: H lies in [lo, hi] (fits_int16's bounds), an intermediate is one weight away from an H value
 * or a border value.  Batches that fail this run on the int32 kernels (same results, whatever the batch size). */
bool packed_safe(const dpx_params &p, long long m, long long n) {
    if (p.algo != DPX_ALGO_LNW && p.algo != DPX_ALGO_LSW && p.algo != DPX_ALGO_BSW) return false;
    auto pos = [](long long v) { return v > 0 ? v : 0; };
    auto neg = [](long long v) { return v < 0 ? v : 0; };
    const long long wmin = std::min<long long>({p.match, p.mismatch, p.gapOpen, 0}), wmax = std::max<long long>({p.match, p.mismatch, p.gapOpen, 0});
    if (wmin < -32768 || wmax > 32767) return false;
    const long long diag = pos(std::max<long long>(p.match, p.mismatch)) * std::min(m, n);
    const long long hi = diag + pos(p.gapOpen) * (m + n);
    const long long lo = p.algo == DPX_ALGO_LNW ? neg(p.gapOpen) * (m + n) : 0;
    return lo + wmin >= -32768 && hi + wmax <= 32767 && n <= 65535;
}

/* rows per lane of the lane-packed kernels: a pair of m rows takes ceil(m / 8) lanes (m <= 512); 16 rows per lane (two row
 * blocks) for the linear-gap kernels up to 1024 rows */
static int lanes_rows(int maxM, int algo) { return (maxM <= 512 || is_affine(algo)) ? 8 : 16; }

/* Pack pairs (`idx`, sorted by reference length, longest first) into waves of 64 lanes for the lane-packed kernels:
 * a pair takes ceil(m / R) consecutive lanes, a wave up to DPX_WAVE_SLOTS pairs whose staged references fit the wave's
 * LDS reference area.  Best fit over a window of open waves, so that the pairs of a wave have nearly the same reference
 * length (the wave runs max(n + lanes) steps) and the lanes fill up: 100k short reads (queries 80-130) reach 94 % lane
 * occupancy.  Returns the reference area in bytes; `idx` comes back in slot order (= matrix placement order). */
static size_t pack_waves(const std::vector<dpx_pair_dev> &pairs, std::vector<int32_t> &idx, int R, int maxN, size_t refFloor, int maxSlots,
                         std::vector<dpx_wave_desc> &waves) {
    struct Bin { dpx_wave_desc d; int lanes = 0, slots = 0; size_t ref = 0; bool closed = false; };
    const size_t refCap = std::max<size_t>(refFloor, align_up((size_t)maxN + 31, 16)); /* bytes of staged references per wave */
    constexpr size_t kWindow = 256; /* open waves: pairs arrive sorted by reference length, so a window keeps a wave's pairs alike */
    std::vector<Bin> bins;          /* in opening order = emission order */
    std::vector<int32_t> byFree[65]; /* open bins by free lanes (entries go stale when a bin moves on: checked on use) */
    uint64_t nonEmpty = 0;           /* bit f-1: byFree[f] holds entries (the search skips the empty buckets with one ctz) */
    size_t oldestOpen = 0, numOpen = 0;
    bins.reserve(idx.size() / 3 + 8);
    for (int32_t i : idx) {
        const dpx_pair_dev &pd = pairs[i];
        const int L = (pd.m + R - 1) / R;
        const size_t need = align_up((size_t)pd.n + 31, 16);
        int best = -1;
        for (uint64_t cand = L <= 64 ? nonEmpty & (~0ull << (L - 1)) : 0; cand && best < 0; cand &= cand - 1) { /* tightest fit first */
            const int f = __builtin_ctzll(cand) + 1;
            std::vector<int32_t> &lst = byFree[f];
            while (!lst.empty()) {
                const int32_t k = lst.back();
                const Bin &bn = bins[k];
                if (bn.closed || 64 - bn.lanes != f) { lst.pop_back(); continue; } /* stale entry */
                if (bn.slots >= maxSlots || bn.ref + need > refCap) break;   /* this bucket's newest bin is full in another way */
                best = k;
                lst.pop_back();
                break;
            }
            if (lst.empty()) nonEmpty &= ~(1ull << (f - 1));
        }
        if (best < 0) {
            if (numOpen >= kWindow) { /* retire the oldest open wave */
                while (bins[oldestOpen].closed) oldestOpen++;
                bins[oldestOpen].closed = true;
                numOpen--;
            }
            bins.emplace_back();
            memset(&bins.back().d, 0, sizeof(dpx_wave_desc));
            best = (int)bins.size() - 1;
            numOpen++;
        }
        Bin &bn = bins[best];
        bn.d.pair[bn.slots] = i;
        bn.d.first[bn.slots] = (uint8_t)bn.lanes;
        bn.d.num[bn.slots] = (uint8_t)L;
        bn.d.refOff[bn.slots] = (uint16_t)(bn.ref >> 4);
        bn.lanes += L;
        bn.slots++;
        bn.ref += need;
        if (bn.lanes < 64 && bn.slots < maxSlots) { byFree[64 - bn.lanes].push_back(best); nonEmpty |= 1ull << (64 - bn.lanes - 1); }
        else { bn.closed = true; numOpen--; }
    }
    std::vector<int32_t> order;
    order.reserve(idx.size());
    size_t area = 0;
    waves.reserve(bins.size());
    for (const Bin &bn : bins) {
        waves.push_back(bn.d);
        for (int k = 0; k < bn.slots; k++) order.push_back(bn.d.pair[k]);
        area = std::max(area, bn.ref);
    }
    idx.swap(order);
    return area;
}

/* cells (i, j) with 1 <= i <= m, 1 <= j <= n, |i - j| <= B - 1: sum over the rows of min(n, i+B-1) - max(1, i-B+1) + 1 */
static uint64_t band_cells(long long m, long long n, long long B) {
    if (m <= 0 || n <= 0 || B <= 0) return 0;
    const long long M = std::min(m, n + B - 1);                 /* rows that still reach the band */
    const long long a = std::max(0ll, std::min(n - B + 1, M));  /* rows whose right end is i + B - 1 (not clipped at n) */
    const long long s1 = a * (a + 1) / 2 + a * (B - 1) + (M - a) * n;
    const long long b = std::min(B, M);                         /* rows whose left end is clipped at column 1 */
    const long long s2 = b + (M > B ? (M - B + 1) * (M - B + 2) / 2 - 1 : 0);
    return (uint64_t)(s1 - s2 + M);
}

/* Waves per workgroup of the one-wave-per-pair / -couple kernels.  Their waves share nothing, so the workgroup is only the unit in which
 * the dispatcher hands waves to CUs: with four-wave workgroups 1250 waves are 313 workgroups on 256 CUs -- 57 CUs get eight waves, the
 * others four, and the launch takes as long as eight (tools/pairs_sweep.py: 2500 pairs of 1024^2 on the packed kernel 2322 GCUPS, 1900
 * pairs = 238 workgroups 3265).  Small launches therefore use one-wave workgroups (the CUs differ by at most one wave); big ones keep
 * four (a few per cent faster there: fewer workgroups to dispatch, profiles/r03/ab_nontemporal_stores_and_wg64.txt).  DPX_WPB=1|4 forces one. */
static uint32_t fill_waves_per_block(size_t waves, int knob) {
    if (knob == 1 || knob == 4) return (uint32_t)knob;
    return waves <= 4096 ? 1u : 4u;
}

namespace {

constexpr size_t kLdsMax = 160u * 1024u; /* one workgroup's LDS */
struct Shape { bool ragged = false, linear = false, banded = false; }; /* of the batch, and of the algorithm its kernel runs */

/* LDS layouts, each in one place.  One wave's staged reference [n + 128] (+16 everywhere: a staged string starts up to 15 bytes into its
 * buffer, at its own address mod 16 -- stage_bytes) */
size_t staged_ref_bytes(int maxN) { return align_up((size_t)maxN + 128 + 16, 16); }
/* one-wave-per-pair kernels, per wave: edge row(s) of int16 [n+2] + staged reference [n+128] + staged query of the rolling multi-stripe
 * schedule; band kernels: staged query + 64 B of index slack, then the reference; direction kernels: int32 edge row(s) [n+2] + staged
 * reference [n+192] */
struct MainLds { size_t edge, nEdges, ref, qry, perWave, dirEdge, dirPerWave; };
MainLds main_lds(const dpx_plan &p, bool banded) {
    const size_t edge = align_up((size_t)(p.maxN + 2) * 2, 16), nEdges = is_affine(p.prm.algo) ? 2 : 1 /* H and D */, ref = staged_ref_bytes(p.maxN);
    const size_t qry = align_up((size_t)p.maxM + 64 + 32, 16), rollQ = align_up((size_t)p.maxM + 64 * 16 + 32, 16);
    const size_t dirEdge = align_up((size_t)(p.maxN + 2) * 4, 16);
    return {edge, nEdges, ref, qry, banded ? qry + ref : edge * nEdges + ref + rollQ, dirEdge, dirEdge * nEdges + align_up((size_t)p.maxN + 192, 16)};
}
/* packed kernels, per wave: 4-byte edge entries (two int16) + 2-byte reference entries (two chars); band kernel: 2-byte query and
 * reference entries (two chars each) */
struct PackedLds { size_t refOff, perWave; };
PackedLds packed_lds(bool banded, int maxM, int maxN) {
    const size_t first = banded ? align_up(((size_t)maxM + 96) * 2, 16) : align_up((size_t)(maxN + 2) * 4, 16);
    return {first, first + (banded ? align_up(((size_t)maxN + 32) * 2, 16) : align_up(((size_t)maxN + 128) * 2, 16))};
}
/* split kernel, per workgroup: [control 512 B][staged reference][edge rows, one per stripe boundary, edgeStride int16 elements each] */
struct SplitLds { size_t qryOff, edgeStride, bytes; };
SplitLds split_lds(int maxN, int stripes) {
    const size_t edgeStride = align_up((size_t)maxN + 2, 8), qryOff = 512 + staged_ref_bytes(maxN);
    return {qryOff, edgeStride, qryOff + (size_t)std::max(stripes - 1, 0) * edgeStride * 2};
}
/* fits_int16()'s bound on H over the whole batch */
long long top_score(const dpx_plan &p) {
    return std::max<long long>({p.prm.match, p.prm.mismatch, 0}) * std::min<long long>(p.maxM, p.maxN) + std::max<long long>(p.prm.gapOpen, 0) * ((long long)p.maxM + p.maxN);
}
/* packed_safe() for the algorithm the kernel runs */
bool kernel_packed_safe(const dpx_plan &p) { dpx_params kp = p.prm; kp.algo = p.kernelAlgo; return packed_safe(kp, p.maxM, p.maxN); }

/* step 1: pairs and geometry */
int validate_pairs(const dpx_seq_pair *pairs, size_t numBytes, dpx_plan &p, Shape &sh, std::string &err) {
    const bool dirRange = (p.flags & (DPX_KEEP_DIRECTIONS | DPX_KEEP_BAND_DIRECTIONS | DPX_KEEP_LOCAL_BAND_DIRECTIONS)) != 0;
    p.pairs.resize(p.numPairs);
    for (size_t i = 0; i < p.numPairs; i++) {
        const dpx_seq_pair &sp = pairs[i];
        if (sp.referenceSize < 0 || sp.querySize < 0 || sp.referenceIdx < 0 || sp.queryIdx < 0 ||
            (size_t)sp.referenceIdx + (size_t)sp.referenceSize > numBytes || (size_t)sp.queryIdx + (size_t)sp.querySize > numBytes)
            return DPX_ERR_INVALID;
        const long long diff = std::llabs((long long)sp.querySize - (long long)sp.referenceSize);
        if (p.prm.algo == DPX_ALGO_BANW && diff >= (long long)p.prm.band) { /* no global path stays inside the band: the end cell (m, n) itself is outside it */
            err = "DPX_ALGO_BANW: pair " + std::to_string(i) + " (query " + std::to_string(sp.querySize) + ", reference " + std::to_string(sp.referenceSize) +
                  ") needs band >= " + std::to_string(diff + 1) + ", the batch has band " + std::to_string(p.prm.band);
            return DPX_ERR_UNSUPPORTED;
        }
        if (!(dirRange ? fits_dir(p.prm, sp.querySize, sp.referenceSize) : fits_int16(p.prm, sp.querySize, sp.referenceSize))) return DPX_ERR_RANGE;
        p.pairs[i] = dpx_pair_dev{sp.referenceIdx, sp.referenceSize, sp.queryIdx, sp.querySize, 0, 0, 64, 0};
        p.maxN = std::max(p.maxN, sp.referenceSize); p.maxM = std::max(p.maxM, sp.querySize);
        p.cells += (uint64_t)sp.referenceSize * (uint64_t)sp.querySize;
        if (sp.referenceSize != pairs[0].referenceSize || sp.querySize != pairs[0].querySize) sh.ragged = true;
    }
    return DPX_OK;
}

/* only the bytes this batch's pairs touch go to the device (a driver that cuts one big file into batches hands the whole file to every
 * dpx_batch_create): [seqLo, seqHi) is uploaded and the device-side indices are rebased */
void sequence_window(size_t numBytes, dpx_plan &p) {
    size_t seqLo = numBytes, seqHi = 0;
    for (const dpx_pair_dev &pd : p.pairs) {
        seqLo = std::min(seqLo, (size_t)std::min(pd.refIdx, pd.qryIdx));
        seqHi = std::max(seqHi, std::max((size_t)pd.refIdx + (size_t)pd.n, (size_t)pd.qryIdx + (size_t)pd.m));
    }
    if (seqHi <= seqLo) seqLo = seqHi = 0;
    if (p.packed2) seqLo &= ~(size_t)15; /* 2-bit input: the device expands whole dwords of 16 bases */
    for (dpx_pair_dev &pd : p.pairs) { pd.refIdx -= (int32_t)seqLo; pd.qryIdx -= (int32_t)seqLo; }
    p.seqLo = seqLo; p.seqHi = seqHi;
    if (!p.packed2) return;
    const size_t packedTotal = (numBytes + 3) / 4; /* bytes of the caller's packed buffer */
    p.packedDwords = (seqHi - seqLo + 15) / 16;
    p.packedCopy = std::min(p.packedDwords * 4, packedTotal - std::min(packedTotal, seqLo / 4));
}

/* step 2: dirs, bandDirs, kernelAlgo, and in `R` the rows (band kernels: cells) per lane of that algorithm's one-wave-per-pair kernel */
int choose_kernel(const Knobs &kn, dpx_plan &p, int &R) {
    const dpx_params &prm = p.prm;
    const long long longest = std::max(p.maxM, p.maxN);
    /* DPX_KEEP_BAND_DIRECTIONS: a covering BANW band takes the matrix batch's fall-back to ANW, as an ANW direction batch; every other band
     * runs k_bdir_fill */
    const bool bandDirFlag = (p.flags & DPX_KEEP_BAND_DIRECTIONS) != 0;
    const bool localFlag = (p.flags & DPX_KEEP_LOCAL_BAND_DIRECTIONS) != 0;
    /* (no ANW / ASW fall-back: neither has a second piece; dpx_plan_batch has paired each two-piece flag with its storage flag) */
    p.twoPiece = (bandDirFlag && (p.flags & DPX_TWO_PIECE_GAPS) != 0) || (localFlag && (p.flags & DPX_LOCAL_TWO_PIECE_GAPS) != 0);
    p.gapOpen2 = prm.gapOpen; p.gapExtend2 = prm.gapExtend;
    /* (DPX_LONG_SCORES: no fall-back either way -- no unbanded int32 score-only kernel exists; every band <= 512 runs the band kernel) */
    const bool bandDirCovering = bandDirFlag && !p.twoPiece && !p.bandScores && prm.algo == DPX_ALGO_BANW && (long long)prm.band >= longest + 1;
    /* DPX_KEEP_LOCAL_BAND_DIRECTIONS (BSW / BASW; dpx_plan_batch has refused every other algorithm): a covering band takes the matrix batch's
     * fall-back to LSW / ASW, as a direction batch of that algorithm; every other band runs k_bdl_fill (two pieces: k_lb2_fill, covering
     * or not) */
    const bool localCovering = localFlag && !p.twoPiece && !p.bandScores && (long long)prm.band >= longest;
    p.bandLocal = localFlag && !localCovering;
    p.dirs = (p.flags & DPX_KEEP_DIRECTIONS) != 0 || bandDirCovering || localCovering; p.bandDirs = (bandDirFlag && !bandDirCovering) || p.bandLocal; p.kernelAlgo = prm.algo;
    /* rows per lane: smallest tile that keeps short queries in one stripe, 8 (or DPX_R) otherwise */
    /* linear gaps: 16 rows per lane once a query is longer than 512 (one stripe up to 1024 rows, two 1-KiB sub-tiles per
     * step: measured 4 % faster than 8 rows x 2 rolling stripes); the affine kernel carries three chains and stays at 8 */
    /* direction kernels: LSW keeps per-row best cells and stays at <= 8 rows per lane (VGPRs), ANW at <= 8 as always */
    const bool wide = p.dirs ? prm.algo == DPX_ALGO_LNW : !is_affine(prm.algo);
    const int v = kn.rowsPerLane;
    R = (v == 2 || v == 4 || v == 8 || (v == 16 && wide)) ? v : p.maxM <= 128 ? 2 : p.maxM <= 256 ? 4 : (p.maxM <= 512 || !wide) ? 8 : 16;
    if (!is_banded(prm.algo)) return DPX_OK;
    if (p.twoPiece) { /* k_bd2_fill and k_lb2_fill hold <= 4 cells per lane, covering band or not */
        if (prm.band > DPX_BANDDIR2_MAX_BAND) return DPX_ERR_UNSUPPORTED;
        R = dpx_band_cpl(prm.band);
        return DPX_OK;
    }
    /* (BANW: + 1, its band applies to the border cells too -- at B = max(m, n) the border cell (m, 0) or (0, n) is outside it) */
    /* (BAXT: no covering fall-back -- no unbanded extension kernel exists; a band <= 512 that covers the matrix runs k_baxt_fill) */
    if (prm.algo != DPX_ALGO_BAXT && !p.bandScores && (long long)prm.band >= longest + (prm.algo == DPX_ALGO_BANW ? 1 : 0)) {
        p.kernelAlgo = prm.algo == DPX_ALGO_BSW ? DPX_ALGO_LSW : prm.algo == DPX_ALGO_BASW ? DPX_ALGO_ASW : DPX_ALGO_ANW; /* the band covers every cell: identical to the unbanded recurrence */
        return DPX_OK;
    }
    if (prm.band > 512) return DPX_ERR_UNSUPPORTED; /* band kernel holds <= 8 cells per lane (band <= 512) */
    R = dpx_band_cpl(prm.band);
    return DPX_OK;
}

/* step 3: the path.  Lane-packed path (short reads, the reference's own dataset shape): queries of <= 512 rows in a batch large enough to
 * fill the chip with a fraction of the waves run several pairs per wave, ceil(m/8) lanes each (k_linear_lanes /
 * k_affine_lanes, tile layout); DPX_LANES=0/1 overrides. */
struct LanePacking {
    int R = 0; bool pk = false;
    std::vector<int32_t> empties; /* pairs without cells: they run on the one-pair-per-wave kernel at this tile height */
    std::vector<dpx_wave_desc> waves;
    size_t refArea = 0, numPairs = 0;
};
/* Packed lane kernel (round 3, k_linear_lanes_pk): 16 rows per lane as two 8-row blocks of the SAME pair in the two halves of every
 * register.  Needs the 16-bit wrapping adds to be safe (packed_safe), room below the smallest border for its "minus infinity"
 * (the low half's column 0), and for SW: score * 8 + 7 in 16 bits (row tags) and gap <= 0, mismatch <= 0 (rows past the query's
 * end are not masked: with such weights they never exceed the real rows above them).  DPX_LANES_PK=0 keeps the int32 kernels. */
bool lanes_pk_ok(const dpx_plan &p, const Knobs &kn, const Shape &sh) {
    if (!(sh.linear && p.store && !p.dirs && p.maxM > 0 && p.maxM <= 1024) || kn.lanesPk == 0) return false;
    const dpx_params &prm = p.prm;
    const long long wmin = std::min<long long>({prm.match, prm.mismatch, prm.gapOpen, 0}), wmax = std::max<long long>({prm.match, prm.mismatch, prm.gapOpen, 0});
    const long long lowest = p.kernelAlgo == DPX_ALGO_LNW ? std::min<long long>(prm.gapOpen, 0) * ((long long)p.maxM + p.maxN) : 0;
    return kernel_packed_safe(p) && (-32768 - wmin + wmax <= lowest) &&
           (p.kernelAlgo != DPX_ALGO_LSW || (top_score(p) * 8 + 7 <= 65535 && prm.gapOpen <= 0 && prm.mismatch <= 0));
}
/* pack, measure the occupancy, keep or drop: nothing of the plan changes here */
bool try_lanes(const dpx_plan &p, const Knobs &kn, const Shape &sh, LanePacking &lp) {
    const bool lanesAlgo = sh.linear || (is_affine(p.kernelAlgo) && !sh.banded); /* (ANW: k_affine_lanes, ASW: k_asw_lanes, ASG: k_asg_lanes) */
    lp.pk = lanes_pk_ok(p, kn, sh); lp.R = lp.pk ? 16 : lanes_rows(p.maxM, p.kernelAlgo);
    /* (the staged references of a wave's pairs share its LDS: keep the path to references that leave the request small) */
    const bool lanesShape = lanesAlgo && p.maxM <= 64 * lp.R && p.maxM > 0 && p.maxN <= 4096;
    /* measured (tools/lanes_threshold.py): short reads x2048 56 vs 66 us, x4096 56 vs 114, x16384 121 vs 222 (below 2048 pairs the
     * split / one-wave-per-pair kernels win); 20000 x 250x300 (32 lanes per pair, two per wave) 608 vs 645 us, but 300x300 (38 lanes, one
     * per wave) 1074 vs 818 and 180x200 (23 lanes, two per wave) 395 vs 363: the path pays when the packing fills the lanes */
    const bool forced = kn.lanes >= 0;
    if (!(forced ? kn.lanes != 0 && lanesShape : lanesShape && p.maxM <= 256 && p.numPairs >= 2048) || p.dirs) return false; /* (directions: every pair on k_linear_dir / k_affine_dir) */
    std::vector<int32_t> idx; idx.reserve(p.numPairs);
    for (size_t i = 0; i < p.numPairs; i++) (p.pairs[i].m > 0 && p.pairs[i].n > 0 ? idx : lp.empties).push_back((int32_t)i);
    if (idx.empty()) return false;
    /* a wave runs max(n + lanes) steps: neighbours of similar reference length, longest first (then longest query first).
     * Both keys are small integers: two stable counting passes instead of a comparison sort (12 ms per 100k pairs) */
    std::vector<int32_t> tmp(idx.size());
    auto pass = [&](const std::vector<int32_t> &in, std::vector<int32_t> &out, int maxKey, auto key) {
        std::vector<uint32_t> cnt((size_t)maxKey + 2, 0);
        for (int32_t c : in) cnt[(size_t)(maxKey - key(c)) + 1]++; /* descending */
        for (size_t k = 1; k < cnt.size(); k++) cnt[k] += cnt[k - 1];
        for (int32_t c : in) out[cnt[(size_t)(maxKey - key(c))]++] = c;
    };
    pass(idx, tmp, p.maxM, [&](int32_t c) { return p.pairs[c].m; });
    pass(tmp, idx, p.maxN, [&](int32_t c) { return p.pairs[c].n; });
    lp.numPairs = idx.size();
    /* (reference area: 1 KiB keeps four workgroups of the 8-rows-per-lane kernels on a CU, up to 8 pairs per wave as in round 2; the
     * packed kernel's pairs take half the lanes, so its waves hold up to 12 pairs in 2 KiB: 2 x (18 + 2) KiB x 4 waves = 160 KiB) */
    lp.refArea = pack_waves(p.pairs, idx, lp.R, p.maxN, lp.pk ? 2048 : 1024, lp.pk ? DPX_WAVE_SLOTS : 8, lp.waves);
    size_t lanesUsed = 0;
    for (const dpx_wave_desc &wd : lp.waves) for (int k = 0; k < DPX_WAVE_SLOTS; k++) lanesUsed += wd.num[k];
    return forced || lanesUsed * 100 >= lp.waves.size() * 64 * 85; /* under 85 % of the lanes own rows: not worth it */
}

/* "+Opt" packed path (two equal-shaped pairs per wave on the v_pk_*_i16 pipe).  The fill is bound by store
 * instructions per CU-cycle, so halving the VALU work buys no cycles -- it buys clock: the chip holds ~2.3 GHz
 * instead of ~2.1 GHz under the lighter instruction stream (profiles/README.md), 4-7 % wall time.  Used when every
 * query fits one stripe (the packed kernel has no rolling schedule); DPX_PACKED=0/1 overrides. */
bool want_packed(const dpx_plan &p, const Knobs &kn, const Shape &sh, int R) {
    const bool bandedLinear = p.kernelAlgo == DPX_ALGO_BSW; /* (the packed-int16 band kernel exists for linear gaps only) */
    /* small batches need every wave they can get: one pair per wave there.  Measured with one-wave workgroups (round 3,
     * tools/pairs_sweep.py, profiles/r03/kernel_choice_by_batch_size.txt; GCUPS packed / one wave per pair / split): 1024 x 1024 at 1000
     * pairs 2014 / 2813 / 2615, 1500: 2971 / 2622 / 2487, 1900: 3052 / 2770 / 2650, 2500: 2749 / 2731 / 2683, 4000: 3226 / 2993 / 2650 --
     * the 16-rows-per-lane packed kernel wins from ~700 couples on; 512 x 512 (8 rows per lane) at 1500: 2235 / 2060 / 1987, 2000: 2432 /
     * 2495 / 2211, 3000: 2334 / 2744 / 2446, 4000: 2877 / 2811 / 2478 -- there only from ~2000 couples on */
    const size_t pkMinPairs = (sh.linear && R == 16) ? 1400 : 4096;
    bool use = p.store && ((sh.linear && dpx_tiled_stripes(p.maxM, R) == 1) || bandedLinear) && p.numPairs >= pkMinPairs;
    if (kn.packed >= 0) use = kn.packed != 0 && p.store && (sh.linear || bandedLinear);
    if (!use || p.dirs || p.bandDirs) return false; /* (band directions of BSW: every pair on k_bdl_fill) */
    /* 16-bit wrapping arithmetic: only when weights and every intermediate provably fit (also under DPX_PACKED=1) */
    if (!(kernel_packed_safe(p) && (!sh.banded || p.prm.gapOpen <= 0))) return false; /* (the packed band kernel's gap term saturates at 0) */
    return packed_lds(sh.banded, p.maxM, p.maxN).perWave * (DPX_FILL_THREADS / 64) <= kLdsMax; /* very long references do not fit the LDS twice over */
}
/* couple pairs of identical (m, n); everything else is left single */
void couple_pairs(const dpx_plan &p, bool ragged, std::vector<int32_t> &couples, std::vector<int32_t> &singles) {
    std::vector<int32_t> idx; idx.reserve(p.numPairs);
    for (size_t i = 0; i < p.numPairs; i++) (p.pairs[i].m > 0 && p.pairs[i].n > 0 ? idx : singles).push_back((int32_t)i);
    if (ragged)
        std::stable_sort(idx.begin(), idx.end(), [&](int32_t x, int32_t y) {
            const dpx_pair_dev &X = p.pairs[x], &Y = p.pairs[y];
            const uint64_t cx = (uint64_t)X.m * X.n, cy = (uint64_t)Y.m * Y.n;
            if (cx != cy) return cx > cy; /* longest first */
            return X.m != Y.m ? X.m > Y.m : X.n > Y.n;
        });
    for (size_t i = 0; i < idx.size();) {
        const bool twin = i + 1 < idx.size() && p.pairs[idx[i]].m == p.pairs[idx[i + 1]].m && p.pairs[idx[i]].n == p.pairs[idx[i + 1]].n;
        if (twin) couples.insert(couples.end(), {idx[i], idx[i + 1]});
        else singles.push_back(idx[i]);
        i += twin ? 2 : 1;
    }
}

/* Split path (small batches: fewer pairs than the chip has wave slots worth filling): one workgroup per pair, one wave per
 * stripe of 64 * R rows with R = 4 (2 for queries up to 256 rows), stripes concurrent (k_linear_split).  1000 pairs of
 * 512 x 512 become 2000 waves with half the dependent chain per step.  DPX_SPLIT=0/1 overrides.  `other`: the batch has a second kernel */
int split_rows(int maxM) { return maxM > 256 ? 4 : 2; }
bool want_split(const dpx_plan &p, const Knobs &kn, const Shape &sh, bool other) {
    const bool anyEmpty = std::any_of(p.pairs.begin(), p.pairs.end(), [](const dpx_pair_dev &pd) { return pd.m <= 0 || pd.n <= 0; });
    /* (queries over 4096 rows would need more than 16 stripes: not split.  Twice the stripes at 2 rows per lane -- four waves per 512-row pair --
     * lose: 1000 x 512^2 0.146 vs 0.120 ms, profiles/r04/configs1_split_variants.txt: the kernel is bound by its instruction stream, not by waves) */
    const int sW = dpx_tiled_stripes(p.maxM, split_rows(p.maxM));
    const bool shape = sh.linear && p.store && !p.dirs && !other && !anyEmpty && p.numPairs > 0 && sW >= 2 && sW <= 16 && split_lds(p.maxN, sW).bytes <= kLdsMax;
    /* measured (bench.py --pairs N, DPX_SPLIT=0/1, HIP events around every fill; GCUPS split vs one wave per pair):
     *   1024 x 1024 (4 stripes of 4 rows per lane against ONE 16-rows-per-lane wave): 600 pairs 1864 vs 1768, 1200: 2229 vs 1765,
     *   2500: 2483 vs 2315, 3500: 2592 vs 2393, 4096: 2603 vs 2671 (and the packed kernel takes over);
     *   512 x 512 (2 stripes against one 8-rows-per-lane wave): 500 pairs 1021 vs 1003, 1000: 2084 vs 2003, 1500: 1841 vs 1935.
     * So: any shape up to ~1100 pairs, shapes of four or more stripes up to the packed kernel's threshold.
     * Round 3, with one-wave workgroups for the one-wave-per-pair kernels (tools/pairs_sweep.py; split vs one wave per pair): 1024 x 1024
     * 300 pairs 1373 vs 855, 600: 2111 vs 1699, 1000: 2615 vs 2805, 1500: 2487 vs 2622, 3000: 2636 vs 2779-2962; 512 x 512 600 pairs 1323 vs
     * 1173, 1000: 1943 vs 1932, 1500: 1987 vs 2060, 3000: 2446 vs 2744 -- queries that fit one stripe of the other kernels (<= 1024
     * rows) split only up to ~900 pairs (up to 512 rows: ~1100, a tie from there on); longer ones (the other kernels roll over several stripes) as before. */
    /* (round 3's packed variant of this kernel -- couples of equal-shaped pairs, two per workgroup on the VOP3P pipe -- halved the waves as
     * well as the instructions and lost wherever the split kernel is used: 1000 x 512^2 0.158 vs 0.119 ms, 2000 x 512^2 0.209 vs 0.206;
     * deleted in round 4, profiles/r04/configs1_split_variants.txt) */
    if (kn.split >= 0) return kn.split != 0 && shape;
    return shape && (p.maxM > 1024 ? (p.numPairs <= 1100 || (sW >= 4 && p.numPairs < 4096)) : p.numPairs <= (p.maxM > 512 ? 900u : 1100u));
}

/* lanes, packed, split or plain; returns the lane-packed waves' reference area */
size_t decide_path(const Knobs &kn, const Shape &sh, int baseR, dpx_plan &p) {
    LanePacking lp;
    if (try_lanes(p, kn, sh, lp)) {
        p.lanePacked = true; p.lanesPk = lp.pk;
        p.waves = std::move(lp.waves); p.singles = std::move(lp.empties);
        p.nLanePairs = lp.numPairs; p.nWaves = p.waves.size();
    } else if (want_packed(p, kn, sh, baseR)) {
        couple_pairs(p, sh.ragged, p.couples, p.singles); /* (no couple found: every pair runs the one-wave-per-pair kernel, in this order) */
        p.packed = !p.couples.empty();
        p.nCouples = p.couples.size() / 2;
    }
    p.split = want_split(p, kn, sh, p.lanePacked || p.packed);
    if (p.split) { p.splitWaves = dpx_tiled_stripes(p.maxM, split_rows(p.maxM)); p.splitLds = split_lds(p.maxN, p.splitWaves).bytes; }
    p.R = p.lanePacked ? lp.R : p.split ? split_rows(p.maxM) : baseR;
    for (dpx_pair_dev &pd : p.pairs) { /* the layout tag of every pair and the rows per lane of the kernel that fills it (dpx_layout.h) */
        const bool inWave = p.lanePacked && pd.m > 0 && pd.n > 0;
        pd.lanes = p.split ? 32 : inWave ? 16 : 64;
        pd.rows = p.split || inWave ? (uint16_t)p.R : 0;
    }
    return p.lanePacked ? lp.refArea : 0;
}

/* step 4: the order of the one-wave-per-pair kernel, longest first (a ragged batch without a second kernel: all its pairs) */
void order_singles(bool ragged, dpx_plan &p) {
    if (!p.packed && !p.lanePacked && ragged) {
        p.singles.resize(p.numPairs);
        std::iota(p.singles.begin(), p.singles.end(), 0);
    }
    std::stable_sort(p.singles.begin(), p.singles.end(), [&](int32_t x, int32_t y) {
        return (uint64_t)p.pairs[x].m * p.pairs[x].n > (uint64_t)p.pairs[y].m * p.pairs[y].n;
    });
    p.nSingles = (p.packed || p.lanePacked) ? p.singles.size() : p.numPairs;
}

/* step 5: matrix placement (dpx_layout.h): pairs that are launched next to each other are interleaved chunk by chunk in
 * groups of `group` waves, so a group writes one compact moving window instead of `group` far-apart streams; and the algorithmic
 * bytes: int16 cells incl. borders, sequences, 16 B pair record, 12 B result */
void place_matrices(const Knobs &kn, bool banded, dpx_plan &p) {
    const int bandPlanes = is_banded_affine(p.kernelAlgo) ? 3 : 1;
    for (const dpx_pair_dev &pd : p.pairs) {
        p.algBytes += (uint64_t)pd.m + (uint64_t)pd.n + 16u + 12u;
        const uint64_t inband = (p.bandDirs || (banded && p.store && !p.dirs)) ? band_cells(pd.m, pd.n, p.prm.band) : 0;
        p.bandCells += inband;
        if (p.dirs) p.algBytes += ((uint64_t)(pd.m + 1) * (uint64_t)(pd.n + 1) + 1) / 2; /* half a byte per cell */
        else if (p.bandScores) {}                                                        /* DPX_LONG_SCORES: nothing but the results */
        else if (p.bandDirs) p.algBytes += p.twoPiece ? inband : (inband + 1) / 2;        /* half a byte per in-band cell, two-piece: a byte */
        else if (p.store && banded) p.algBytes += 2ull * (uint64_t)bandPlanes * inband;   /* 2 B per in-band cell and plane */
        else if (p.store) p.algBytes += 2ull * (uint64_t)p.planes * (uint64_t)(pd.m + 1) * (uint64_t)(pd.n + 1);
    }
    if (!p.store) return;
    const size_t group = (kn.group >= 1 && kn.group <= 1000000) ? (size_t)kn.group : 64;
    const uint32_t chunkElems = p.bandDirs ? 512u : banded ? dpx_band_chunk_elems(bandPlanes) : (p.split || p.dirs) ? 512u : dpx_tiled_chunk_elems(p.R, p.planes); /* (dirs: 1-KiB code chunks) */
    auto chunksOf = [&](const dpx_pair_dev &pd) -> uint64_t {
        if (p.dirs) return dpx_dir_chunks(pd.m, pd.n, p.R);
        if (p.bandDirs) return p.twoPiece ? dpx_banddir2_chunks(pd.m, pd.n, p.prm.band) : dpx_banddir_chunks(pd.m, pd.n, p.prm.band);
        if (pd.lanes == 32) return dpx_split_chunks(pd.m, pd.n, p.R);
        return banded ? dpx_band_chunks(pd.m, pd.n, p.prm.band) : dpx_tiled_chunks(pd.m, pd.n, p.R);
    };
    uint64_t off = 0;
    auto place = [&](const std::vector<int32_t> &slots, size_t slotsPerGroup) { /* slots in launch order */
        for (size_t s0 = 0; s0 < slots.size(); s0 += slotsPerGroup) {
            const size_t cnt = std::min(slotsPerGroup, slots.size() - s0);
            uint64_t maxChunks = 0;
            for (size_t g = 0; g < cnt; g++) maxChunks = std::max(maxChunks, chunksOf(p.pairs[slots[s0 + g]]));
            for (size_t g = 0; g < cnt; g++) {
                dpx_pair_dev &pd = p.pairs[slots[s0 + g]];
                pd.matOff = off + (uint64_t)g * chunkElems;
                pd.chunkStride = (uint32_t)(cnt * chunkElems);
            }
            off += maxChunks * (uint64_t)cnt * chunkElems;
        }
    };
    if (p.packed) place(p.couples, group * 2); /* one wave (workgroup) = two adjacent slots */
    else if (p.lanePacked) { /* tile layout (dpx_layout.h): every wave a contiguous stream of chunks, one per step; its pairs share the base */
        const uint32_t stepElems = dpx_wtile_step_elems(p.R / 8, p.planes);
        for (const dpx_wave_desc &wd : p.waves) {
            uint64_t steps = 0;
            for (int k = 0; k < DPX_WAVE_SLOTS; k++) {
                if (!wd.num[k]) continue;
                dpx_pair_dev &pd = p.pairs[wd.pair[k]];
                pd.matOff = off; pd.chunkStride = wd.first[k];
                steps = std::max(steps, dpx_wtile_steps(pd.m, pd.n, p.R, wd.first[k]));
            }
            off += steps * (uint64_t)stepElems;
        }
    }
    if (p.packed || p.lanePacked || !p.singles.empty()) {
        place(p.singles, group);
    } else { /* launch order == pair order */
        std::vector<int32_t> ident(p.numPairs);
        std::iota(ident.begin(), ident.end(), 0);
        place(ident, group);
    }
    p.matElems = off;
    /* where k_traceback puts a pair's three lines (each with a dword-aligned capacity of m + n + 1): needed by the output path,
     * uploaded at creation so that dpx_batch_output_begin() never has to wait for the host */
    uint64_t tb = 0; p.tbOff.resize(p.numPairs + 1);
    for (size_t i = 0; i < p.numPairs; i++) { p.tbOff[i] = tb; tb += 3ull * (uint64_t)((p.pairs[i].m + p.pairs[i].n + 1 + 3) & ~3); }
    p.tbOff[p.numPairs] = tb;
}

/* step 6: LDS geometry and launch scalars */
int launch_scalars(const Knobs &kn, bool banded, size_t lanesRefArea, dpx_plan &p) {
    const dpx_params &prm = p.prm;
    const MainLds l = main_lds(p, banded);
    /* Store-bound fills run ~2 % faster with 3-4 waves per SIMD than with 6-7 (fewer write streams in flight,
     * profiles/README.md): cap residency at 4 workgroups per CU through the LDS request. */
    const size_t four = l.perWave * (DPX_FILL_THREADS / 64), floored = (p.store && !banded && four < kLdsFloor) ? kLdsFloor : four;
    /* band directions: BANW's staging; when four waves' strings do not fit one workgroup's LDS (long references are what these batches
     * are for) the fill runs one-wave workgroups, and the batch is refused only when one wave's strings do not fit */
    const bool bandDirOneWave = p.bandDirs && floored > kLdsMax && l.perWave <= kLdsMax;
    p.ldsBytes = p.dirs ? 0 : bandDirOneWave ? l.perWave : floored;
    if (p.ldsBytes > kLdsMax) return DPX_ERR_UNSUPPORTED;
    dpx_fill_args &a = p.args;
    a.numPairs = (int32_t)p.nSingles; a.wavesPerBlock = bandDirOneWave ? 1u : fill_waves_per_block(p.nSingles, kn.wavesPerBlock);
    a.match = prm.match; a.mismatch = prm.mismatch; a.gapOpen = prm.gapOpen; a.gapExtend = prm.gapExtend; a.band = prm.band;
    a.ldsPerWave = (uint32_t)l.perWave; a.ldsEdge2Off = (uint32_t)l.edge;
    a.ldsRefOff = banded ? (uint32_t)l.qry : (uint32_t)(l.edge * l.nEdges);
    a.ldsQryOff = banded ? 0u : (uint32_t)(l.edge * l.nEdges + l.ref);
    /* big batches are bound by the bytes they write: their ramp steps store only the lines that hold cells (6 % fewer bytes at
     * 1024 x 1024: +3 % LSW, +5 % LNW); small ones are bound by step latency and keep the cheaper whole-chunk stores */
    a.rampLines = kn.rampLines >= 0 ? kn.rampLines != 0 : p.numPairs >= 2048;
    if (p.split) {
        const SplitLds s = split_lds(p.maxN, p.splitWaves);
        a.ldsRefOff = 512u; a.ldsQryOff = (uint32_t)s.qryOff; a.ldsBufStride = (uint32_t)s.edgeStride;
    }
    dpx_fill_args &k = p.pkArgs;
    if (p.packed) {
        const PackedLds pl = packed_lds(banded, p.maxM, p.maxN);
        k = a;
        k.numPairs = (int32_t)p.nCouples; k.wavesPerBlock = fill_waves_per_block(p.nCouples, kn.wavesPerBlock);
        k.ldsPerWave = (uint32_t)pl.perWave; k.ldsRefOff = (uint32_t)pl.refOff;
        p.pkLdsBytes = pl.perWave * (DPX_FILL_THREADS / 64);
        /* SW start cell: one (score, row-in-lane, column) key per pair and lane where score * R + R-1 provably fits 16 bits
         * (1024 x 1024 at match 3: 3072 * 16 + 15), else one (score, column) key per pair and row (32 more registers at R = 16) */
        k.rowTags = !banded && p.kernelAlgo == DPX_ALGO_LSW && top_score(p) * p.R + p.R - 1 <= 65535 && prm.gapOpen <= 0 /* (the saturating gap term) */ &&
                    kn.rowTags != 0; /* (tests: 0 = the per-row keys) */
    } else if (p.lanePacked) { /* per wave: the line stage of the writeback (dpx_kernels.hip: LineStage) + the staged references of its pairs */
        k = a;
        k.numPairs = (int32_t)p.nWaves; k.ldsPerWave = (uint32_t)(dpx_lanes_stage_bytes(p.kernelAlgo, p.R, p.store) + lanesRefArea);
        /* (the lane-packed kernels keep their four-wave workgroups at every size: 20 000 short reads 131-148 us against 150-153 with one-wave
         * workgroups, 100 000 the same; DPX_WPB=1 forces the latter) */
        k.wavesPerBlock = is_affine(p.kernelAlgo) ? 1u : (kn.wavesPerBlock == 1 ? 1u : (uint32_t)dpx_lanes_waves_per_block(p.kernelAlgo));
        p.pkLdsBytes = (size_t)k.ldsPerWave * (size_t)k.wavesPerBlock;
        if (p.pkLdsBytes > kLdsMax) return DPX_ERR_UNSUPPORTED;
    }
    if (p.dirs) {
        /* the edge rows live per wave in LDS, or -- when even a one-wave workgroup could not hold them -- behind the codes */
        const bool dirGlobal = l.dirPerWave > 64u * 1024u;
        if (dirGlobal) p.dirScratch = align_up(std::min<size_t>(std::max<size_t>(p.nSingles, 1), DPX_DIR_SCRATCH_SLOTS) * l.dirPerWave, 256);
        dpx_dir_args &d = p.dirArgs;
        d.numPairs = (int32_t)p.nSingles; d.match = prm.match; d.mismatch = prm.mismatch; d.gapOpen = prm.gapOpen; d.gapExtend = prm.gapExtend;
        d.ldsPerWave = (uint32_t)l.dirPerWave; d.ldsEdge2Off = (uint32_t)l.dirEdge; d.ldsRefOff = (uint32_t)(l.dirEdge * l.nEdges);
        /* four waves per workgroup when their LDS fits, one otherwise */
        d.wavesPerBlock = (dirGlobal || l.dirPerWave * 4 > kLdsMax) ? 1u : fill_waves_per_block(p.nSingles, kn.wavesPerBlock);
    }
    return DPX_OK;
}

} // namespace

int dpx_plan_batch(const dpx_params &params, const dpx_seq_pair *pairs, size_t firstPair, size_t numPairs, size_t numBytes, bool packed2Input,
                   unsigned flags, const Knobs &kn, dpx_plan &p, std::string &err) {
    p = dpx_plan();
    if (flags & DPX_KEEP_LOCAL_BAND_DIRECTIONS) { /* BSW / BASW only, and with none of the flags that choose another storage */
        if (flags & (DPX_SCORE_ONLY | DPX_KEEP_BAND_DIRECTIONS | DPX_TWO_PIECE_GAPS)) return DPX_ERR_INVALID;
        if (params.algo != DPX_ALGO_BSW && params.algo != DPX_ALGO_BASW) return DPX_ERR_UNSUPPORTED;
        if (flags & DPX_KEEP_DIRECTIONS) return DPX_ERR_UNSUPPORTED; /* 0x8 on a banded algorithm stays refused */
    }
    if (flags & DPX_LOCAL_TWO_PIECE_GAPS) { /* legal only together with DPX_KEEP_LOCAL_BAND_DIRECTIONS (whose own checks came first), on BASW: BSW has one linear gap weight */
        if (!(flags & DPX_KEEP_LOCAL_BAND_DIRECTIONS) || (flags & (DPX_SCORE_ONLY | DPX_KEEP_BAND_DIRECTIONS | DPX_TWO_PIECE_GAPS))) return DPX_ERR_INVALID;
        if (params.algo != DPX_ALGO_BASW) return DPX_ERR_UNSUPPORTED;
    }
    if (flags & DPX_TWO_PIECE_GAPS) { /* legal only together with DPX_KEEP_BAND_DIRECTIONS, on the algorithms that flag serves */
        if (!(flags & DPX_KEEP_BAND_DIRECTIONS)) return DPX_ERR_INVALID;
        if (params.algo != DPX_ALGO_BANW && params.algo != DPX_ALGO_BAXT) return DPX_ERR_UNSUPPORTED;
    }
    if (flags & DPX_LONG_SCORES) { /* legal only together with exactly one of the two band-direction storage flags, whose own checks came first */
        const bool global = (flags & DPX_KEEP_BAND_DIRECTIONS) != 0, local = (flags & DPX_KEEP_LOCAL_BAND_DIRECTIONS) != 0;
        if (global == local || (flags & DPX_SCORE_ONLY)) return DPX_ERR_INVALID;
        if (flags & DPX_KEEP_DIRECTIONS) return DPX_ERR_UNSUPPORTED; /* 0x8 on a banded algorithm stays refused */
        if (global ? (params.algo != DPX_ALGO_BANW && params.algo != DPX_ALGO_BAXT) : (params.algo != DPX_ALGO_BSW && params.algo != DPX_ALGO_BASW)) return DPX_ERR_UNSUPPORTED;
        if (flags & (DPX_TWO_PIECE_GAPS | DPX_LOCAL_TWO_PIECE_GAPS)) return DPX_ERR_UNSUPPORTED; /* the two-piece steps are not built for the scoring pass */
    }
    p.prm = params; p.flags = flags; p.numPairs = numPairs; p.packed2 = packed2Input;
    p.bandScores = (flags & DPX_LONG_SCORES) != 0;
    p.store = !(flags & DPX_SCORE_ONLY) && !p.bandScores; p.planes = is_affine(params.algo) ? 3 : 1;
    Shape sh; int baseR = 0;
    int rc = validate_pairs(numPairs ? pairs + firstPair : pairs, numBytes, p, sh, err);
    if (rc == DPX_OK) rc = choose_kernel(kn, p, baseR);
    if (rc != DPX_OK) return rc;
    sh.linear = p.kernelAlgo == DPX_ALGO_LNW || p.kernelAlgo == DPX_ALGO_LSW; sh.banded = is_banded(p.kernelAlgo);
    const size_t lanesRefArea = decide_path(kn, sh, baseR, p);
    order_singles(sh.ragged, p);
    sequence_window(numBytes, p);
    place_matrices(kn, sh.banded, p);
    return launch_scalars(kn, sh.banded, lanesRefArea, p);
}

/* How to walk (round 4, tools/tb_kernel.sh, kernel time alone; profiles/r04/traceback_walks.txt).  Walk 2 = one WAVE per pair
 * (k_traceback_wave: runs of path steps decided by all lanes at once from an LDS window): LSW / LNW always -- 1000 x 512^2 0.13 vs
 * 0.60 ms for one lane per pair, 16 000 x 512^2 0.50 vs 0.76, 20 000 x 300^2 0.36 vs 0.54, 100 000 short reads 0.33 vs 0.57 (LSW) /
 * 0.71 vs 0.69 (LNW); ANW (three planes per window, 48-row banded windows) up to 20 000 pairs -- 1000 x 512^2 0.17 vs 1.16,
 * 5000 x 1024^2 0.86 vs 2.51, 20 000 x 300^2 0.92 vs 0.98, but 100 000 short reads 1.48 vs 0.98.  Walks 0 / 1 = one lane
 * per pair, cell by cell / through register-cached column vectors (the latter from 64k pairs on: enough lanes in flight to thrash
 * L1 / L2 between two steps of a lane).  Banded matrices: walk 2 as well (its band-layout window loads; numbers in the same file).
 * Banded affine SW: as ASW -- one wave per pair up to 20 000 pairs (k_basw_traceback_wave, band-layout window loads for the three
 * planes), one lane per pair beyond that or under DPX_TB_WALK=0 / 1 (k_basw_traceback); banded affine NW and the extension, which walks
 * from its end cell to the anchor: the same choice.  DPX_TB_WALK=0/1/2 forces one (tests). */
static int walk_mode(const dpx_plan &p, int tbWalk) {
    if (tbWalk >= 0) return std::min(2, tbWalk);
    if (!is_affine(p.kernelAlgo)) return 2; /* LSW, LNW, BSW */
    return p.numPairs <= 20000 ? 2 : p.numPairs >= 65536 ? 1 : 0; /* (ASW: as ANW; its walk 1 is walk 0) */
}

dpx_route dpx_plan_route(const dpx_plan &p, int tbWalk, int zdrop, int endBonus, int substAlphabet) {
    const int algo = p.kernelAlgo;
    dpx_route r{};
    r.ext = algo == DPX_ALGO_BAXT;
    const bool extension = r.ext && (zdrop >= 0 || endBonus >= 0);
    const dpx_fill_kernel lanes[] = {DPX_K_LINEAR_LANES, DPX_K_AFFINE_LANES, DPX_K_ASW_LANES, DPX_K_ASG_LANES};
    const dpx_fill_kernel fill[] = {DPX_K_LINEAR_FILL, DPX_K_AFFINE_FILL, DPX_K_ASW_FILL, DPX_K_ASG_FILL};
    const dpx_fill_kernel dir[] = {DPX_K_LINEAR_DIR, DPX_K_AFFINE_DIR, DPX_K_ASW_DIR, DPX_K_ASG_DIR};
    const int family = algo == DPX_ALGO_ANW ? 1 : algo == DPX_ALGO_ASW ? 2 : algo == DPX_ALGO_ASG ? 3 : 0;
    if (p.dirs) {
        r.dirs = true; r.kernel = dir[family];
        r.dirTable = substAlphabet != 0 && family != 0; /* (set only by dpx_batch_set_direction_table, on a DPX_KEEP_DIRECTIONS batch of the three) */
    } else if (p.bandScores) { /* (DPX_LONG_SCORES: one kernel per unit in every mode the admitted setters bring; no walk, no export) */
        r.main = p.bandLocal ? DPX_MAIN_LSCORE : DPX_MAIN_BSCORE; r.kernel = p.bandLocal ? DPX_K_LSCORE_FILL : DPX_K_BSCORE_FILL;
    } else if (p.bandLocal) { /* (a table comes through dpx_batch_set_local_direction_table only; every other setter refuses these batches) */
        if (p.twoPiece) { r.main = DPX_MAIN_LB2; r.kernel = DPX_K_LB2_FILL; } /* (DPX_LOCAL_TWO_PIECE_GAPS: one kernel with and without a table) */
        else { r.main = substAlphabet ? DPX_MAIN_BDLT : DPX_MAIN_BDL; r.kernel = substAlphabet ? DPX_K_BDLT_FILL : DPX_K_BDL_FILL; }
    } else if (p.bandDirs) { /* (a mode comes through dpx_batch_set_direction_scoring only; extension mode is BAXT's) */
        const bool bdx = extension || substAlphabet;
        r.main = p.twoPiece ? DPX_MAIN_BD2 : bdx ? DPX_MAIN_BDX : DPX_MAIN_BDIR; r.kernel = p.twoPiece ? DPX_K_BD2_FILL : bdx ? DPX_K_BDX_FILL : DPX_K_BDIR_FILL;
    } else if (substAlphabet && family != 0) { /* (set only by dpx_batch_set_score_table, on a DPX_SCORE_ONLY batch of the three: the launches of the plain
                                                * batch, each through its k_scoretab twin; the kernel= names stay) */
        r.scoreTable = true;
        r.second = p.lanePacked ? DPX_SECOND_LANES : DPX_SECOND_NONE;
        if (!r.second || p.args.numPairs > 0) r.main = DPX_MAIN_FILL;
        r.kernel = p.lanePacked ? lanes[family] : fill[family];
    } else if (substAlphabet) { /* (set only on batches whose kernel is BANW's or BAXT's; with extension mode: dpx_batch_set_extension_table) */
        r.main = extension ? DPX_MAIN_ZSUB : DPX_MAIN_SUBST; r.kernel = extension ? DPX_K_ZSUB_FILL : DPX_K_SUBST_FILL;
    } else if (algo == DPX_ALGO_BAXT) {
        r.main = extension ? DPX_MAIN_ZEXT : DPX_MAIN_BAXT; r.kernel = extension ? DPX_K_ZEXT_FILL : DPX_K_BAXT_FILL;
    } else if (algo == DPX_ALGO_BANW) {
        r.main = DPX_MAIN_BANW; r.kernel = DPX_K_BANW_FILL;
    } else if (algo == DPX_ALGO_BASW) {
        r.main = DPX_MAIN_BASW; r.kernel = DPX_K_BASW_FILL;
    } else { /* dpx_launch_fill's algorithms, with or without a secondary kernel that takes most of the pairs */
        const bool bsw = algo == DPX_ALGO_BSW;
        r.second = p.packed ? (bsw ? DPX_SECOND_BANDED_PACKED : DPX_SECOND_PACKED) : p.lanesPk ? DPX_SECOND_LANES_PK : p.lanePacked ? DPX_SECOND_LANES : DPX_SECOND_NONE;
        r.split = !r.second && p.split;
        if (r.second ? p.args.numPairs > 0 : !r.split) r.main = DPX_MAIN_FILL;
        r.kernel = bsw ? (p.packed ? DPX_K_BANDED_FILL_PK : DPX_K_BANDED_FILL)
                   : family ? (p.lanePacked ? lanes[family] : fill[family])
                   : p.packed ? DPX_K_LINEAR_FILL_PK : p.lanesPk ? DPX_K_LINEAR_LANES_PK : p.lanePacked ? DPX_K_LINEAR_LANES : p.split ? DPX_K_LINEAR_SPLIT : DPX_K_LINEAR_FILL;
    }
    r.extRecords = r.main == DPX_MAIN_ZEXT || r.main == DPX_MAIN_ZSUB || ((r.main == DPX_MAIN_BDX || r.main == DPX_MAIN_BD2 || r.main == DPX_MAIN_BSCORE) && extension);
    r.walk = p.bandLocal ? (p.twoPiece ? DPX_WALK_LB2 : DPX_WALK_BDL) : p.twoPiece ? DPX_WALK_BD2 : p.bandDirs ? DPX_WALK_BDIR : (substAlphabet && !p.dirs && !r.scoreTable) ? DPX_WALK_SUBST : algo == DPX_ALGO_BASW ? DPX_WALK_BASW : is_banw_layout(algo) ? DPX_WALK_BANW
             : p.dirs ? DPX_WALK_DIR : DPX_WALK_PLAIN;
    r.walkMode = (r.walk == DPX_WALK_BDL || r.walk == DPX_WALK_LB2 || r.walk == DPX_WALK_BD2 || r.walk == DPX_WALK_BDIR || r.walk == DPX_WALK_DIR) ? 0 : walk_mode(p, tbWalk); /* (one walk: DPX_TB_WALK has no effect) */
    r.exportKind = is_banw_layout(algo) /* (BAXT stores what BANW stores) */ ? DPX_EXPORT_BANW : algo == DPX_ALGO_BASW ? DPX_EXPORT_BASW : DPX_EXPORT_PLAIN;
    return r;
}

unsigned dpx_plan_bdx_waves(const dpx_plan &p, bool table) {
    if (!table) return p.args.wavesPerBlock;
    const size_t perWave = (size_t)p.args.ldsPerWave + DPX_SUBST_IMAGE_BYTES;
    if (perWave > kLdsMax) return 0u;
    return perWave * (DPX_FILL_THREADS / 64) > kLdsMax ? 1u : p.args.wavesPerBlock;
}

unsigned dpx_plan_dirtab_waves(const dpx_plan &p) {
    const size_t perWave = (p.dirScratch ? 0 : (size_t)p.dirArgs.ldsPerWave) + DPX_SUBST_IMAGE_BYTES;
    return perWave * p.dirArgs.wavesPerBlock <= kLdsMax ? p.dirArgs.wavesPerBlock : 1u;
}

unsigned dpx_plan_scoretab_waves(const dpx_plan &p) {
    const size_t perWave = dpx_plan_scoretab_lds(p);
    if (perWave > kLdsMax) return 0u;
    return perWave * p.args.wavesPerBlock <= kLdsMax ? p.args.wavesPerBlock : 1u;
}
size_t dpx_plan_scoretab_lds(const dpx_plan &p) { return (size_t)p.args.ldsPerWave + DPX_SUBST_IMAGE_BYTES; }
size_t dpx_plan_scoretab_lanes_lds(const dpx_plan &p) { return p.lanePacked ? (size_t)p.pkArgs.ldsPerWave + DPX_SUBST_IMAGE_BYTES : 0; }
bool dpx_plan_scoretab_fits(const dpx_plan &p, std::string &err) {
    char text[160];
    if ((!p.lanePacked || p.args.numPairs > 0) && dpx_plan_scoretab_waves(p) == 0u) {
        snprintf(text, sizeof text, "score table: one wave's LDS slice with the table image (%zu bytes) exceeds a workgroup's %zu", dpx_plan_scoretab_lds(p), kLdsMax);
        err = text;
        return false;
    }
    if (dpx_plan_scoretab_lanes_lds(p) * (DPX_ALANES_THREADS / 64) > kLdsMax) {
        snprintf(text, sizeof text, "score table: a lane-packed wave's LDS with the table image (%zu bytes) exceeds a workgroup's %zu", dpx_plan_scoretab_lanes_lds(p), kLdsMax);
        err = text;
        return false;
    }
    return true;
}

const char *dpx_route_kernel_name(dpx_fill_kernel k) {
    /* (the table below names the kernels a created batch can run, each with a case in tests/layout_cases.py; the one that only
     * dpx_batch_set_local_direction_table brings is named here, its layout case is in tests/test_gpu_bdlt.py) */
    if (k == DPX_K_BDLT_FILL) return "k_bdlt_fill";
    if (k == DPX_K_LB2_FILL) return "k_lb2_fill"; /* (DPX_LOCAL_TWO_PIECE_GAPS; its layout cases are in tests/test_gpu_lb2.py) */
    if (k == DPX_K_BSCORE_FILL) return "k_bscore_fill"; /* (DPX_LONG_SCORES; their layout cases are in tests/test_gpu_bscore.py) */
    if (k == DPX_K_LSCORE_FILL) return "k_lscore_fill";
    static const char *const names[DPX_K_COUNT] = {
        "k_linear_fill", "k_linear_fill_pk", "k_linear_lanes", "k_linear_lanes_pk", "k_linear_split",
        "k_affine_fill", "k_asw_fill", "k_asg_fill", "k_affine_lanes", "k_asw_lanes", "k_asg_lanes",
        "k_banded_fill", "k_banded_fill_pk", "k_basw_fill", "k_banw_fill", "k_baxt_fill",
        "k_zext_fill", "k_subst_fill", "k_zsub_fill", "k_bdir_fill", "k_bdx_fill", "k_bd2_fill",
        "k_linear_dir", "k_affine_dir", "k_asw_dir", "k_asg_dir", "k_bdl_fill"};
    return k >= 0 && k < DPX_K_COUNT ? names[k] : "?";
}

const char *dpx_route_walk_name(dpx_walk_family walk, int walkMode) {
    const bool wave = walkMode == 2;
    switch (walk) {
    case DPX_WALK_PLAIN: return wave ? "k_traceback_wave" : "k_traceback";
    case DPX_WALK_DIR: return "k_traceback_dir";
    case DPX_WALK_BASW: return wave ? "k_basw_traceback_wave" : "k_basw_traceback";
    case DPX_WALK_BANW: return wave ? "k_banw_traceback_wave" : "k_banw_traceback";
    case DPX_WALK_SUBST: return wave ? "k_subst_traceback_wave" : "k_subst_traceback";
    case DPX_WALK_BDIR: return "k_bdir_traceback";
    case DPX_WALK_BD2: return "k_bd2_traceback";
    case DPX_WALK_BDL: return "k_bdl_traceback";
    case DPX_WALK_LB2: return "k_lb2_traceback";
    }
    return "?";
}

int dpx_plan_describe(const dpx_plan &b, int tbWalk, int zdrop, int endBonus, int substAlphabet, char *buf, size_t cap) {
    const dpx_route r = dpx_plan_route(b, tbWalk, zdrop, endBonus, substAlphabet);
    const bool extension = r.ext && (zdrop >= 0 || endBonus >= 0);
    auto name = [](int algo) -> const char * { /* (sparse: 8 and 9 are unassigned) */
        static const char *names[] = {"LNW", "LSW", "ANW", "BSW", "ASW", "BASW", "ASG", "BANW"};
        return algo == DPX_ALGO_BAXT ? "BAXT" : (algo >= 0 && algo <= DPX_ALGO_BANW) ? names[algo] : "?";
    };
    /* dtype = the arithmetic type of the kernel that fills (most of) the batch */
    int len = snprintf(buf, cap, "algo=%s kernel_algo=%s kernel=%s dtype=%s rows_per_lane=%d store=%d couples=%zu lane_pairs=%zu waves=%zu singles=%zu row_tags=%d seq_input=%s waves_per_workgroup=%u",
                       name(b.prm.algo), name(b.kernelAlgo), dpx_route_kernel_name(r.kernel), (b.packed || b.lanesPk) ? "int16" : "int32", b.R, b.store ? 1 : 0, b.nCouples, b.nLanePairs,
                       b.nWaves, b.nSingles, (int)b.pkArgs.rowTags, b.packed2 ? "packed2" : "bytes",
                       b.dirs ? (r.dirTable ? dpx_plan_dirtab_waves(b) : b.dirArgs.wavesPerBlock) : (b.packed || b.lanePacked) ? b.pkArgs.wavesPerBlock : b.split ? (unsigned)b.splitWaves : b.bandDirs ? dpx_plan_bdx_waves(b, substAlphabet != 0) : r.scoreTable ? dpx_plan_scoretab_waves(b) : b.args.wavesPerBlock);
    if ((is_banded_affine(b.kernelAlgo) || b.bandLocal) && !b.bandScores && len > 0 && (size_t)len < cap) /* which walk the batch's traceback takes (DPX_LONG_SCORES: none) */
        len += snprintf(buf + len, cap - (size_t)len, " traceback=%s", dpx_route_walk_name(r.walk, r.walkMode));
    if (extension && len > 0 && (size_t)len < cap)
        len += snprintf(buf + len, cap - (size_t)len, " zdrop=%d end_bonus=%d", (int)zdrop, (int)endBonus);
    if (substAlphabet && len > 0 && (size_t)len < cap) len += snprintf(buf + len, cap - (size_t)len, " subst=%d", substAlphabet);
    if (b.bandDirs && !b.bandScores && len > 0 && (size_t)len < cap) len += snprintf(buf + len, cap - (size_t)len, b.twoPiece ? " matrix=banddir8" : " matrix=banddir4");
    if (b.twoPiece && len > 0 && (size_t)len < cap) len += snprintf(buf + len, cap - (size_t)len, " gap2=%d,%d", (int)b.gapOpen2, (int)b.gapExtend2);
    if (b.dirs && len > 0 && (size_t)len < cap) /* the code layout, and where the edge rows live */
        len += snprintf(buf + len, cap - (size_t)len, " matrix=dir4 dir_edges=%s dir_scratch_bytes=%zu", b.dirScratch ? "global" : "lds", b.dirScratch);
    return len;
}
