/* dpx_cigar_kernels.hip -- the batch's traceback lines, run-length encoded on the device: one dpx_alignment record per pair and one
 * packed array of CIGAR ops for the whole batch (dpx_batch_cigars_begin / _end, include/dpx_align.h).
 *
 * Input is the traceback-lines contract every walk kernel of every algorithm and storage mode meets: tbOff[p] is the byte offset of
 * pair p's three lines (reference, relation, query) in `tb`, each line has a capacity of cap = (m + n + 1 + 3) & ~3 bytes and holds
 * its tbLen[p] characters right-aligned.  `tb` is 256-byte aligned and every tbOff and cap is a multiple of 4, so the relation and the
 * query line start at the same offset modulo 4 and the aligned dwords that cover them lie inside the pair's own capacity.
 *
 * A column is classified from its relation and query character ('*' -> '=', '|' -> 'X', otherwise a gap: query '_' -> 'D', anything
 * else -> 'I'); the reference line is never read.  One wave per pair walks the two lines in trips of 256 columns, one aligned dword
 * of each line per lane, so every load instruction of the wave covers 256 contiguous bytes.  A column starts a run when its class
 * differs from the class of the column before it (the first column always does; the last class of a trip is carried into the next).
 *
 *   k_cigar_count   class counts and number of run starts per pair (ballots + popcounts) -> every field of the record but opsOffset
 *   k_cigar_scan    opsOffset = exclusive prefix of numOps over the pairs, and the total (the tile scheme of k_out_scan)
 *   k_cigar_write   the same pass again: the lane that holds a run start writes op number (run starts before it), its length is the
 *                   distance to the next run start; the last run of a trip stays open in wave-uniform registers (class, first
 *                   column, op index) and is written when the next run start is seen or the line ends
 *
 * No LDS in the two line kernels, no atomics, no scratch; every op is written exactly once with a plain vector store. */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpx_cigar.h"
#include "dpx_device.hpp"

namespace {

using namespace dpx_dev;

constexpr int kCigarThreads = 256;                  /* four independent waves per workgroup, one pair each (as k_out_compact) */
constexpr int kTripCols = 4 * DPX_WAVE;             /* one dword per lane */
constexpr int kNoClass = 0xFF;                      /* "no column before this one" */

/* classes, in the order of the record's counters */
constexpr int kEq = 0, kX = 1, kDel = 2, kIns = 3, kM = 4;
/* BAM op code of a run class: '=' 7, 'X' 8, 'D' 2, 'I' 1, 'M' 0 -- one nibble per class */
__device__ __forceinline__ uint32_t cigar_op(int runClass, int length) {
    return ((uint32_t)length << 4) | ((0x01287u >> (4 * runClass)) & 0xFu);
}

/* the relation and the query line of one pair (wave-uniform): aligned dwords, `skew` bytes in front of column 0 in dword 0 */
struct CigarLines {
    const uint32_t *rel, *qry;
    int skew, len;
};

__device__ __forceinline__ CigarLines cigar_lines(const dpx_pair_dev *pairs, const int32_t *tbLen, const uint64_t *tbOff, const char *tb, int p) {
    CigarLines L;
    L.len = tbLen[p];
    const int cap = (pairs[p].m + pairs[p].n + 1 + 3) & ~3; /* line capacity, as in k_traceback */
    const int lead = cap - L.len;                           /* the lines are right-aligned */
    L.skew = lead & 3;
    const char *rel = tb + tbOff[p] + (size_t)cap + (size_t)(lead & ~3);
    L.rel = reinterpret_cast<const uint32_t *>(rel);
    L.qry = reinterpret_cast<const uint32_t *>(rel + cap);
    return L;
}

/* One trip: this lane's four columns.  cls[k]: class of column k for the counters (-1: not a column of the alignment); rc[k]: its
 * class for run purposes ('=' and 'X' are one class under DPX_CIGAR_M); st[k]: the column starts a run.  `carry` is the run class
 * of the last column of the trip before (kNoClass in front of trip 0) and is replaced by this trip's. */
__device__ __forceinline__ void cigar_trip(const CigarLines &L, int t, int lane, bool mergeM, int &carry, int cls[4], int rc[4], bool st[4]) {
    const int d = t * DPX_WAVE + lane; /* the dword of the lines this lane holds */
    const int c0 = d * 4 - L.skew;     /* column of its first byte */
    uint32_t w = 0, q = 0;
    if (d * 4 < L.skew + L.len) { w = L.rel[d]; q = L.qry[d]; } /* (skew + len is a multiple of 4: the dword ends inside the line) */
    bool valid[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int c = c0 + k;
        const uint32_t r = (w >> (8 * k)) & 0xFFu, y = (q >> (8 * k)) & 0xFFu;
        const int cl = r == (uint32_t)'*' ? kEq : r == (uint32_t)'|' ? kX : y == (uint32_t)'_' ? kDel : kIns;
        valid[k] = c >= 0 && c < L.len;
        cls[k] = valid[k] ? cl : -1;
        rc[k] = c < 0 ? kNoClass : (mergeM && cl <= kX) ? kM : cl;
    }
    int prev = __shfl_up(rc[3], 1, DPX_WAVE);
    if (lane == 0) prev = carry;
    st[0] = valid[0] && rc[0] != prev;
#pragma unroll
    for (int k = 1; k < 4; k++) st[k] = valid[k] && rc[k] != rc[k - 1];
    carry = __shfl(rc[3], DPX_WAVE - 1, DPX_WAVE); /* (read only when another trip follows: then it is a column of the alignment) */
}

__global__ void __launch_bounds__(kCigarThreads) k_cigar_count(const dpx_pair_dev *pairs, const int32_t *endRow, const int32_t *endCol,
                                                               const int32_t *tbLen, const uint64_t *tbOff, const char *tb, int numPairs,
                                                               unsigned flags, dpx_alignment *records) {
    const int lane = threadIdx.x & 63;
    const int p = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kCigarThreads / DPX_WAVE) + (threadIdx.x >> 6)));
    if (p >= numPairs) return;
    const CigarLines L = cigar_lines(pairs, tbLen, tbOff, tb, p);
    const bool mergeM = (flags & DPX_CIGAR_M) != 0;
    int count[4] = {0, 0, 0, 0}, starts = 0, carry = kNoClass;
    const int trips = (L.skew + L.len + kTripCols - 1) / kTripCols;
    for (int t = 0; t < trips; t++) {
        int cls[4], rc[4];
        bool st[4];
        cigar_trip(L, t, lane, mergeM, carry, cls, rc, st);
#pragma unroll
        for (int k = 0; k < 4; k++) {
#pragma unroll
            for (int c = 0; c < 4; c++) count[c] += __popcll(__ballot(cls[k] == c));
            starts += __popcll(__ballot(st[k]));
        }
    }
    if (lane == 0) {
        dpx_alignment &r = records[p];
        const int refEnd = endCol[p], qryEnd = endRow[p];
        r.numOps = starts;
        r.refStart = refEnd - (count[kEq] + count[kX] + count[kDel]);
        r.refEnd = refEnd;
        r.qryStart = qryEnd - (count[kEq] + count[kX] + count[kIns]);
        r.qryEnd = qryEnd;
        r.matches = count[kEq];
        r.mismatches = count[kX];
        r.insertions = count[kIns];
        r.deletions = count[kDel];
        r.reserved = 0;
    }
}

__global__ void __launch_bounds__(kCigarThreads) k_cigar_write(const dpx_pair_dev *pairs, const int32_t *tbLen, const uint64_t *tbOff,
                                                               const char *tb, int numPairs, unsigned flags, const dpx_alignment *records,
                                                               uint32_t *ops) {
    const int lane = threadIdx.x & 63;
    const int p = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kCigarThreads / DPX_WAVE) + (threadIdx.x >> 6)));
    if (p >= numPairs) return;
    const CigarLines L = cigar_lines(pairs, tbLen, tbOff, tb, p);
    if (L.len <= 0) return; /* an empty alignment has no ops */
    const bool mergeM = (flags & DPX_CIGAR_M) != 0;
    uint32_t *dst = ops + records[p].opsOffset;
    int carry = kNoClass;
    int seen = 0;                            /* run starts in the trips before this one */
    int openClass = 0, openCol = 0, openOp = -1; /* the run that was still open at the end of the trip before (wave-uniform) */
    const int trips = (L.skew + L.len + kTripCols - 1) / kTripCols;
    for (int t = 0; t < trips; t++) {
        int cls[4], rc[4];
        bool st[4];
        cigar_trip(L, t, lane, mergeM, carry, cls, rc, st);
        const unsigned long long S0 = __ballot(st[0]), S1 = __ballot(st[1]), S2 = __ballot(st[2]), S3 = __ballot(st[3]);
        const unsigned long long any = S0 | S1 | S2 | S3;
        if (any == 0) continue; /* (wave-uniform) the open run covers the whole trip */
        const int tripCol = t * kTripCols - L.skew; /* column of lane 0's first byte */
        /* the first run start of the trip ends the open run */
        const int fl = __builtin_ctzll(any);
        const int fk = ((S0 >> fl) & 1) ? 0 : ((S1 >> fl) & 1) ? 1 : ((S2 >> fl) & 1) ? 2 : 3;
        if (openOp >= 0 && lane == 0) dst[openOp] = cigar_op(openClass, tripCol + fl * 4 + fk - openCol);
        /* every run start but the last of the trip: its run ends at the next start, in this lane or in the next lane that has one */
        const unsigned long long below = (1ull << lane) - 1ull, above = any & ~((2ull << lane) - 1ull);
        int next = -1;
        if (above) {
            const int nl = __builtin_ctzll(above);
            const int nk = ((S0 >> nl) & 1) ? 0 : ((S1 >> nl) & 1) ? 1 : ((S2 >> nl) & 1) ? 2 : 3;
            next = tripCol + nl * 4 + nk;
        }
        const int myCol = tripCol + lane * 4;
        int r = seen + __popcll(S0 & below) + __popcll(S1 & below) + __popcll(S2 & below) + __popcll(S3 & below) + (int)st[0] + (int)st[1] +
                (int)st[2] + (int)st[3]; /* op index behind this lane's run starts */
#pragma unroll
        for (int k = 3; k >= 0; k--)
            if (st[k]) {
                r--;
                if (next >= 0) dst[r] = cigar_op(rc[k], next - (myCol + k));
                next = myCol + k;
            }
        /* the last run start of the trip opens the run that is carried on */
        const int ll = 63 - __builtin_clzll(any);
        const int lk = ((S3 >> ll) & 1) ? 3 : ((S2 >> ll) & 1) ? 2 : ((S1 >> ll) & 1) ? 1 : 0;
        const uint32_t packed = (uint32_t)rc[0] | ((uint32_t)rc[1] << 8) | ((uint32_t)rc[2] << 16) | ((uint32_t)rc[3] << 24);
        openClass = (int)((__shfl(packed, ll, DPX_WAVE) >> (8 * lk)) & 0xFFu);
        openCol = tripCol + ll * 4 + lk;
        seen += __popcll(S0) + __popcll(S1) + __popcll(S2) + __popcll(S3);
        openOp = seen - 1;
    }
    if (lane == 0 && openOp >= 0) dst[openOp] = cigar_op(openClass, L.len - openCol); /* the line ends: so does the last run */
}

/* ---- exclusive prefix of numOps over the pairs: the tile scheme of k_out_scan / k_out_scan_tiles (dpx_output_kernels.hip); the scan
 * itself is dpx_device.hpp's ---- */

/* phase 1: per-tile totals of numOps; phase 3 (FINAL): opsOffset = tile base + exclusive prefix, and the batch's total.  A batch of
 * one tile runs phase 3 alone (tileSums == nullptr: its base is 0). */
template <bool FINAL>
__global__ void __launch_bounds__(kScanThreads) k_cigar_scan(dpx_alignment *records, int numPairs, unsigned long long *tileSums,
                                                             unsigned long long *totalOps) {
    __shared__ unsigned long long lds[kScanThreads / 64];
    const size_t base = (size_t)blockIdx.x * kScanTile + (size_t)threadIdx.x * kScanPerThread;
    unsigned long long v[kScanPerThread], mine = 0;
#pragma unroll
    for (int k = 0; k < kScanPerThread; k++) {
        const size_t p = base + k;
        v[k] = p < (size_t)numPairs ? (unsigned long long)records[p].numOps : 0ull;
        mine += v[k];
    }
    unsigned long long total;
    unsigned long long ex = group_exclusive(mine, lds, &total);
    if constexpr (!FINAL) {
        if (threadIdx.x == 0) tileSums[blockIdx.x] = total;
    } else {
        if (tileSums) ex += tileSums[blockIdx.x]; /* exclusive prefix of the tiles, from k_cigar_scan_tiles */
#pragma unroll
        for (int k = 0; k < kScanPerThread; k++) {
            const size_t p = base + k;
            if (p < (size_t)numPairs) records[p].opsOffset = ex;
            ex += v[k];
        }
        if (blockIdx.x == gridDim.x - 1 && threadIdx.x == kScanThreads - 1) *totalOps = ex;
    }
}

/* phase 2: exclusive scan of the tile totals, in place (one workgroup; numTiles is small: pairs / 2048) */
__global__ void __launch_bounds__(kScanThreads) k_cigar_scan_tiles(unsigned long long *tileSums, int numTiles) {
    __shared__ unsigned long long lds[kScanThreads / 64];
    unsigned long long carry = 0;
    for (int t0 = 0; t0 < numTiles; t0 += kScanThreads) {
        const int t = t0 + (int)threadIdx.x;
        const unsigned long long v = t < numTiles ? tileSums[t] : 0ull;
        unsigned long long total;
        const unsigned long long ex = group_exclusive(v, lds, &total);
        if (t < numTiles) tileSums[t] = carry + ex;
        carry += total;
    }
}

} // namespace

size_t dpx_cigar_scan_tiles(size_t numPairs) { return (numPairs + kScanTile - 1) / kScanTile; }

hipError_t dpx_launch_cigars(const dpx_pair_dev *pairs, const int32_t *endRow, const int32_t *endCol, const int32_t *tbLen,
                             const uint64_t *tbOff, const char *tb, int numPairs, unsigned flags, dpx_alignment *records,
                             unsigned long long *tileSums, unsigned long long *total, uint32_t *ops, hipStream_t stream) {
    if (numPairs <= 0) return hipSuccess;
    const dim3 perPair((unsigned)((numPairs + kCigarThreads / DPX_WAVE - 1) / (kCigarThreads / DPX_WAVE)));
    const int tiles = (int)dpx_cigar_scan_tiles((size_t)numPairs);
    hipLaunchKernelGGL(k_cigar_count, perPair, dim3(kCigarThreads), 0, stream, pairs, endRow, endCol, tbLen, tbOff, tb, numPairs, flags, records);
    if (tiles == 1) {
        hipLaunchKernelGGL(k_cigar_scan<true>, dim3(1), dim3(kScanThreads), 0, stream, records, numPairs, (unsigned long long *)nullptr, total);
    } else {
        hipLaunchKernelGGL(k_cigar_scan<false>, dim3(tiles), dim3(kScanThreads), 0, stream, records, numPairs, tileSums, total);
        hipLaunchKernelGGL(k_cigar_scan_tiles, dim3(1), dim3(kScanThreads), 0, stream, tileSums, tiles);
        hipLaunchKernelGGL(k_cigar_scan<true>, dim3(tiles), dim3(kScanThreads), 0, stream, records, numPairs, tileSums, total);
    }
    hipLaunchKernelGGL(k_cigar_write, perPair, dim3(kCigarThreads), 0, stream, pairs, tbLen, tbOff, tb, numPairs, flags, records, ops);
    return hipGetLastError();
}
