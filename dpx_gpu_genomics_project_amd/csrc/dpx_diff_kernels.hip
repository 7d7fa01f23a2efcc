/* dpx_diff_kernels.hip -- the batch's traceback lines as SAM's MD string or minimap2's short cs string per pair, built on the device:
 * one packed text buffer per kind for the whole batch and numPairs + 1 byte offsets (dpx_batch_diffs_begin / _end,
 * include/dpx_align.h states both formats and the length bound).
 *
 * Input is the traceback-lines contract of dpx_cigar_kernels.hip: three right-aligned lines per pair in a capacity of
 * cap = (m + n + 1 + 3) & ~3 each, so the aligned dwords that cover the same columns of the three lines lie inside the pair's own
 * capacity.  Columns are classified as the CIGAR kernels classify them.  One wave per pair walks the lines in trips of 256 columns,
 * one aligned dword of each line per lane: lane l holds columns 4l .. 4l + 3 of the trip (lane-major).
 *
 * Both formats are "a number in front of a breaker".  A breaker is an X or D column for MD and any column that is not '=' for cs; the
 * number is n = the '=' columns since the breaker before (for cs: the length of the '=' run that ends here, printed only if > 0).
 * Inside a trip, n in front of a lane's first column comes from ballots: ('=' columns in lower lanes) - ('=' columns up to the last
 * breaker in lower lanes); with no breaker below, the count carried from the trips before is added.  The lane then steps through its
 * four columns in order (diff_walk), which gives its byte count; a wave exclusive prefix sum of the counts (__shfl_up steps) gives its
 * output position, and the same walk again stores the bytes.  Three wave-uniform values are carried across trips: n, the class of the
 * last column and the output position.  The closing number (MD) or the last ":L" (cs) is lane 0's, behind the loop.
 *
 *   k_diff_count<KIND>   the pair's byte length -> offsets[p]
 *   k_diff_scan          exclusive prefix of the lengths, in place, offsets[numPairs] = the total (the tile scheme of k_cigar_scan)
 *   k_diff_write<KIND>   the same pass again; every byte is stored exactly once, by the lane that owns its column
 *
 * No LDS in the two line kernels, no atomics, no scratch, plain byte stores: the strings are a small fraction of the lines read. */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpx_device.hpp"
#include "dpx_diff.h"

namespace {

using namespace dpx_dev;

constexpr int kDiffThreads = 256;                   /* four independent waves per workgroup, one pair each (as k_cigar_count) */
constexpr int kTripCols = 4 * DPX_WAVE;             /* one dword per lane */
constexpr int kEq = 0, kX = 1, kDel = 2, kIns = 3;  /* column classes, in the order of the record's counters */
constexpr int kNone = 0xFF;                         /* not a column of the alignment / no column before this one */
constexpr int MD = (int)DPX_DIFF_MD, CS = (int)DPX_DIFF_CS;

/* the three lines of one pair (wave-uniform): aligned dwords, `skew` bytes in front of column 0 in dword 0 */
struct DiffLines {
    const uint32_t *ref, *rel, *qry;
    int skew, len;
};

__device__ __forceinline__ DiffLines diff_lines(const dpx_pair_dev *pairs, const int32_t *tbLen, const uint64_t *tbOff, const char *tb, int p) {
    DiffLines L;
    L.len = tbLen[p];
    const int cap = (pairs[p].m + pairs[p].n + 1 + 3) & ~3; /* line capacity, as in k_traceback */
    const int lead = cap - L.len;                           /* the lines are right-aligned */
    L.skew = lead & 3;
    const char *ref = tb + tbOff[p] + (size_t)(lead & ~3);
    L.ref = reinterpret_cast<const uint32_t *>(ref);
    L.rel = reinterpret_cast<const uint32_t *>(ref + cap);
    L.qry = reinterpret_cast<const uint32_t *>(ref + 2 * (size_t)cap);
    return L;
}

/* digits of decimal(n), by a compare chain */
__device__ __forceinline__ uint32_t digits(uint32_t n) {
    return n < 10u ? 1u : n < 100u ? 2u : n < 1000u ? 3u : n < 10000u ? 4u : n < 100000u ? 5u : n < 1000000u ? 6u : n < 10000000u ? 7u
           : n < 100000000u ? 8u : n < 1000000000u ? 9u : 10u;
}

__device__ __forceinline__ uint32_t lc(uint32_t b) { return b - (uint32_t)'A' < 26u ? b + 32u : b; }

template <bool WRITE>
__device__ __forceinline__ void put(unsigned char *dst, uint32_t &pos, uint32_t byte) {
    if constexpr (WRITE) dst[pos] = (unsigned char)byte;
    pos++;
}

template <bool WRITE>
__device__ __forceinline__ void put_num(unsigned char *dst, uint32_t &pos, uint32_t n) {
    const uint32_t d = digits(n);
    if constexpr (WRITE) {
        uint32_t v = n;
        for (int i = (int)d - 1; i >= 0; i--) { dst[pos + (uint32_t)i] = (unsigned char)('0' + v % 10u); v /= 10u; }
    }
    pos += d;
}

/* what a lane knows about its four columns of one trip: the classes (kNone: not a column of the alignment), the reference and query
 * dwords, and the state in front of its first column: the class of the column before (kNone: none) and n */
struct DiffTrip {
    int cls[4];
    uint32_t r, q;
    int prev;
    uint32_t n;
};

/* One trip.  carryCls: class of the last column of the trip before (kNone in front of trip 0), replaced by this trip's; carryN: n
 * at the start of the trip (the caller replaces it with lane 63's n behind its walk). */
template <int KIND>
__device__ __forceinline__ void diff_trip(const DiffLines &L, int t, int lane, int &carryCls, uint32_t carryN, DiffTrip &T) {
    const int d = t * DPX_WAVE + lane; /* the dword of the lines this lane holds */
    const int c0 = d * 4 - L.skew;     /* column of its first byte */
    uint32_t w = 0;
    T.r = 0;
    T.q = 0;
    if (d * 4 < L.skew + L.len) { w = L.rel[d]; T.q = L.qry[d]; T.r = L.ref[d]; } /* (skew + len is a multiple of 4: the dword ends inside the line) */
    bool eq[4], br[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int c = c0 + k;
        const uint32_t r = (w >> (8 * k)) & 0xFFu, y = (T.q >> (8 * k)) & 0xFFu;
        const int cl = r == (uint32_t)'*' ? kEq : r == (uint32_t)'|' ? kX : y == (uint32_t)'_' ? kDel : kIns;
        T.cls[k] = (c >= 0 && c < L.len) ? cl : kNone;
        eq[k] = T.cls[k] == kEq;
        br[k] = KIND == MD ? (T.cls[k] == kX || T.cls[k] == kDel) : (T.cls[k] >= kX && T.cls[k] <= kIns);
    }
    T.prev = __shfl_up(T.cls[3], 1, DPX_WAVE);
    if (lane == 0) T.prev = carryCls;
    carryCls = __shfl(T.cls[3], DPX_WAVE - 1, DPX_WAVE); /* (read only when another trip follows: then it is a column of the alignment) */
    /* n in front of this lane's first column, from ballots over the lanes below */
    const unsigned long long E0 = __ballot(eq[0]), E1 = __ballot(eq[1]), E2 = __ballot(eq[2]), E3 = __ballot(eq[3]);
    const unsigned long long B0 = __ballot(br[0]), B1 = __ballot(br[1]), B2 = __ballot(br[2]), B3 = __ballot(br[3]);
    const unsigned long long below = (1ull << lane) - 1ull;
    const uint32_t eqBelow = (uint32_t)(__popcll(E0 & below) + __popcll(E1 & below) + __popcll(E2 & below) + __popcll(E3 & below));
    const unsigned long long brBelow = (B0 | B1 | B2 | B3) & below;
    if (brBelow == 0) {
        T.n = carryN + eqBelow;
    } else {
        const int hl = 63 - __builtin_clzll(brBelow); /* the last lane below with a breaker, and its last breaker hk */
        const int hk = ((B3 >> hl) & 1) ? 3 : ((B2 >> hl) & 1) ? 2 : ((B1 >> hl) & 1) ? 1 : 0;
        const unsigned long long upTo = (1ull << hl) - 1ull;
        uint32_t eqAt = (uint32_t)(__popcll(E0 & upTo) + __popcll(E1 & upTo) + __popcll(E2 & upTo) + __popcll(E3 & upTo)); /* '=' columns in front of it */
        if (hk > 0) eqAt += (uint32_t)((E0 >> hl) & 1);
        if (hk > 1) eqAt += (uint32_t)((E1 >> hl) & 1);
        if (hk > 2) eqAt += (uint32_t)((E2 >> hl) & 1);
        T.n = eqBelow - eqAt;
    }
}

/* The lane's four columns in order, from the state (T.prev, n): returns the bytes they emit and stores them at dst[0 ..) when WRITE;
 * n is left as it stands behind the lane's last column. */
template <int KIND, bool WRITE>
__device__ __forceinline__ uint32_t diff_walk(const DiffTrip &T, uint32_t &n, unsigned char *dst) {
    uint32_t pos = 0;
    int prev = T.prev;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int c = T.cls[k];
        if (c == kNone) continue;
        const uint32_t rb = (T.r >> (8 * k)) & 0xFFu, qb = (T.q >> (8 * k)) & 0xFFu;
        if (c == kEq) {
            n++;
        } else if constexpr (KIND == MD) {
            if (c == kX) {
                put_num<WRITE>(dst, pos, n);
                put<WRITE>(dst, pos, rb);
                n = 0;
            } else if (c == kDel) {
                if (prev != kDel) {
                    put_num<WRITE>(dst, pos, n);
                    put<WRITE>(dst, pos, (uint32_t)'^');
                }
                put<WRITE>(dst, pos, rb);
                n = 0;
            } /* an insertion emits nothing and leaves n alone */
        } else {
            if (n > 0) {
                put<WRITE>(dst, pos, (uint32_t)':');
                put_num<WRITE>(dst, pos, n);
                n = 0;
            }
            if (c == kX) {
                put<WRITE>(dst, pos, (uint32_t)'*');
                put<WRITE>(dst, pos, lc(rb));
                put<WRITE>(dst, pos, lc(qb));
            } else {
                if (prev != c) put<WRITE>(dst, pos, c == kIns ? (uint32_t)'+' : (uint32_t)'-');
                put<WRITE>(dst, pos, lc(c == kIns ? qb : rb));
            }
        }
        prev = c;
    }
    return pos;
}

/* what follows the last column: MD's closing number, cs's last '=' run */
template <int KIND, bool WRITE>
__device__ __forceinline__ uint32_t diff_close(uint32_t n, unsigned char *dst) {
    uint32_t pos = 0;
    if constexpr (KIND == MD) {
        put_num<WRITE>(dst, pos, n);
    } else if (n > 0) {
        put<WRITE>(dst, pos, (uint32_t)':');
        put_num<WRITE>(dst, pos, n);
    }
    return pos;
}

template <int KIND>
__global__ void __launch_bounds__(kDiffThreads) k_diff_count(const dpx_pair_dev *pairs, const int32_t *tbLen, const uint64_t *tbOff, const char *tb,
                                                             int numPairs, unsigned long long *offsets) {
    const int lane = threadIdx.x & 63;
    const int p = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kDiffThreads / DPX_WAVE) + (threadIdx.x >> 6)));
    if (p >= numPairs) return;
    const DiffLines L = diff_lines(pairs, tbLen, tbOff, tb, p);
    int carryCls = kNone;
    uint32_t carryN = 0;
    unsigned long long mine = 0;
    const int trips = (L.skew + L.len + kTripCols - 1) / kTripCols;
    for (int t = 0; t < trips; t++) {
        DiffTrip T;
        diff_trip<KIND>(L, t, lane, carryCls, carryN, T);
        uint32_t n = T.n;
        mine += diff_walk<KIND, false>(T, n, nullptr);
        carryN = __shfl(n, DPX_WAVE - 1, DPX_WAVE);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, DPX_WAVE);
    if (lane == 0) offsets[p] = mine + diff_close<KIND, false>(carryN, nullptr);
}

template <int KIND>
__global__ void __launch_bounds__(kDiffThreads) k_diff_write(const dpx_pair_dev *pairs, const int32_t *tbLen, const uint64_t *tbOff, const char *tb,
                                                             int numPairs, const unsigned long long *offsets, char *text) {
    const int lane = threadIdx.x & 63;
    const int p = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kDiffThreads / DPX_WAVE) + (threadIdx.x >> 6)));
    if (p >= numPairs) return;
    const DiffLines L = diff_lines(pairs, tbLen, tbOff, tb, p);
    unsigned char *dst = reinterpret_cast<unsigned char *>(text) + offsets[p]; /* (wave-uniform) the output position, carried across the trips */
    int carryCls = kNone;
    uint32_t carryN = 0;
    const int trips = (L.skew + L.len + kTripCols - 1) / kTripCols;
    for (int t = 0; t < trips; t++) {
        DiffTrip T;
        diff_trip<KIND>(L, t, lane, carryCls, carryN, T);
        uint32_t n = T.n;
        const uint32_t bytes = diff_walk<KIND, false>(T, n, nullptr);
        uint32_t incl = bytes; /* inclusive prefix sum of the lanes' byte counts */
#pragma unroll
        for (int off = 1; off < DPX_WAVE; off <<= 1) {
            const uint32_t o = __shfl_up(incl, off, DPX_WAVE);
            if (lane >= off) incl += o;
        }
        uint32_t again = T.n;
        if (bytes) diff_walk<KIND, true>(T, again, dst + (incl - bytes));
        dst += __shfl(incl, DPX_WAVE - 1, DPX_WAVE);
        carryN = __shfl(n, DPX_WAVE - 1, DPX_WAVE);
    }
    if (lane == 0) diff_close<KIND, true>(carryN, dst);
}

/* ---- exclusive prefix of the lengths over the pairs, in place: the tile scheme of k_cigar_scan / k_out_scan; the scan itself is
 * dpx_device.hpp's ---- */

/* phase 1: per-tile totals; phase 3 (FINAL): offsets[p] = tile base + exclusive prefix, offsets[numPairs] = the total.  Every thread
 * reads its own eight lengths before it overwrites them.  A batch of one tile runs phase 3 alone (tileSums == nullptr: its base is 0). */
template <bool FINAL>
__global__ void __launch_bounds__(kScanThreads) k_diff_scan(unsigned long long *offsets, int numPairs, unsigned long long *tileSums) {
    __shared__ unsigned long long lds[kScanThreads / 64];
    const size_t base = (size_t)blockIdx.x * kScanTile + (size_t)threadIdx.x * kScanPerThread;
    unsigned long long v[kScanPerThread], mine = 0;
#pragma unroll
    for (int k = 0; k < kScanPerThread; k++) {
        const size_t p = base + k;
        v[k] = p < (size_t)numPairs ? offsets[p] : 0ull;
        mine += v[k];
    }
    unsigned long long total;
    unsigned long long ex = group_exclusive(mine, lds, &total);
    if constexpr (!FINAL) {
        if (threadIdx.x == 0) tileSums[blockIdx.x] = total;
    } else {
        if (tileSums) ex += tileSums[blockIdx.x]; /* exclusive prefix of the tiles, from k_diff_scan_tiles */
#pragma unroll
        for (int k = 0; k < kScanPerThread; k++) {
            const size_t p = base + k;
            if (p < (size_t)numPairs) offsets[p] = ex;
            ex += v[k];
        }
        if (blockIdx.x == gridDim.x - 1 && threadIdx.x == kScanThreads - 1) offsets[numPairs] = ex;
    }
}

/* phase 2: exclusive scan of the tile totals, in place (one workgroup; numTiles is small: pairs / 2048) */
__global__ void __launch_bounds__(kScanThreads) k_diff_scan_tiles(unsigned long long *tileSums, int numTiles) {
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

template <int KIND>
hipError_t launch_kind(const dpx_pair_dev *pairs, const int32_t *tbLen, const uint64_t *tbOff, const char *tb, int numPairs,
                       unsigned long long *offsets, unsigned long long *tileSums, char *text, hipStream_t stream) {
    const dim3 perPair((unsigned)((numPairs + kDiffThreads / DPX_WAVE - 1) / (kDiffThreads / DPX_WAVE)));
    const int tiles = (int)dpx_diff_scan_tiles((size_t)numPairs);
    hipLaunchKernelGGL(k_diff_count<KIND>, perPair, dim3(kDiffThreads), 0, stream, pairs, tbLen, tbOff, tb, numPairs, offsets);
    if (tiles == 1) {
        hipLaunchKernelGGL(k_diff_scan<true>, dim3(1), dim3(kScanThreads), 0, stream, offsets, numPairs, (unsigned long long *)nullptr);
    } else {
        hipLaunchKernelGGL(k_diff_scan<false>, dim3(tiles), dim3(kScanThreads), 0, stream, offsets, numPairs, tileSums);
        hipLaunchKernelGGL(k_diff_scan_tiles, dim3(1), dim3(kScanThreads), 0, stream, tileSums, tiles);
        hipLaunchKernelGGL(k_diff_scan<true>, dim3(tiles), dim3(kScanThreads), 0, stream, offsets, numPairs, tileSums);
    }
    hipLaunchKernelGGL(k_diff_write<KIND>, perPair, dim3(kDiffThreads), 0, stream, pairs, tbLen, tbOff, tb, numPairs, (const unsigned long long *)offsets, text);
    return hipGetLastError();
}

} // namespace

size_t dpx_diff_scan_tiles(size_t numPairs) { return (numPairs + kScanTile - 1) / kScanTile; }

hipError_t dpx_launch_diffs(unsigned kind, const dpx_pair_dev *pairs, const int32_t *tbLen, const uint64_t *tbOff, const char *tb,
                            int numPairs, unsigned long long *offsets, unsigned long long *tileSums, char *text, hipStream_t stream) {
    if (kind != DPX_DIFF_MD && kind != DPX_DIFF_CS) return hipErrorInvalidValue;
    if (numPairs <= 0) return hipSuccess;
    return kind == DPX_DIFF_MD ? launch_kind<MD>(pairs, tbLen, tbOff, tb, numPairs, offsets, tileSums, text, stream)
                               : launch_kind<CS>(pairs, tbLen, tbOff, tb, numPairs, offsets, tileSums, text, stream);
}
