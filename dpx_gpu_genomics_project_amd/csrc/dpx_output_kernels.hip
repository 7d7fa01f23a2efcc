/*
 * dpx_output_kernels.hip -- the kernels behind a batch's results that are no fill and no walk: the result text (k_out_scan,
 * k_out_scan_tiles, k_out_compact, k_out_small), the 2-bit sequence expansion (k_unpack2) and the evaluator of the dpx_prims.hpp
 * primitives (k_prim_eval).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpx_device.hpp"
#include "dpx_kernels.h"
#include "dpx_layout.h"
#include "dpx_prims.hpp"

namespace {

using namespace dpx_dev;

/* =====================================================================================================
 * Output path: packed, variable-length result text built on the device -- the reference's V15 idea
 * (cuda/LNW/LinearNeedlemanWunschV15.cu:168-172,372-425: per-pair string lengths, prefix offsets, one packed buffer, one
 * D2H of the real bytes) taken one step further: the device writes each pair's block exactly as c++/main.cpp prints it,
 *     "<pair number> | <score>\n<reference line>\n<relation line>\n<query line>\n"
 * (three empty lines for a zero-score local alignment, c++/LinearSmithWaterman.cpp:253-257), so the host's share of the
 * output is one fwrite per batch.  Three small kernels after k_traceback: block lengths, an exclusive scan, the copy.
 * ===================================================================================================== */
__device__ __forceinline__ int dec_digits(unsigned long long v) {
    int d = 1;
    while (v >= 10ull) { v /= 10ull; d++; }
    return d;
}
__device__ __forceinline__ unsigned long long block_len(unsigned long long number, int score, int len) {
    const unsigned us = score < 0 ? 0u - (unsigned)score : (unsigned)score;
    return (unsigned long long)(dec_digits(number) + 3 + (score < 0 ? 1 : 0) + dec_digits(us) + 1) + 3ull * (unsigned long long)(len + 1);
}

/* phase 1: per-tile totals of the block lengths; phase 3 (FINAL): per-pair offsets = tile base + exclusive prefix */
template <bool FINAL>
__global__ void __launch_bounds__(kScanThreads) k_out_scan(const int32_t *score, const int32_t *tbLen, int numPairs, unsigned long long firstNumber,
                                                           unsigned long long *tileSums, unsigned long long *outOff) {
    __shared__ unsigned long long lds[kScanThreads / 64];
    const size_t base = (size_t)blockIdx.x * kScanTile + (size_t)threadIdx.x * kScanPerThread;
    unsigned long long v[kScanPerThread], mine = 0;
#pragma unroll
    for (int k = 0; k < kScanPerThread; k++) {
        const size_t p = base + k;
        v[k] = p < (size_t)numPairs ? block_len(firstNumber + p, score[p], tbLen[p]) : 0ull;
        mine += v[k];
    }
    unsigned long long total;
    unsigned long long ex = group_exclusive(mine, lds, &total);
    if constexpr (!FINAL) {
        if (threadIdx.x == 0) tileSums[blockIdx.x] = total;
    } else {
        ex += tileSums[blockIdx.x]; /* exclusive prefix of the tiles, from k_out_scan_tiles */
#pragma unroll
        for (int k = 0; k < kScanPerThread; k++) {
            const size_t p = base + k;
            if (p < (size_t)numPairs) outOff[p] = ex;
            ex += v[k];
        }
        if (blockIdx.x == gridDim.x - 1 && threadIdx.x == kScanThreads - 1) outOff[numPairs] = ex; /* total bytes */
    }
}

/* phase 2: exclusive scan of the tile totals, in place (one workgroup; numTiles is small: pairs / 2048) */
__global__ void __launch_bounds__(kScanThreads) k_out_scan_tiles(unsigned long long *tileSums, int numTiles) {
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

/* one pair's block, written by one wave: header by lane 0, the three right-aligned lines of k_traceback copied 64 bytes per instruction */
__device__ __forceinline__ void out_write_block(const dpx_pair_dev *pairs, const int32_t *score, const int32_t *tbLen, const uint64_t *tbOff,
                                                const char *tb, const int p, const int lane, const unsigned long long firstNumber,
                                                const unsigned long long dstOff, char *out) {
    const int len = tbLen[p], sc = score[p];
    const int cap = (pairs[p].m + pairs[p].n + 1 + 3) & ~3; /* line capacity, as in k_traceback */
    char *dst = out + dstOff;
    const unsigned long long number = firstNumber + (unsigned long long)p;
    const unsigned us = sc < 0 ? 0u - (unsigned)sc : (unsigned)sc;
    const int dn = dec_digits(number), ds = dec_digits(us), neg = sc < 0 ? 1 : 0;
    const int hdr = dn + 3 + neg + ds + 1;
    if (lane == 0) {
        unsigned long long v = number;
        for (int k = dn - 1; k >= 0; k--) { dst[k] = (char)('0' + (int)(v % 10ull)); v /= 10ull; }
        dst[dn] = ' '; dst[dn + 1] = '|'; dst[dn + 2] = ' ';
        if (neg) dst[dn + 3] = '-';
        unsigned u = us;
        for (int k = ds - 1; k >= 0; k--) { dst[dn + 3 + neg + k] = (char)('0' + (int)(u % 10u)); u /= 10u; }
        dst[hdr - 1] = '\n';
    }
    const char *src = tb + tbOff[p] + (cap - len);
#pragma unroll
    for (int line = 0; line < 3; line++) {
        const char *s = src + (size_t)line * cap;
        char *d = dst + hdr + (size_t)line * (len + 1);
        for (int x = lane; x < len; x += 64) d[x] = s[x];
        if (lane == 0) d[len] = '\n';
    }
}

__global__ void __launch_bounds__(256) k_out_compact(const dpx_pair_dev *pairs, const int32_t *score, const int32_t *tbLen, const uint64_t *tbOff,
                                                      const char *tb, int numPairs, unsigned long long firstNumber,
                                                      const unsigned long long *outOff, char *out) {
    const int lane = threadIdx.x & 63;
    const int p = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (p >= numPairs) return;
    out_write_block(pairs, score, tbLen, tbOff, tb, p, lane, firstNumber, outOff[p], out);
}

/* Small batches (up to kOutSmallPairs pairs: the class-per-pair drivers send 20 per device round trip): lengths, scan and copy in ONE
 * workgroup -- one launch instead of four in a chain of dependent kernels whose launches are most of the round trip. */
constexpr int kOutSmallPairs = 256;
static_assert(kOutSmallPairs <= kScanThreads, "one pair per thread");
__global__ void __launch_bounds__(kScanThreads) k_out_small(const dpx_pair_dev *pairs, const int32_t *score, const int32_t *tbLen, const uint64_t *tbOff,
                                                            const char *tb, int numPairs, unsigned long long firstNumber, unsigned long long *outOff,
                                                            char *out) {
    __shared__ unsigned long long lds[kScanThreads / 64];
    __shared__ unsigned long long offs[kOutSmallPairs];
    const int p = (int)threadIdx.x; /* one pair per thread (kScanThreads >= kOutSmallPairs) */
    const unsigned long long mine = p < numPairs ? block_len(firstNumber + (unsigned long long)p, score[p], tbLen[p]) : 0ull;
    unsigned long long total;
    const unsigned long long ex = group_exclusive(mine, lds, &total);
    if (p < numPairs) { outOff[p] = ex; offs[p] = ex; }
    if (p == 0) outOff[numPairs] = total;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int q = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); q < numPairs; q += kScanThreads / 64)
        out_write_block(pairs, score, tbLen, tbOff, tb, q, lane, firstNumber, offs[q], out);
}

/* =====================================================================================================
 * 2-bit packed input (dpx_batch_create_packed2; the input side of c++/parseInput.cpp:78-112): the host sends four bases
 * per byte (base k in bits 2*(k%4) of byte k/4) and a 4-entry alphabet; one thread expands one dword = 16 bases into the 16 bytes
 * of the byte buffer that every fill, traceback and output kernel reads (one aligned 16-byte store).  The fills keep matching
 * plain bytes (the reference's contract: any alphabet), so a packed batch and a byte batch are the same batch after this kernel.
 * ===================================================================================================== */
__global__ void __launch_bounds__(256) k_unpack2(const uint32_t *packed, const uint32_t alphabet, uint4 *out, const size_t numDwords) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= numDwords) return;
    const uint32_t w = packed[i];
    uint32_t o[4];
#pragma unroll
    for (int k = 0; k < 4; k++) { /* eight bits of w = four bases = one output dword: v_perm_b32 picks alphabet bytes by selector */
        const uint32_t c = (w >> (8 * k)) & 0xFFu;
        const uint32_t sel = (c & 3u) | (((c >> 2) & 3u) << 8) | (((c >> 4) & 3u) << 16) | ((c >> 6) << 24);
        o[k] = __builtin_amdgcn_perm(0u, alphabet, sel);
    }
    out[i] = make_uint4(o[0], o[1], o[2], o[3]);
}

/* =====================================================================================================
 * DPX primitive probe (dpx_prim_eval): runs the CDNA4 mappings of dpx_prims.hpp on the device.
 * ===================================================================================================== */
__global__ void k_prim_eval(const int32_t *op, const uint32_t *a, const uint32_t *b, const uint32_t *c, size_t count,
                            uint32_t *res, uint32_t *pred) {
    const size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= count) return;
    const uint32_t A = a[x], B = b[x], C = c[x];
    const int sa = (int)A, sb = (int)B, sc = (int)C;
    bool p = false, ph = false, pl = false;
    uint32_t r = 0;
    switch (op[x]) {
    case 0: r = (uint32_t)dpx::vimax3_s32(sa, sb, sc); break;
    case 1: r = dpx::vimax3_s16x2(A, B, C); break;
    case 2: r = dpx::vimax3_u32(A, B, C); break;
    case 3: r = dpx::vimax3_u16x2(A, B, C); break;
    case 4: r = (uint32_t)dpx::vimin3_s32(sa, sb, sc); break;
    case 5: r = dpx::vimin3_s16x2(A, B, C); break;
    case 6: r = dpx::vimin3_u32(A, B, C); break;
    case 7: r = dpx::vimin3_u16x2(A, B, C); break;
    case 8: r = (uint32_t)dpx::vimax_s32_relu(sa, sb); break;
    case 9: r = dpx::vimax_s16x2_relu(A, B); break;
    case 10: r = (uint32_t)dpx::vimin_s32_relu(sa, sb); break;
    case 11: r = dpx::vimin_s16x2_relu(A, B); break;
    case 12: r = (uint32_t)dpx::vimax3_s32_relu(sa, sb, sc); break;
    case 13: r = dpx::vimax3_s16x2_relu(A, B, C); break;
    case 14: r = (uint32_t)dpx::vimin3_s32_relu(sa, sb, sc); break;
    case 15: r = dpx::vimin3_s16x2_relu(A, B, C); break;
    case 16: r = (uint32_t)dpx::vibmax_s32(sa, sb, &p); break;
    case 17: r = dpx::vibmax_u32(A, B, &p); break;
    case 18: r = (uint32_t)dpx::vibmin_s32(sa, sb, &p); break;
    case 19: r = dpx::vibmin_u32(A, B, &p); break;
    case 20: r = dpx::vibmax_s16x2(A, B, &ph, &pl); break;
    case 21: r = dpx::vibmax_u16x2(A, B, &ph, &pl); break;
    case 22: r = dpx::vibmin_s16x2(A, B, &ph, &pl); break;
    case 23: r = dpx::vibmin_u16x2(A, B, &ph, &pl); break;
    case 24: r = (uint32_t)dpx::viaddmax_s32(sa, sb, sc); break;
    case 25: r = dpx::viaddmax_u32(A, B, C); break;
    case 26: r = dpx::viaddmax_s16x2(A, B, C); break;
    case 27: r = dpx::viaddmax_u16x2(A, B, C); break;
    case 28: r = (uint32_t)dpx::viaddmin_s32(sa, sb, sc); break;
    case 29: r = dpx::viaddmin_u32(A, B, C); break;
    case 30: r = dpx::viaddmin_s16x2(A, B, C); break;
    case 31: r = dpx::viaddmin_u16x2(A, B, C); break;
    case 32: r = (uint32_t)dpx::viaddmax_s32_relu(sa, sb, sc); break;
    case 33: r = dpx::viaddmax_s16x2_relu(A, B, C); break;
    case 34: r = (uint32_t)dpx::viaddmin_s32_relu(sa, sb, sc); break;
    case 35: r = dpx::viaddmin_s16x2_relu(A, B, C); break;
    default: break;
    }
    res[x] = r;
    const int o = op[x];
    pred[x] = (o >= 20 && o <= 23) ? (uint32_t)((ph ? 2 : 0) | (pl ? 1 : 0)) : (uint32_t)(p ? 1 : 0);
}

} // namespace

/* result text of a batch: lengths -> exclusive scan (tileSums: ceil(numPairs / 2048) + 1 entries of scratch) -> packed copy.
 * outOff[numPairs] receives the total number of bytes. */
size_t dpx_out_scan_tiles(size_t numPairs) { return (numPairs + kScanTile - 1) / kScanTile; }
hipError_t dpx_launch_output(const dpx_pair_dev *pairs, const int32_t *score, const int32_t *tbLen, const uint64_t *tbOff, const char *tb,
                             int numPairs, unsigned long long firstNumber, unsigned long long *tileSums, unsigned long long *outOff, char *out,
                             bool scanOnly, bool compactOnly, hipStream_t stream) {
    if (numPairs <= 0) return hipSuccess;
    const int tiles = (int)dpx_out_scan_tiles((size_t)numPairs);
    if (!compactOnly && !scanOnly && numPairs <= kOutSmallPairs) {
        hipLaunchKernelGGL(k_out_small, dim3(1), dim3(kScanThreads), 0, stream, pairs, score, tbLen, tbOff, tb, numPairs, firstNumber, outOff, out);
        return hipGetLastError();
    }
    if (!compactOnly) {
        hipLaunchKernelGGL(k_out_scan<false>, dim3(tiles), dim3(kScanThreads), 0, stream, score, tbLen, numPairs, firstNumber, tileSums, outOff);
        hipLaunchKernelGGL(k_out_scan_tiles, dim3(1), dim3(kScanThreads), 0, stream, tileSums, tiles);
        hipLaunchKernelGGL(k_out_scan<true>, dim3(tiles), dim3(kScanThreads), 0, stream, score, tbLen, numPairs, firstNumber, tileSums, outOff);
    }
    if (!scanOnly)
        hipLaunchKernelGGL(k_out_compact, dim3((unsigned)((numPairs + 3) / 4)), dim3(256), 0, stream, pairs, score, tbLen, tbOff, tb, numPairs, firstNumber,
                           outOff, out);
    return hipGetLastError();
}

/* expand numDwords x 16 bases (2 bits each) into bytes: out must be 16-byte aligned and hold 16 * numDwords bytes */
hipError_t dpx_launch_unpack2(const uint32_t *packed, uint32_t alphabet, char *out, size_t numDwords, hipStream_t stream) {
    if (numDwords == 0) return hipSuccess;
    hipLaunchKernelGGL(k_unpack2, dim3((unsigned)((numDwords + 255) / 256)), dim3(256), 0, stream, packed, alphabet, reinterpret_cast<uint4 *>(out), numDwords);
    return hipGetLastError();
}

hipError_t dpx_launch_prim_eval(const int32_t *op, const uint32_t *a, const uint32_t *b, const uint32_t *c, size_t count,
                                uint32_t *res, uint32_t *pred, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(k_prim_eval, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, op, a, b, c, count, res,
                       pred);
    return hipGetLastError();
}
