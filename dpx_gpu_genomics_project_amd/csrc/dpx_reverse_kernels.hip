/* dpx_reverse_kernels.hip -- per-pair orientation of BANW / BAXT batches (dpx_batch_set_reversed, include/dpx_align.h).
 *
 * No fill, walk or export kernel knows about orientation: each finds its strings through dpx_pair_dev.refIdx / qryIdx, so a reversed
 * pair is a pair whose indices point at reversed COPIES of its strings, and its results come out in the reversed frame.  Three small
 * kernels around the existing ones put the rest in place:
 *
 *   k_reverse_strings  once per dpx_batch_set_reversed: one wave per string.  Output block k (16 bytes at the 16-byte aligned
 *                      destination) is the source's bytes [n - 16 - 16k, n - 16k) back to front.  They sit at an arbitrary address, so a
 *                      lane loads the one or two aligned 16-byte blocks that hold them, shifts by whole dwords with selects (no register
 *                      array is indexed by a variable: no scratch) and lets v_perm_b32 do the byte shift and the byte reverse in one
 *                      instruction per dword.  A block that holds no byte of the string is never loaded (the first string of the buffer
 *                      has nothing in front of it); the bytes it would have supplied land behind the copy's last character, inside
 *                      its own slot, and are never read as characters.
 *   k_flip_lines       once per fill, behind the walk: one wave per flagged pair reverses its three traceback lines in place.  A line's
 *                      tbLen characters are right-aligned in a capacity that is a multiple of 4 at an offset that is a multiple of 4
 *                      (dpx_cigar.h), so the range ends on a dword boundary and starts `skew` bytes into one, and an aligned dword is
 *                      the widest access every line admits.  With A / B the first / one-past-last dword, output dword d is the byte
 *                      reverse of the 4 bytes that end `skew` bytes into dword E = A + B - d: v_perm_b32 over dwords E - 1 and E.  A
 *                      trip takes 64 dwords from either end, loads all it needs, then stores; the one dword a trip needs that the trip
 *                      before has overwritten (dword `hi`) travels in a wave-uniform register.  The last <= 128 dwords are one trip.
 *                      The `skew` bytes in front of the line keep their values.
 *   k_map_records      behind k_cigar_write: the coordinates of the flagged pairs' dpx_alignment records, reversed frame -> original.
 *
 * Every access is an aligned dword or wider, one per lane; no LDS, no atomics, no scratch. */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpx_device.hpp"
#include "dpx_reverse.h"

namespace {

using namespace dpx_dev;

constexpr int kRevThreads = 256; /* four independent waves per workgroup, one string / pair each (as the CIGAR kernels) */

/* v_perm_b32 selector: byte j of the result is byte 3 + r - j of {hi, lo} -- the dword that starts r bytes into lo, back to front */
__device__ __forceinline__ uint32_t rev_selector(int r) { return 0x00010203u + 0x01010101u * (uint32_t)r; }

__global__ void __launch_bounds__(kRevThreads) k_reverse_strings(char *seq, const dpx_rev_job *jobs, int numJobs) {
    const int lane = threadIdx.x & 63;
    const int j = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kRevThreads / DPX_WAVE) + (threadIdx.x >> 6)));
    if (j >= numJobs) return;
    const int src = jobs[j].src, n = jobs[j].len;
    u32x4 *dst = reinterpret_cast<u32x4 *>(seq + jobs[j].dst);
    const int blocks = (n + 15) >> 4; /* (n <= 0: none) */
    for (int k = lane; k < blocks; k += DPX_WAVE) {
        const int s0 = src + n - 16 - 16 * k; /* first of the 16 source bytes; >= src - 15, so it may lie in front of the string (and of the buffer) */
        const int sh = s0 & 15, base = s0 - sh;
        u32x4 lo = {0u, 0u, 0u, 0u}, hi = {0u, 0u, 0u, 0u};
        if (base + 16 > src) lo = *reinterpret_cast<const u32x4 *>(seq + base);                  /* (base < src + n always) */
        if (sh != 0 && base + 16 < src + n) hi = *reinterpret_cast<const u32x4 *>(seq + base + 16); /* (base + 32 > src always) */
        /* the five dwords from dword sh / 4 of {lo, hi} on: two select stages, every index a constant */
        const bool by1 = (sh & 4) != 0, by2 = (sh & 8) != 0;
        const uint32_t w0 = lo.x, w1 = lo.y, w2 = lo.z, w3 = lo.w, w4 = hi.x, w5 = hi.y, w6 = hi.z, w7 = hi.w;
        const uint32_t y0 = by1 ? w1 : w0, y1 = by1 ? w2 : w1, y2 = by1 ? w3 : w2, y3 = by1 ? w4 : w3, y4 = by1 ? w5 : w4, y5 = by1 ? w6 : w5,
                       y6 = by1 ? w7 : w6;
        const uint32_t x0 = by2 ? y2 : y0, x1 = by2 ? y3 : y1, x2 = by2 ? y4 : y2, x3 = by2 ? y5 : y3, x4 = by2 ? y6 : y4;
        const uint32_t sel = rev_selector(sh & 3);
        u32x4 out;
        out.x = __builtin_amdgcn_perm(x4, x3, sel);
        out.y = __builtin_amdgcn_perm(x3, x2, sel);
        out.z = __builtin_amdgcn_perm(x2, x1, sel);
        out.w = __builtin_amdgcn_perm(x1, x0, sel);
        dst[k] = out;
    }
}

/* Between the loads and the stores of a trip, and between two trips: the wave reads dwords that another of its lanes overwrites.  The
 * fence keeps the compiler from moving a memory operation across; the wait (gfx9 encoding of vmcnt(0) alone) lets every load of the
 * wave return before the first store is issued, although one wave's vector memory operations reach the cache in order anyway. */
__device__ __forceinline__ void flip_fence() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_s_waitcnt(0x0F70);
}

/* dwords [A, B) of `L`, the first `skew` bytes of dword A excepted, back to front in place (one wave) */
__device__ __forceinline__ void flip_range(uint32_t *L, const int A, const int B, const int skew, const int lane) {
    if (B - A <= 0) return;
    const uint32_t sel = rev_selector(skew);
    const uint32_t keep = skew ? (1u << (8 * skew)) - 1u : 0u; /* the bytes of dword A that are not the line's */
    const uint32_t first = L[A];                               /* (wave-uniform address) */
    int lo = A, hi = B;   /* what is left to write; lo - A == B - hi */
    uint32_t carry = 0u;  /* the dword at `hi` as it was before the trip that overwrote it; dword B is not the line's and is not read */
    while (hi - lo > 2 * DPX_WAVE) {
        /* front: d = lo + lane takes dwords E - 1, E with E = A + B - d = hi - lane; back: d = hi - 64 + lane, E = lo + 64 - lane */
        const uint32_t f1 = L[hi - 1 - lane], f2 = lane == 0 ? carry : L[hi - lane];
        const uint32_t b1 = L[lo + 63 - lane], b2 = L[lo + 64 - lane];
        flip_fence();
        uint32_t f = __builtin_amdgcn_perm(f2, f1, sel);
        if (lo + lane == A) f = (f & ~keep) | (first & keep);
        L[lo + lane] = f;
        L[hi - DPX_WAVE + lane] = __builtin_amdgcn_perm(b2, b1, sel);
        carry = (uint32_t)__builtin_amdgcn_readlane((int)f1, DPX_WAVE - 1); /* dword hi - 64 */
        lo += DPX_WAVE;
        hi -= DPX_WAVE;
        flip_fence();
    }
    /* the middle, at most 128 dwords: two per lane, all loaded before the first store */
    uint32_t v[2] = {0u, 0u};
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const int d = lo + lane + u * DPX_WAVE;
        if (d < hi) {
            const int E = lo + hi - d;
            const uint32_t e1 = L[E - 1], e2 = E == hi ? carry : L[E];
            v[u] = __builtin_amdgcn_perm(e2, e1, sel);
            if (d == A) v[u] = (v[u] & ~keep) | (first & keep);
        }
    }
    flip_fence();
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const int d = lo + lane + u * DPX_WAVE;
        if (d < hi) L[d] = v[u];
    }
}

__global__ void __launch_bounds__(kRevThreads) k_flip_lines(const dpx_pair_dev *pairs, const int32_t *flagged, int numFlagged, const int32_t *tbLen,
                                                            const uint64_t *tbOff, char *tb) {
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kRevThreads / DPX_WAVE) + (threadIdx.x >> 6)));
    if (w >= numFlagged) return;
    const int p = flagged[w];
    const int len = tbLen[p];
    if (len <= 1) return; /* nothing to turn round */
    const int cap = (pairs[p].m + pairs[p].n + 1 + 3) & ~3; /* line capacity, as in k_traceback */
    const int lead = cap - len;                             /* the lines are right-aligned */
#pragma unroll 1
    for (int l = 0; l < 3; l++)
        flip_range(reinterpret_cast<uint32_t *>(tb + tbOff[p] + (size_t)l * (size_t)cap), lead >> 2, cap >> 2, lead & 3, lane);
}

__global__ void __launch_bounds__(kRevThreads) k_map_records(const dpx_pair_dev *pairs, const int32_t *flagged, int numFlagged, dpx_alignment *records) {
    const int w = (int)(blockIdx.x * kRevThreads + threadIdx.x);
    if (w >= numFlagged) return;
    const int p = flagged[w];
    dpx_alignment &r = records[p];
    const int n = pairs[p].n, m = pairs[p].m;
    const int refStart = n - r.refEnd, refEnd = n - r.refStart, qryStart = m - r.qryEnd, qryEnd = m - r.qryStart;
    r.refStart = refStart; r.refEnd = refEnd;
    r.qryStart = qryStart; r.qryEnd = qryEnd;
}

} // namespace

hipError_t dpx_launch_reverse_strings(char *seq, const dpx_rev_job *jobs, int numJobs, hipStream_t stream) {
    if (numJobs <= 0) return hipSuccess;
    const int perBlock = kRevThreads / DPX_WAVE;
    hipLaunchKernelGGL(k_reverse_strings, dim3((unsigned)((numJobs + perBlock - 1) / perBlock)), dim3(kRevThreads), 0, stream, seq, jobs, numJobs);
    return hipGetLastError();
}

hipError_t dpx_launch_flip_lines(const dpx_pair_dev *pairs, const int32_t *flagged, int numFlagged, const int32_t *tbLen, const uint64_t *tbOff,
                                 char *tb, hipStream_t stream) {
    if (numFlagged <= 0) return hipSuccess;
    const int perBlock = kRevThreads / DPX_WAVE;
    hipLaunchKernelGGL(k_flip_lines, dim3((unsigned)((numFlagged + perBlock - 1) / perBlock)), dim3(kRevThreads), 0, stream, pairs, flagged, numFlagged,
                       tbLen, tbOff, tb);
    return hipGetLastError();
}

hipError_t dpx_launch_map_records(const dpx_pair_dev *pairs, const int32_t *flagged, int numFlagged, dpx_alignment *records, hipStream_t stream) {
    if (numFlagged <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_map_records, dim3((unsigned)((numFlagged + kRevThreads - 1) / kRevThreads)), dim3(kRevThreads), 0, stream, pairs, flagged,
                       numFlagged, records);
    return hipGetLastError();
}
