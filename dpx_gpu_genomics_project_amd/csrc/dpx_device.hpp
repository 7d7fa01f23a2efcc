/*
 * dpx_device.hpp -- what the kernel units of every family share: vector types, sequence staging, wave reductions, the character
 * window of the walks, the band test, the workgroup scan of the two result-size passes, and the host side of a launch.
 *
 * Everything here is a __forceinline__ function, a template or a constant inside namespace dpx_dev; a unit names what it uses with
 * `using`.  Kernels stay in the anonymous namespace of their unit under their own names.
 */
#ifndef DPX_DEVICE_HPP
#define DPX_DEVICE_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "dpx_kernels.h"
#include "dpx_prims.hpp"

namespace dpx_dev {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

template <bool V>
using bool_c = std::integral_constant<bool, V>;
template <int V>
using int_c = std::integral_constant<int, V>;

/* ---- sequence staging: wide loads instead of one byte per lane and instruction ----------------------------------
 * Sequences sit at arbitrary byte offsets of the flat parseInput buffer (c++/parseInput.cpp:78-112 keeps the file's
 * bytes where they are).  stage_bytes() copies a string into LDS with aligned 16-byte loads and stores: the copy
 * starts at the 16-byte block that holds the first character, so the string lands `src & 15` bytes into the
 * (16-byte aligned) LDS buffer; the returned pointer is its first character.  The buffer needs n + 31 bytes.  The
 * device arena is 256-byte aligned and padded, so the blocks read never leave it.  `l` = the calling lane's index
 * among the G lanes that share the copy. */
__device__ __forceinline__ unsigned char *stage_bytes(unsigned char *dst16, const unsigned char *src, const int n, const int l, const int G) {
    const unsigned a = (unsigned)(reinterpret_cast<uintptr_t>(src) & 15u);
    const u32x4 *from = reinterpret_cast<const u32x4 *>(src - a);
    u32x4 *to = reinterpret_cast<u32x4 *>(dst16);
    const int blocks = n > 0 ? (int)((a + (unsigned)n + 15u) >> 4) : 0;
    for (int k = l; k < blocks; k += G) to[k] = from[k];
    return dst16 + a;
}

/* four bytes from an arbitrary address: two aligned dword loads + v_alignbyte_b32 */
__device__ __forceinline__ uint32_t load4(const unsigned char *p) {
    const unsigned sh = (unsigned)(reinterpret_cast<uintptr_t>(p) & 3u);
    const uint32_t *al = reinterpret_cast<const uint32_t *>(p - sh);
    return __builtin_amdgcn_alignbyte(al[1], al[0], sh);
}

/* eight int32 values -> eight int16, one 16-byte store */
__device__ __forceinline__ void store8(int16_t *dst, const int (&v)[8]) {
    u32x4 w = {dpx::pack_lo16(v[0], v[1]), dpx::pack_lo16(v[2], v[3]), dpx::pack_lo16(v[4], v[5]), dpx::pack_lo16(v[6], v[7])};
    *reinterpret_cast<u32x4 *>(dst) = w;
}

/* 64-lane max-reduction of a 64-bit key (once per pair; cost irrelevant) */
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        unsigned long long o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
    return v;
}

/* A byte string read back to front through one register: four characters per aligned dword load (a walk reads
 * query[i-1] and reference[j-1] on every step; with ~100k lanes in flight neither L1 nor L2 keeps a sector between two
 * steps of the same lane, so every byte load was an HBM sector fetch -- profiles/README.md). */
struct CharWin {
    const unsigned char *s;
    uintptr_t at = 1; /* address of the dword held in `w` (1 = none) */
    uint32_t w = 0;
    __device__ __forceinline__ int get(int x) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(s + x), al = a & ~(uintptr_t)3;
        if (al != at) { at = al; w = *reinterpret_cast<const uint32_t *>(al); } /* never leaves the 256-byte aligned arena */
        return (int)((w >> (8 * (int)(a & 3))) & 0xFFu);
    }
};

/* ---- exclusive scan of one 64-bit value per item over a whole launch, in three passes (result text, CIGAR operations): per-tile
 * totals, a scan over them in one workgroup, then tile base + prefix inside each tile ---- */
constexpr int kScanThreads = 256, kScanPerThread = 8, kScanTile = kScanThreads * kScanPerThread;

/* inclusive scan of one value per thread across the workgroup; returns the exclusive prefix, *total = sum over the group */
__device__ __forceinline__ unsigned long long group_exclusive(unsigned long long v, unsigned long long *lds, unsigned long long *total) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    unsigned long long x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long o = __shfl_up(x, off, 64);
        if (lane >= off) x += o;
    }
    if (lane == 63) lds[wv] = x;
    __syncthreads();
    unsigned long long base = 0, all = 0;
    for (int k = 0; k < kScanThreads / 64; k++) { const unsigned long long w = lds[k]; if (k < wv) base += w; all += w; }
    __syncthreads();
    *total = all;
    return base + x - v;
}

/* (The middle pass, ten lines, is written out in k_out_scan_tiles and in k_cigar_scan_tiles: as one inlined function, with the LDS
 * array passed in or declared inside, both kernels came out with one compare-and-branch pair inverted -- tools/isa_same.py,
 * profiles/unit_split.md -- and a split that is checked by instruction identity keeps the code each had.) */

/* ---------------------------------------------------------- launches --------------------------------------------------------- */

/* a launch with dynamic LDS: opt in to more than the default 64 KiB when `optIn` asks for it (160 KiB per CU on gfx950), launch,
 * report the launch error */
template <class K, class Args>
hipError_t launch_lds(K kernel, const dim3 grid, const dim3 block, const size_t lds, hipStream_t s, const Args &args, const size_t optIn) {
    if (optIn > 64u * 1024u) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)optIn);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, grid, block, lds, s, args);
    return hipGetLastError();
}
template <class K, class Args>
hipError_t launch_lds(K kernel, const dim3 grid, const dim3 block, const size_t lds, hipStream_t s, const Args &args) {
    return launch_lds(kernel, grid, block, lds, s, args, lds);
}

/* a fill: one wave per pair (or couple), f.wavesPerBlock independent waves per workgroup (4, or 1 for small launches: see
 * dpx_fill_waves_per_block); `lds` is the request of a four-wave workgroup */
template <class K, class Args>
hipError_t launch_fill(K kernel, const Args &args, const dpx_fill_args &f, const size_t lds, hipStream_t s) {
    const unsigned wpb = f.wavesPerBlock;
    return launch_lds(kernel, dim3(((unsigned)f.numPairs + wpb - 1) / wpb), dim3(64u * wpb), lds / 4u * wpb, s, args, lds);
}

/* f(int_c<V>) for the V among Vs that equals v; hipErrorInvalidValue when there is none */
template <int... Vs, class F>
hipError_t dispatch_int(const int v, F f) {
    hipError_t e = hipErrorInvalidValue;
    (void)((v == Vs ? ((void)(e = f(int_c<Vs>{})), true) : false) || ...);
    return e;
}
template <class F>
hipError_t dispatch_bool(const bool v, F f) {
    return v ? f(bool_c<true>{}) : f(bool_c<false>{});
}

/* launch(int_c<C>, bool_c<PB>, bool_c<FLAG>) for the cells per lane C of a banded fill, the parity PB of step 0 under `band`, and one
 * more switch */
template <class Launch>
hipError_t dispatch_fill(const int C, const int band, const bool flag, Launch launch) {
    const bool pb = ((band + 1) & 1) != 0; /* parity of step A = 0 */
    return dispatch_int<1, 2, 4, 8>(C, [&](auto c) {
        return dispatch_bool(pb, [&](auto p) { return dispatch_bool(flag, [&](auto f) { return launch(c, p, f); }); });
    });
}

} // namespace dpx_dev
#endif
