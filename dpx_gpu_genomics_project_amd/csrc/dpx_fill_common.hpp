/*
 * dpx_fill_common.hpp -- what the stripe-schedule fills share: the linear-gap fills (dpx_kernels.hip), the Gotoh fills
 * (dpx_affine_kernels.hip with dpx_affine_fill.inc / dpx_affine_lanes.inc) and, for the packed-int16 pieces, the banded fills
 * (dpx_bsw_kernels.hip).  The ablation switches, the query-row load, the tile stores and their ramp rules, the wave descriptor of the
 * lane-packed kernels, the fold of per-row start-cell keys.  __forceinline__ functions and templates in namespace dpx_fill; the cross-
 * family helpers are in dpx_device.hpp.
 */
#ifndef DPX_FILL_COMMON_HPP
#define DPX_FILL_COMMON_HPP

#include "dpx_device.hpp"
#include "dpx_layout.h"

/* matrices are written once and never re-read by the fill: DPX_NT_STORES selects `global_store ... nt` */
#ifndef DPX_NT_STORES
#define DPX_NT_STORES 0
#endif
#ifndef DPX_EXP_NOCOMPUTE
#define DPX_EXP_NOCOMPUTE 0
#endif
#ifndef DPX_EXP_NORAMPSTORE
#define DPX_EXP_NORAMPSTORE 0
#endif
/* ablation builds of the lane-packed kernels (tools/ab_quad.sh): 1 = no global stores, 2 = stores without the LDS round trip */
#ifndef DPX_EXP_QUAD
#define DPX_EXP_QUAD 0
#endif

namespace dpx_fill {

using dpx::as_s16x2;
using dpx::as_u16x2;
using dpx::as_u32;
using dpx::pack_lo16;
using dpx::s16x2;
using dpx_dev::u32x2;
using dpx_dev::u32x4;

/* the R query characters of a lane's rows (row0 .. row0+R-1 of `qry`) from R/4 + 1 aligned dword loads and
 * v_alignbyte_b32 instead of R byte loads; rows past the query's end get 0x100 (matches no byte) */
template <int R>
__device__ __forceinline__ void load_query_rows(int (&qc)[R], const unsigned char *qry, const int row0, const int nrows) {
    if (nrows <= 0) {
#pragma unroll
        for (int r = 0; r < R; r++) qc[r] = 0x100;
        return;
    }
    constexpr int W = (R + 3) / 4;
    const unsigned char *at = qry + row0;
    const unsigned sh = (unsigned)(reinterpret_cast<uintptr_t>(at) & 3u);
    const uint32_t *al = reinterpret_cast<const uint32_t *>(at - sh);
    uint32_t d[W + 1];
#pragma unroll
    for (int k = 0; k <= W; k++) d[k] = al[k];
#pragma unroll
    for (int k = 0; k < W; k++) {
        const uint32_t v = __builtin_amdgcn_alignbyte(d[k + 1], d[k], sh); /* bytes 4k .. 4k+3 of the lane's rows */
#pragma unroll
        for (int bq = 0; bq < 4 && 4 * k + bq < R; bq++) {
            const int r = 4 * k + bq;
            qc[r] = (r < nrows) ? (int)((v >> (8 * bq)) & 0xFFu) : 0x100;
        }
    }
}

template <class V>
__device__ __forceinline__ void stream_store(V *dst, V v) {
#if DPX_NT_STORES
    __builtin_nontemporal_store(v, dst);
#else
    *dst = v;
#endif
}

template <int R>
__device__ __forceinline__ void store_tile(int16_t *dst, const int (&v)[R]) {
    if constexpr (R == 1) {
        *dst = (int16_t)v[0];
    } else if constexpr (R == 2) {
        stream_store(reinterpret_cast<uint32_t *>(dst), pack_lo16(v[0], v[1]));
    } else if constexpr (R == 4) {
        u32x2 w = {pack_lo16(v[0], v[1]), pack_lo16(v[2], v[3])};
        stream_store(reinterpret_cast<u32x2 *>(dst), w);
    } else {
#pragma unroll
        for (int q = 0; q < R / 8; q++) {
            u32x4 w = {pack_lo16(v[8 * q + 0], v[8 * q + 1]), pack_lo16(v[8 * q + 2], v[8 * q + 3]),
                       pack_lo16(v[8 * q + 4], v[8 * q + 5]), pack_lo16(v[8 * q + 6], v[8 * q + 7])};
            stream_store(reinterpret_cast<u32x4 *>(dst + q * 512), w); /* sub-tile q: its own 1 KiB [lane][8] block */
        }
    }
}

/* Single-stripe pairs shorter than 64*R rows leave the upper lanes without rows; those lanes need not store.  Returns
 * the number of lanes that do: the row-owning lanes rounded up to whole 128-byte lines of the store (a line written
 * in part costs a read-modify-write at the memory side: rounding to 64-byte sectors measured 25 % slower on the
 * short-read batch, profiles/README.md). */
template <int R>
__device__ __forceinline__ int store_lanes(const int m) {
    constexpr int perLine = 128 / (2 * (R < 8 ? R : 8)); /* lanes per 128-byte line: 32 / 16 / 8 for R = 2 / 4 / >= 8 */
    const int owning = (m + R - 1) / R;
    return min(64, (owning + perLine - 1) / perLine * perLine);
}

/* Skew ramps: in step t of a stripe of n columns only the lanes t-n+1 .. t are on a real cell.  Storing the whole chunk writes
 * 6 % of padding at 1024 x 1024 (12 % at 512 x 512); storing exactly the lanes on a cell leaves partly written 128-byte lines,
 * which cost more than they save (profiles/README.md).  So the ramp steps store the lanes on a cell ROUNDED OUT TO WHOLE LINES
 * (8 lanes x 16 B; 16 / 32 lanes for 4 / 2 rows per lane): nearly all of the padding stays unwritten, every written line is
 * whole.  DPX_EXP_FULLRAMP=1 builds the round-1 behaviour (whole chunks) for A/B runs. */
#ifndef DPX_EXP_FULLRAMP
#define DPX_EXP_FULLRAMP 0
#endif
template <int R>
__device__ __forceinline__ bool ramp_stores(const int lane, const int t, const int n, const int rampLines) {
#if DPX_EXP_FULLRAMP
    return true;
#else
    if (!rampLines) return true; /* small batches are bound by the latency of a step, not by bytes: whole chunks are cheaper there */
    constexpr int perLine = 128 / (2 * (R < 8 ? R : 8));
    const int lo = max(t - n + 1, 0) & ~(perLine - 1), hi = (min(t, 63) + perLine) & ~(perLine - 1);
    return lane >= lo && lane < hi;
#endif
}

/* what a lane learns from the wave's descriptor */
struct LaneSlot {
    bool has;
    int p, l, num, d; /* pair, lane inside the slot, lanes of the slot, start delay (first lane mod 8) */
    uint32_t refOff;  /* LDS byte offset of the slot's staged reference inside the wave's reference area */
};
__device__ __forceinline__ LaneSlot find_slot(const dpx_wave_desc *wd, const int lane) {
    LaneSlot s{false, 0, 0, 0, 0, 0u};
    const uint32_t *w = reinterpret_cast<const uint32_t *>(wd); /* wave-uniform address: 2 dwords per slot through scalar loads */
    static_assert(DPX_WAVE_SLOTS % 4 == 0 && sizeof(dpx_wave_desc) == 8 * DPX_WAVE_SLOTS, "descriptor is read as dwords");
    constexpr int kFirst = DPX_WAVE_SLOTS, kNum = DPX_WAVE_SLOTS + DPX_WAVE_SLOTS / 4, kRef = DPX_WAVE_SLOTS + DPX_WAVE_SLOTS / 2; /* dword offsets */
#pragma unroll
    for (int k = 0; k < DPX_WAVE_SLOTS; k++) {
        const int f = (int)((w[kFirst + (k >> 2)] >> (8 * (k & 3))) & 0xFFu), c = (int)((w[kNum + (k >> 2)] >> (8 * (k & 3))) & 0xFFu);
        const uint32_t ro = (w[kRef + (k >> 1)] >> (16 * (k & 1))) & 0xFFFFu;
        if (lane >= f && lane < f + c) { s.has = true; s.p = (int)w[k]; s.l = lane - f; s.num = c; s.d = f & 7; s.refOff = ro << 4; }
    }
    return s;
}

/* SW / ASW: fold the finished stripe's per-row (H << 16 | 0xFFFF - j) keys into the lane's best (rows ascend with r and with the
 * stripe index, so a strict '>' keeps the first row holding the lane's maximum) */
template <int R>
__device__ __forceinline__ void fold_row_keys(const unsigned (&key)[R], const int row0, const int nrows, int &bestv, int &bestrow, int &bestcol) {
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int hv = (int)(key[r] >> 16), col = 0xFFFF - (int)(key[r] & 0xFFFFu);
        if (r < nrows && hv > bestv) {
            bestv = hv;
            bestrow = row0 + 1 + r;
            bestcol = col;
        }
    }
}

__device__ __forceinline__ uint32_t pk_hi16(uint32_t lo, uint32_t hi) { return __builtin_amdgcn_perm(hi, lo, 0x07060302u); } /* {lo.hi16, hi.hi16} */

/* SW with gap <= 0 (round 3): max(up, left) - |gap| SATURATING at 0 (v_pk_sub_u16 ... clamp; SW cells are never negative, so the signed
 * maximum of two of them is their unsigned one).  The gap term is then >= 0, so H = max(gap term, diag + s) >= 0 without the extra
 * v_pk_max_i16(H, 0) of c++/LinearSmithWaterman.cpp:103 -- the SW cell costs what the NW cell costs.  The host sends a batch to the
 * kernels that use this only if gap <= 0. */
__device__ __forceinline__ s16x2 pk_gap_sat(const uint32_t up, const uint32_t left, const uint32_t gabsP) {
    return as_s16x2(as_u32(__builtin_elementwise_sub_sat(as_u16x2(as_u32(dpx::pk_max(as_s16x2(up), as_s16x2(left)))), as_u16x2(gabsP))));
}

} // namespace dpx_fill
#endif
