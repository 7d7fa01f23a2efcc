/*
 * dpx_table_dev.hpp -- the substitution table in LDS, for every kernel that scores through one.
 * The image of dpx_kernels.h (dpx_table_ref: 1 KiB of int8 at row stride 32, row = reference code, then the 256-byte map; both 16-byte
 * aligned in one device allocation) goes into `img`, DPX_SUBST_IMAGE_BYTES of the calling wave's LDS, by all 64 lanes.  The waves of a
 * workgroup share nothing and return at different points, so every wave keeps its own copy and there is no barrier to meet at: the
 * helpers end in a wavefront-scope release / wave_barrier / acquire (table_copy_rows excepted), after which a lane may read what other
 * lanes of its wave stored.
 */
#ifndef DPX_TABLE_DEV_HPP
#define DPX_TABLE_DEV_HPP

#include "dpx_device.hpp"
#include "dpx_kernels.h"

namespace dpx_table {

/* a lane's LDS stores become readable by the other lanes of its wave */
__device__ __forceinline__ void wave_publish_lds() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
}

/* The image as it is: the table is `img` itself, a cell's byte at (reference code << 5) + query code, the map behind it.
 * DPX_TABLE_COPY_ROWS is the copy alone, as text: k_subst_fill and k_zsub_fill expand it in their own bodies, because their code moves
 * with any grouping of these stores into a function (dpx_band_affine.hpp, profiles/table_path_ab.md).  Those two read the image and
 * their staged strings with no fence, which holds on this hardware because one wave's LDS operations stay in order, and by the memory
 * model is a data race.  Every other kernel calls table_stage_rows, which returns the map. */
#define DPX_TABLE_COPY_ROWS(img_, ref_, lane_)                                                                                                 \
    {                                                                                                                                          \
        reinterpret_cast<dpx_dev::u32x4 *>(img_)[lane_] = reinterpret_cast<const dpx_dev::u32x4 *>((ref_).table)[lane_];                       \
        if ((lane_) < 16)                                                                                                                      \
            reinterpret_cast<dpx_dev::u32x4 *>((img_) + DPX_SUBST_TABLE_BYTES)[lane_] = reinterpret_cast<const dpx_dev::u32x4 *>((ref_).codeOf)[lane_]; \
    }
__device__ __forceinline__ const unsigned char *table_stage_rows(unsigned char *img, const dpx_table_ref &ref, const int lane) {
    DPX_TABLE_COPY_ROWS(img, ref, lane)
    wave_publish_lds();
    return img + DPX_SUBST_TABLE_BYTES;
}

/* The table TRANSPOSED (the entry of reference code c and query code q at (q << 5) + c), the map behind it as it is: a lane's row bases
 * are then formed once per stripe and a cell's address is one add of the staged reference code, no shift per step (dpx_affine_dev.hpp).
 * Returns the map. */
__device__ __forceinline__ const unsigned char *table_stage(unsigned char *img, const int8_t *tableG, const unsigned char *codeOfG, const int lane) {
    const dpx_dev::u32x4 v = reinterpret_cast<const dpx_dev::u32x4 *>(tableG)[lane]; /* row lane / 2, columns 16 * (lane & 1) ... */
    unsigned char *col = img + (lane >> 1) + ((lane & 1) << 9);
#pragma unroll
    for (int k = 0; k < 16; k++) col[k << 5] = (unsigned char)(v[k >> 2] >> (8 * (k & 3)));
    if (lane < 16) reinterpret_cast<dpx_dev::u32x4 *>(img + DPX_SUBST_TABLE_BYTES)[lane] = reinterpret_cast<const dpx_dev::u32x4 *>(codeOfG)[lane];
    wave_publish_lds();
    return img + DPX_SUBST_TABLE_BYTES;
}
/* a staged string of n bytes becomes codes in place, by the G lanes that share it (l = the calling lane's index among them): a lane
 * translates bytes that other lanes staged */
__device__ __forceinline__ void table_translate(unsigned char *s, const int n, const int l, const int G, const unsigned char *codeL) {
    for (int x = l; x < n; x += G) s[x] = codeL[s[x]];
    wave_publish_lds();
}

} // namespace dpx_table

#endif
