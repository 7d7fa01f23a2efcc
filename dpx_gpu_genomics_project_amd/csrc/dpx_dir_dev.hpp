/* dpx_dir_dev.hpp -- device helpers of the direction fills' code stores (layout in dpx_dir.h), shared by dpx_dir_kernels.hip and
 * dpx_dirtab_kernels.hip. */
#ifndef DPX_DIR_DEV_HPP
#define DPX_DIR_DEV_HPP

#include <stdint.h>

#include "dpx_device.hpp"
#include "dpx_table_dev.hpp"

namespace dpx_dir_dev {

using dpx_dev::u32x4;

/* the R codes of one lane and step (4 bits each, row r in bits 4r) into the lane's 32-nibble store word: step q of the group */
template <int R>
__device__ __forceinline__ void dir_put(uint32_t (&acc)[4], const int q, const uint32_t w0, const uint32_t w1) {
    if constexpr (R == 16) {
        acc[2 * q] = w0;
        acc[2 * q + 1] = w1;
    } else if constexpr (R == 8) {
        acc[q] = w0;
    } else if constexpr (R == 4) {
        acc[q >> 1] = (q & 1) ? (acc[q >> 1] | (w0 << 16)) : w0;
    } else {
        acc[q >> 2] = (q & 3) ? (acc[q >> 2] | (w0 << (8 * (q & 3)))) : w0;
    }
}

__device__ __forceinline__ void dir_store(unsigned char *dst, const uint32_t (&acc)[4]) {
    const u32x4 v = {acc[0], acc[1], acc[2], acc[3]};
    *reinterpret_cast<u32x4 *>(dst) = v; /* global_store_dwordx4: the wave writes one whole KiB */
}

} // namespace dpx_dir_dev

#endif
