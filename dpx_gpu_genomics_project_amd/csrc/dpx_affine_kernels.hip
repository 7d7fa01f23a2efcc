/*
 * dpx_affine_kernels.hip -- the Gotoh fills on the stripe schedule of dpx_kernels.hip: ANW, ASW and ASG, one wave per pair
 * (k_affine_fill / k_asw_fill / k_asg_fill, body dpx_affine_fill.inc) and lane-packed (k_affine_lanes / k_asw_lanes / k_asg_lanes,
 * body dpx_affine_lanes.inc).  The cell updates and publishers (shared with dpx_scoretab_kernels.hip, the score-only kernels under a
 * substitution table, which include the same two bodies with TABLE on) are in dpx_affine_dev.hpp; the helpers shared with the linear
 * fills are in dpx_fill_common.hpp and dpx_device.hpp.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpx_affine_dev.hpp"
#include "dpx_fill_common.hpp"
#include "dpx_kernels.h"
#include "dpx_layout.h"
#include "dpx_prims.hpp"

namespace {

using dpx::pack_lo16;
using dpx::wave_shr1;
using namespace dpx_dev;
using namespace dpx_fill;
using namespace dpx_affine;

/* one wave per pair: k_affine_fill (ANW), k_asw_fill (ASW) and k_asg_fill (ASG) share their body, dpx_affine_fill.inc */
template <int R, bool STORE>
__global__ void __launch_bounds__(DPX_FILL_THREADS) k_affine_fill(const dpx_fill_args a) {
    constexpr bool LOCAL = false, SEMI = false, TABLE = false;
    constexpr const int8_t *tableG = nullptr; constexpr const unsigned char *codeOfG = nullptr;
#include "dpx_affine_fill.inc"
}

template <int R, bool STORE>
__global__ void __launch_bounds__(DPX_FILL_THREADS) k_asw_fill(const dpx_fill_args a) {
    constexpr bool LOCAL = true, SEMI = false, TABLE = false;
    constexpr const int8_t *tableG = nullptr; constexpr const unsigned char *codeOfG = nullptr;
#include "dpx_affine_fill.inc"
}

template <int R, bool STORE>
__global__ void __launch_bounds__(DPX_FILL_THREADS) k_asg_fill(const dpx_fill_args a) {
    constexpr bool LOCAL = false, SEMI = true, TABLE = false;
    constexpr const int8_t *tableG = nullptr; constexpr const unsigned char *codeOfG = nullptr;
#include "dpx_affine_fill.inc"
}

template <int R, bool STORE>
__global__ void __launch_bounds__(DPX_ALANES_THREADS) k_affine_lanes(const dpx_fill_args a) {
    constexpr bool LOCAL = false, SEMI = false, TABLE = false;
    constexpr const int8_t *tableG = nullptr; constexpr const unsigned char *codeOfG = nullptr;
#include "dpx_affine_lanes.inc"
}

template <int R, bool STORE>
__global__ void __launch_bounds__(DPX_ALANES_THREADS) k_asw_lanes(const dpx_fill_args a) {
    constexpr bool LOCAL = true, SEMI = false, TABLE = false;
    constexpr const int8_t *tableG = nullptr; constexpr const unsigned char *codeOfG = nullptr;
#include "dpx_affine_lanes.inc"
}

template <int R, bool STORE>
__global__ void __launch_bounds__(DPX_ALANES_THREADS) k_asg_lanes(const dpx_fill_args a) {
    constexpr bool LOCAL = false, SEMI = true, TABLE = false;
    constexpr const int8_t *tableG = nullptr; constexpr const unsigned char *codeOfG = nullptr;
#include "dpx_affine_lanes.inc"
}

} // namespace

/* ---- this unit's side of dpx_launch_fill and dpx_launch_fill_lanes (dpx_kernels.hip); algo is ANW, ASW or ASG ---- */

hipError_t dpx_launch_affine_fill(const dpx_fill_args &a, int algo, int R, bool store, size_t ldsBytes, hipStream_t stream) {
    return dispatch_int<2, 4, 8>(R, [&](auto r) {
        return dispatch_bool(store, [&](auto st) {
            constexpr int kR = decltype(r)::value;
            constexpr bool kStore = decltype(st)::value;
            if (algo == DPX_K_ANW) return launch_fill(k_affine_fill<kR, kStore>, a, a, ldsBytes, stream);
            if (algo == DPX_K_ASW) return launch_fill(k_asw_fill<kR, kStore>, a, a, ldsBytes, stream);
            return launch_fill(k_asg_fill<kR, kStore>, a, a, ldsBytes, stream);
        });
    });
}

hipError_t dpx_launch_affine_lanes(const dpx_fill_args &a, int algo, int R, bool store, size_t ldsBytes, hipStream_t stream) {
    const int wpb = DPX_ALANES_THREADS / 64; /* (ldsBytes = per wave x this) */
    const dim3 grid((unsigned)((a.numPairs + wpb - 1) / wpb)), block(DPX_ALANES_THREADS);
    return dispatch_int<8>(R, [&](auto r) {
        return dispatch_bool(store, [&](auto st) {
            constexpr int kR = decltype(r)::value;
            constexpr bool kStore = decltype(st)::value;
            if (algo == DPX_K_ANW) return launch_lds(k_affine_lanes<kR, kStore>, grid, block, ldsBytes, stream, a);
            if (algo == DPX_K_ASW) return launch_lds(k_asw_lanes<kR, kStore>, grid, block, ldsBytes, stream, a);
            return launch_lds(k_asg_lanes<kR, kStore>, grid, block, ldsBytes, stream, a);
        });
    });
}
