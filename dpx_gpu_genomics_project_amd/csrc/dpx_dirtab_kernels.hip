/*
 * dpx_dirtab_kernels.hip -- the fill of ANW / ASW / ASG direction batches under a substitution table (dpx_batch_set_direction_table).
 *
 * k_dirtab_fill<R, GLOBAL, KIND> is the fill of dpx_dir_kernels.hip -- dpx_affine_dir.inc, shared, with TABLE on -- so schedule, codes,
 * tie order, end-cell rules and stores are k_affine_dir's (KIND = DPX_K_ANW), k_asw_dir's (DPX_K_ASW) and k_asg_dir's (DPX_K_ASG).  One
 * term changes: the diagonal adds table[codeOf[reference byte] * 32 + codeOf[query byte]] in place of match / mismatch.  Every wave
 * keeps the 1280-byte image the band kernels use (dpx_kernels.h) in its own LDS, translates the staged reference to codes once, its R
 * query bytes once per stripe, and pays one signed-byte LDS read per cell for the compare-and-select it replaces.  The walk and the
 * export are dpx_dir_kernels.hip's, untouched: they read the 4-bit codes and the caller's bytes, never a score.
 * No MFMA, no atomics.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "dpx_device.hpp"
#include "dpx_dir.h"
#include "dpx_dir_dev.hpp"
#include "dpx_prims.hpp"

namespace {

using dpx::wave_shr1;
using dpx_dir_dev::dir_put;
using dpx_dir_dev::dir_store;
using dpx_dev::stage_bytes;
using dpx_dev::u32x4;
using dpx_dev::wave_max_u64;
using dpx_table::table_stage_rows;

template <int R, bool GLOBAL, int KIND>
__global__ void __launch_bounds__(DPX_FILL_THREADS) k_dirtab_fill(const dpx_dirtab_args t) {
    constexpr bool LOCAL = KIND == DPX_K_ASW, SEMI = KIND == DPX_K_ASG, TABLE = true;
    const dpx_dir_args &a = t.d;
    const dpx_table_ref &tref = t.tab;
#include "dpx_affine_dir.inc"
}

/* dir_launch of dpx_dir_kernels.hip with the image's LDS: behind every wave's slice, or -- edge rows in the scratch -- alone */
template <class K>
hipError_t dirtab_launch(K kernel, const dpx_dirtab_args &t, hipStream_t s) {
    const dpx_dir_args &a = t.d;
    const unsigned wpb = a.wavesPerBlock ? a.wavesPerBlock : 1u;
    if (!a.scratch) return dpx_dev::launch_lds(kernel, dim3(((unsigned)a.numPairs + wpb - 1) / wpb), dim3(64u * wpb), (size_t)a.ldsPerWave * wpb, s, t);
    dpx_dirtab_args c = t; /* DPX_DIR_SCRATCH_SLOTS waves per launch, each launch reusing the scratch */
    for (c.d.firstSlot = 0; c.d.firstSlot < a.numPairs; c.d.firstSlot += DPX_DIR_SCRATCH_SLOTS) {
        const unsigned waves = (unsigned)std::min(a.numPairs - c.d.firstSlot, DPX_DIR_SCRATCH_SLOTS);
        hipLaunchKernelGGL(kernel, dim3((waves + wpb - 1) / wpb), dim3(64u * wpb), (size_t)DPX_SUBST_IMAGE_BYTES * wpb, s, c);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <int KIND>
hipError_t launch_dirtab_kind(const dpx_dirtab_args &t, int R, hipStream_t s) {
    return dpx_dev::dispatch_int<2, 4, 8>(R, [&](auto r) {
        return t.d.scratch ? dirtab_launch(k_dirtab_fill<decltype(r)::value, true, KIND>, t, s)
                           : dirtab_launch(k_dirtab_fill<decltype(r)::value, false, KIND>, t, s);
    });
}

} // namespace

hipError_t dpx_launch_dirtab_fill(const dpx_dirtab_args &t, int algo, int R, hipStream_t stream) {
    if (t.d.numPairs <= 0) return hipSuccess;
    if (!t.tab.table || !t.tab.codeOf) return hipErrorInvalidValue;
    switch (algo) {
    case DPX_K_ANW: return launch_dirtab_kind<DPX_K_ANW>(t, R, stream);
    case DPX_K_ASW: return launch_dirtab_kind<DPX_K_ASW>(t, R, stream);
    case DPX_K_ASG: return launch_dirtab_kind<DPX_K_ASG>(t, R, stream);
    default: return hipErrorInvalidValue;
    }
}
