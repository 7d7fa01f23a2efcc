/*
 * dpx_scoretab_kernels.hip -- the fills of ANW / ASW / ASG score-only batches under a substitution table (dpx_batch_set_score_table): a
 * query scored against many sequences under a protein matrix, a read against many windows under a 5 x 5 matrix, scores and end cells
 * only.
 *
 * k_scoretab_fill<R, KIND> is the one-wave-per-pair fill of dpx_affine_kernels.hip -- dpx_affine_fill.inc, shared, with TABLE on and
 * STORE off -- and k_scoretab_lanes<KIND> the lane-packed one (dpx_affine_lanes.inc, R = 8), so schedule, borders, tie order and
 * end-cell rules are k_affine_fill's / k_affine_lanes' (KIND = DPX_K_ANW), k_asw_*'s (DPX_K_ASW) and k_asg_*'s (DPX_K_ASG).  One term
 * changes: the diagonal adds table[codeOf[reference byte] * 32 + codeOf[query byte]] in place of match / mismatch.  Every wave keeps
 * the 1280-byte image the band kernels use (dpx_kernels.h) in its own LDS behind its slice, translates its staged reference(s) to codes
 * once and its R query bytes once per stripe, and pays one signed-byte LDS read per cell for the compare-and-select it replaces.  The
 * image is kept TRANSPOSED in LDS and a lane's R row bases (image + (query code << 5)) are formed once, so a cell's address is one add
 * of the staged reference byte.  The lane-packed kernel keeps its state biased by (o+e); the table byte and the frame's -(o+e) enter
 * the diagonal term in one three-operand add (dpx_affine_dev.hpp: aff_cells_g).
 * No MFMA, no atomics, nothing stored but the three results per pair.
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

/* The table costs the one-wave kernels two to four VGPRs (the cell addresses and bytes in flight).  Left alone that costs ASW at R = 4 one
 * wave per SIMD against its plain twin (66 registers against 62).  Each instantiation is therefore held to its twin's occupancy -- 8
 * waves at R = 2 and 4; at R = 8 seven for ANW and five for ASW / ASG -- and fits it without scratch (tests/test_scoretab_kernels_isa.py
 * checks both against the plain unit's metadata). */
constexpr int scoretab_waves(int R, int KIND) { return R < 8 ? 8 : (KIND == DPX_K_ANW ? 7 : 5); }

template <int R, int KIND>
__global__ void __launch_bounds__(DPX_FILL_THREADS) __attribute__((amdgpu_waves_per_eu(scoretab_waves(R, KIND))))
k_scoretab_fill(const dpx_subst_args t) {
    constexpr bool LOCAL = KIND == DPX_K_ASW, SEMI = KIND == DPX_K_ASG, STORE = false, TABLE = true;
    const dpx_fill_args &a = t.f;
    const int8_t *const tableG = t.tab.table;
    const unsigned char *const codeOfG = t.tab.codeOf;
#include "dpx_affine_fill.inc"
}

template <int KIND>
__global__ void __launch_bounds__(DPX_ALANES_THREADS) k_scoretab_lanes(const dpx_subst_args t) {
    constexpr int R = 8;
    constexpr bool LOCAL = KIND == DPX_K_ASW, SEMI = KIND == DPX_K_ASG, STORE = false, TABLE = true;
    const dpx_fill_args &a = t.f;
    const int8_t *const tableG = t.tab.table;
    const unsigned char *const codeOfG = t.tab.codeOf;
#include "dpx_affine_lanes.inc"
}

/* f.wavesPerBlock waves per workgroup, f.ldsPerWave (image included) bytes of LDS each */
template <class K>
hipError_t scoretab_launch(K kernel, const dpx_subst_args &t, hipStream_t s) {
    const unsigned wpb = t.f.wavesPerBlock ? t.f.wavesPerBlock : 1u;
    return launch_lds(kernel, dim3(((unsigned)t.f.numPairs + wpb - 1) / wpb), dim3(64u * wpb), (size_t)t.f.ldsPerWave * wpb, s, t);
}

template <int KIND>
hipError_t launch_scoretab_kind(const dpx_subst_args &t, int R, hipStream_t s) {
    return dispatch_int<2, 4, 8>(R, [&](auto r) { return scoretab_launch(k_scoretab_fill<decltype(r)::value, KIND>, t, s); });
}

} // namespace

hipError_t dpx_launch_scoretab_fill(const dpx_subst_args &t, int algo, int R, hipStream_t stream) {
    if (t.f.numPairs <= 0) return hipSuccess;
    if (!t.tab.table || !t.tab.codeOf || t.f.ldsPerWave < DPX_SUBST_IMAGE_BYTES) return hipErrorInvalidValue;
    switch (algo) {
    case DPX_K_ANW: return launch_scoretab_kind<DPX_K_ANW>(t, R, stream);
    case DPX_K_ASW: return launch_scoretab_kind<DPX_K_ASW>(t, R, stream);
    case DPX_K_ASG: return launch_scoretab_kind<DPX_K_ASG>(t, R, stream);
    default: return hipErrorInvalidValue;
    }
}

hipError_t dpx_launch_scoretab_lanes(const dpx_subst_args &t, int algo, int R, hipStream_t stream) {
    if (t.f.numPairs <= 0) return hipSuccess;
    if (!t.tab.table || !t.tab.codeOf || R != 8 || t.f.wavesPerBlock != DPX_ALANES_THREADS / 64 || t.f.ldsPerWave < DPX_SUBST_IMAGE_BYTES) return hipErrorInvalidValue;
    switch (algo) {
    case DPX_K_ANW: return scoretab_launch(k_scoretab_lanes<DPX_K_ANW>, t, stream);
    case DPX_K_ASW: return scoretab_launch(k_scoretab_lanes<DPX_K_ASW>, t, stream);
    case DPX_K_ASG: return scoretab_launch(k_scoretab_lanes<DPX_K_ASG>, t, stream);
    default: return hipErrorInvalidValue;
    }
}
