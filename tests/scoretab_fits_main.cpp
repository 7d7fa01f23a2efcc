/* scoretab_fits_main.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_scoretab_lds_refusal.py compiles it beside csrc/dpx_plan.cpp, no GPU).
 * dpx_plan_scoretab_waves / _fits on hand-made plans: launch_scalars admits a plan only when four plain slices fit one workgroup, so no
 * plan that dpx_plan_batch makes reaches the refusal of dpx_batch_set_score_table for LDS; this drives the two helpers past that limit.
 * Input, one line per case: <main ldsPerWave> <main wavesPerBlock> <main numPairs> <lanePacked 0|1> <lanes ldsPerWave>
 * Output, one line per case: waves=<n> fits=<0|1> err=<text> */
#include <cstdio>
#include <string>

#include "../dpx_gpu_genomics_project_amd/csrc/dpx_plan.h"

int main() {
    unsigned perWave, waves, lanesPerWave;
    int numPairs, lanePacked;
    while (scanf("%u %u %d %d %u", &perWave, &waves, &numPairs, &lanePacked, &lanesPerWave) == 5) {
        dpx_plan p;
        p.args.ldsPerWave = perWave; p.args.wavesPerBlock = waves; p.args.numPairs = numPairs;
        p.lanePacked = lanePacked != 0; p.pkArgs.ldsPerWave = lanesPerWave; p.pkArgs.wavesPerBlock = 1;
        std::string err;
        const bool fits = dpx_plan_scoretab_fits(p, err);
        printf("waves=%u fits=%d err=%s\n", dpx_plan_scoretab_waves(p), fits ? 1 : 0, err.c_str());
    }
    return 0;
}
