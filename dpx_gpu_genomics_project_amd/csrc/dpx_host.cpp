/* dpx_host.cpp -- what dpx_host.h declares: the error path of every HIP call and the knob snapshot. */
#include "dpx_host.h"

#include <cstdlib>
#include <cstring>
#include <mutex>

namespace dpx_host {

int hip_fail(hipError_t e, const char *what) {
    t_err = std::string(what) + ": " + hipGetErrorString(e);
    (void)hipGetLastError();
    return e == hipErrorOutOfMemory ? DPX_ERR_NOMEM : DPX_ERR_HIP;
}

static std::mutex g_knobsMu;
static Knobs g_knobs;
void refresh_knobs() {
    auto num = [](const char *name, int unset) { const char *e = getenv(name); return e ? atoi(e) : unset; };
    Knobs k;
    k.rowsPerLane = num("DPX_R", 0);
    k.packed = num("DPX_PACKED", -1);
    k.lanes = num("DPX_LANES", -1);
    k.lanesPk = num("DPX_LANES_PK", -1);
    k.split = num("DPX_SPLIT", -1);
    k.rowTags = num("DPX_ROW_TAGS", -1);
    k.rampLines = num("DPX_RAMP_LINES", -1);
    k.wavesPerBlock = num("DPX_WPB", 0);
    k.group = num("DPX_GROUP", 0);
    k.tbWalk = num("DPX_TB_WALK", -1);
    k.poolProbe = num("DPX_POOL_PROBE", -1);
    { const char *e = getenv("DPX_POOL"); k.poolMalloc = e && !strcmp(e, "malloc"); }
    { const long v = num("DPX_POOL_CHUNK_MB", 0); k.poolChunkBytes = v > 0 ? (size_t)v << 20 : 0; }
    { const char *e = getenv("DPX_POOL_GUARD"); k.poolGuard = !e ? 0 : !strcmp(e, "selftest") ? 2 : 1; }
    k.trace = getenv("DPX_TRACE") != nullptr;
    k.traceVmm = getenv("DPX_TRACE_VMM") != nullptr;
    std::lock_guard<std::mutex> lk(g_knobsMu);
    g_knobs = k;
}
Knobs knobs() { std::lock_guard<std::mutex> lk(g_knobsMu); return g_knobs; }

} // namespace dpx_host
