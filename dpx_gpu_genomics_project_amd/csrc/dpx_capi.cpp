/*
 * dpx_capi.cpp -- implementation of include/dpx_align.h on the HIP runtime (host side of libdpxalign.so).
 *
 * Owns device memory, streams and launch geometry; the arithmetic is in the kernel units (dpx_kernels.hip and the other *_kernels.hip).  There is no CPU
 * fallback anywhere in this file: without a gfx950 device every entry point fails with DPX_ERR_NO_DEVICE.
 */
#include "../../include/dpx_align.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "dpx_cigar.h"
#include "dpx_diff.h"
#include "dpx_reverse.h"
#include "dpx_plan.h" /* (brings dpx_kernels.h, dpx_dir.h, dpx_banddir.h and dpx_layout.h) */

namespace {

std::mutex g_mu;
int g_device = -1;             /* default device: the one dpx_init() bound (dpx_batch_create, dpx_device_info, dpx_prim_eval) */
thread_local int t_device = -1; /* device of the call this thread is in (a batch's own device, or the default) */
thread_local std::string t_err;

int hip_fail(hipError_t e, const char *what) {
    t_err = std::string(what) + ": " + hipGetErrorString(e);
    (void)hipGetLastError();
    return e == hipErrorOutOfMemory ? DPX_ERR_NOMEM : DPX_ERR_HIP;
}
#define HIP_TRY(call)                                     \
    do {                                                  \
        hipError_t e__ = (call);                          \
        if (e__ != hipSuccess) return hip_fail(e__, #call); \
    } while (0)

/* Make `device` (-1: the default device, initialising device 0 if dpx_init() was never called) current for this thread.
 * Every buffer / stream cache entry carries its device, so one process can drive several GPUs: a batch lives on the
 * device it was created on and every call on it binds that device first. */
int bind_device(int device = -1) {
    if (device < 0) {
        if (g_device < 0) {
            int rc = dpx_init(0);
            if (rc != DPX_OK) return rc;
        }
        device = g_device;
    }
    HIP_TRY(hipSetDevice(device));
    t_device = device;
    return DPX_OK;
}

constexpr size_t kSmallResultBytes = 12288; /* score / end row / end column of a small batch, as they lie in the arena (dpx_batch_output_begin) */

/* The environment is read here and nowhere else; the snapshot everything else reads is dpx_plan.h's Knobs. */
std::mutex g_knobsMu;
Knobs g_knobs;
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

/* Parked buffers.  The matrix pool is by far the largest allocation (22 GB for the headline batch) and hipMalloc/hipFree
 * of that size cost 50-1000 ms -- the "memory management" slice that dominated the reference's V12 profile (187 of 440 ms)
 * and that it attacked by pooling (V9) and sizing once (V14); pinning ~70 MB of host memory costs ~10 ms; and even the
 * small calls add up when the reference's main.cpp aligns one pair per call from 20 threads.  So nothing a batch
 * allocates is freed when the batch goes away: buffers are parked per kind and handed to the next batch that fits
 * (batched drivers create same-sized batches back to back; the class-per-pair drivers create thousands of tiny ones). */
/* The matrix pool is not one hipMalloc.  Round 3 (tools/poolstudy.hip, profiles/r03/poolstudy.txt): one hipMalloc of 22 GB is
 * written by hipMemset at 6.3 TB/s or at 6.05 TB/s and by a streaming-store kernel at 5.5 or 4.8 TB/s depending on the
 * allocation -- although every single GiB of a "slow" allocation is written as fast as every GiB of a "fast" one, so the
 * mode is a property of how the runtime backed and mapped the whole range, not of where it lies.  The same range built from
 * the virtual-memory API -- one hipMemAddressReserve, physical chunks from hipMemCreate, hipMemMap -- was written at 6.5 - 7.2 TB/s
 * (memset) in every trial, and the headline fill follows: 3.62 ms on one hipMalloc, 3.2 - 3.35 ms on 256-MiB chunks (eight fresh
 * pools each, alternating in one process, profiles/r03/pool_ab_variants_*.txt; 1-GiB and 2-MiB chunks: wider spread, 3.28 - 3.61).
 * So every matrix pool of every caller is a chunked virtual range of 256-MiB chunks (DPX_POOL=malloc restores hipMalloc for
 * A/B runs; DPX_POOL_CHUNK_MB sets the chunk size).  Small pools (< 64 MiB) stay on hipMalloc: the class-per-pair drivers create
 * thousands of them. */
struct VmmRange {
    size_t bytes; int device; size_t chunkBytes;
    void *reserved; size_t reservedBytes; /* what hipMemAddressReserve returned (the pool starts at the first chunk-aligned address inside) */
    std::vector<std::pair<hipMemGenericAllocationHandle_t, size_t>> chunks;
};
std::mutex g_vmmMu;
std::map<void *, VmmRange> g_vmmRanges;
void forget_pool_record(void *pool);

/* Allocation granularity of device memory behind the virtual-memory API, queried once per device (round 4; rounds 1-3 assumed 2 MiB):
 * every chunk size, every mapping offset and the reserved range are multiples of the RECOMMENDED granularity, and the range is reserved
 * with the chunk size as its alignment, so a chunk never straddles a boundary of its own size. */
size_t vmm_granularity(int device) {
    static std::mutex mu;
    static std::map<int, size_t> known;
    std::lock_guard<std::mutex> lk(mu);
    auto it = known.find(device);
    if (it != known.end()) return it->second;
    hipMemAllocationProp prop;
    memset(&prop, 0, sizeof prop);
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = device;
    size_t gmin = 0, grec = 0;
    if (hipMemGetAllocationGranularity(&gmin, &prop, hipMemAllocationGranularityMinimum) != hipSuccess) { (void)hipGetLastError(); gmin = 0; }
    if (hipMemGetAllocationGranularity(&grec, &prop, hipMemAllocationGranularityRecommended) != hipSuccess) { (void)hipGetLastError(); grec = 0; }
    size_t g = std::max<size_t>({gmin, grec, (size_t)2 << 20});
    while (g & (g - 1)) g += g & (~g + 1); /* up to a power of two (it is one on every runtime seen) */
    if (knobs().traceVmm) { fprintf(stderr, "[vmm] device %d: allocation granularity minimum %zu recommended %zu -> %zu\n", device, gmin, grec, g); fflush(stderr); }
    known[device] = g;
    return g;
}

/* Tearing a range down.  ROCm 7.2 crashed inside hipMemAddressFree (SIGSEGV in libamdhip64, profiles/r03/vmm_address_free_crash.txt) in
 * about half the runs of the pool tests.  The crashing version (commit 46f7574) already undid every mapping with exactly the (address,
 * size) it was made with, released the handles and then freed the address range -- in this order; what the fix (c07d102) added, and
 * what the crash therefore depended on, are the two waits for the device: one before the first unmap (work of ANY stream of this
 * process, e.g. a hipMemsetAsync of the previous candidate or a fill on a side stream, may still touch the range) and one between the
 * releases and hipMemAddressFree (unmap / release are queued inside the runtime).  The two were added together and never separated;
 * both stay.  One hipMemUnmap over the whole range instead of one per chunk is a different bug: the chunks behind the first stayed
 * allocated (tools/pool_leak.py).  Every status is checked: on a failure the range stays in g_vmmRanges (nothing is freed twice, the
 * leak is visible) and the error is left in dpx_last_error(). */
bool vmm_release(void *va, VmmRange &r, size_t mappedBytes) {
    const bool dbg = knobs().traceVmm;
    if (dbg) { fprintf(stderr, "[vmm] release [%p, %p) mapped %zu chunks %zu\n", va, (void *)((char *)va + r.bytes), mappedBytes, r.chunks.size()); fflush(stderr); }
    int cur = -1;
    (void)hipGetDevice(&cur);
    if (r.device >= 0 && r.device != cur) (void)hipSetDevice(r.device); /* (one process may drive several devices: wait for the range's own) */
    hipError_t bad = hipDeviceSynchronize();
    const char *where = "hipDeviceSynchronize";
    size_t off = 0;
    for (auto &c : r.chunks) {
        if (bad == hipSuccess && off + c.second <= mappedBytes) { bad = hipMemUnmap((char *)va + off, c.second); where = "hipMemUnmap"; }
        off += c.second;
    }
    for (auto &c : r.chunks) {
        if (bad != hipSuccess) break;
        bad = hipMemRelease(c.first);
        where = "hipMemRelease";
    }
    if (bad == hipSuccess) { bad = hipDeviceSynchronize(); where = "hipDeviceSynchronize"; }
    if (bad == hipSuccess) { bad = hipMemAddressFree(r.reserved, r.reservedBytes); where = "hipMemAddressFree"; }
    if (bad != hipSuccess) {
        t_err = std::string("matrix pool teardown: ") + where + ": " + hipGetErrorString(bad);
        if (dbg) { fprintf(stderr, "[vmm] %s\n", t_err.c_str()); fflush(stderr); }
        (void)hipGetLastError();
    } else if (dbg) { fprintf(stderr, "[vmm] done\n"); fflush(stderr); }
    if (r.device >= 0 && r.device != cur && cur >= 0) (void)hipSetDevice(cur);
    return bad == hipSuccess;
}

hipError_t pool_alloc(void **out, size_t bytes) {
    const Knobs kn = knobs();
    const bool useMalloc = kn.poolMalloc;
    const size_t chunkEnv = kn.poolChunkBytes;
    if (useMalloc || bytes < ((size_t)64 << 20) || t_device < 0) return hipMalloc(out, bytes);
    const size_t gran = vmm_granularity(t_device);
    size_t chunk = std::max(chunkEnv ? chunkEnv : (size_t)256 << 20, gran);
    while (chunk & (chunk - 1)) chunk += chunk & (~chunk + 1); /* a power of two >= the granularity: it is the alignment of the reserved range */
    VmmRange r;
    r.bytes = align_up(bytes, gran);
    r.device = t_device;
    r.chunkBytes = chunk;
    /* hipMemAddressReserve of ROCm 7.2 ignores its alignment argument (ranges come back 2-MiB aligned whatever is asked for:
     * profiles/r04/vmm_granularity_and_alignment.txt), so the range is reserved one chunk longer and the pool starts at the first
     * chunk-aligned address inside it: every chunk is mapped at a multiple of its own size */
    const size_t align = chunk; /* (2 MiB, 256 MiB or 1 GiB: the fills do not care, profiles/r04/vmm_granularity_and_alignment.txt) */
    r.reservedBytes = r.bytes + align;
    r.reserved = nullptr;
    hipError_t e = hipMemAddressReserve(&r.reserved, r.reservedBytes, align, nullptr, 0);
    if (e != hipSuccess) { (void)hipGetLastError(); return hipMalloc(out, bytes); }
    void *va = (void *)align_up((size_t)(uintptr_t)r.reserved, align);
    hipMemAllocationProp prop;
    memset(&prop, 0, sizeof prop);
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = t_device;
    size_t mapped = 0;
    for (size_t off = 0; off < r.bytes && e == hipSuccess; off += chunk) {
        const size_t sz = std::min(chunk, r.bytes - off); /* (the last one: a multiple of the granularity, like r.bytes) */
        hipMemGenericAllocationHandle_t h;
        e = hipMemCreate(&h, sz, &prop, 0);
        if (e != hipSuccess) break;
        r.chunks.emplace_back(h, sz);
        e = hipMemMap((char *)va + off, sz, 0, h, 0);
        if (e == hipSuccess) mapped += sz;
    }
    if (e == hipSuccess) {
        hipMemAccessDesc acc;
        memset(&acc, 0, sizeof acc);
        acc.location.type = hipMemLocationTypeDevice;
        acc.location.id = t_device;
        acc.flags = hipMemAccessFlagsProtReadWrite;
        e = hipMemSetAccess(va, r.bytes, &acc, 1);
    }
    if (e != hipSuccess) {
        if (kn.traceVmm) { fprintf(stderr, "[vmm] building %p failed after %zu of %zu bytes mapped: %s\n", va, mapped, r.bytes, hipGetErrorString(e)); fflush(stderr); }
        (void)vmm_release(va, r, mapped);
        if (e == hipErrorOutOfMemory) return e;
        /* a runtime without (working) virtual-memory management: one hipMalloc, as before round 3 -- slower to write, never wrong */
        (void)hipGetLastError();
        return hipMalloc(out, bytes);
    }
    if (kn.traceVmm) { fprintf(stderr, "[vmm] alloc [%p, %p) chunks %zu of %zu MiB\n", va, (void *)((char *)va + r.bytes), r.chunks.size(), chunk >> 20); fflush(stderr); }
    { std::lock_guard<std::mutex> lk(g_vmmMu); g_vmmRanges.emplace(va, std::move(r)); }
    *out = va;
    return hipSuccess;
}

/* how the pool at `p` was built: chunk size of a virtual range, 0 for one hipMalloc */
size_t pool_chunk_bytes(void *p) {
    std::lock_guard<std::mutex> lk(g_vmmMu);
    auto it = g_vmmRanges.find(p);
    return it == g_vmmRanges.end() ? 0 : it->second.chunkBytes;
}

void pool_free(void *p) {
    if (!p) return;
    forget_pool_record(p); /* (a later pool at the same address must not inherit this one's timings) */
    VmmRange r;
    bool found = false;
    {
        std::lock_guard<std::mutex> lk(g_vmmMu);
        auto it = g_vmmRanges.find(p);
        if (it != g_vmmRanges.end()) { r = std::move(it->second); g_vmmRanges.erase(it); found = true; }
    }
    if (!found) { (void)hipFree(p); return; }
    if (!vmm_release(p, r, r.bytes)) { std::lock_guard<std::mutex> lk(g_vmmMu); g_vmmRanges.emplace(p, std::move(r)); } /* kept: see vmm_release */
}

class BufCache {
public:
    enum Kind { Device, PinnedHost, DevicePool };
    BufCache(Kind kind, size_t maxEntries, size_t maxBytes) : kind_(kind), maxEntries_(maxEntries), maxBytes_(maxBytes) {}

    /* a parked buffer of [need, 1.5 * need + 1 MiB], else a fresh allocation (after an out-of-memory: drop everything
     * that is parked anywhere and retry once) */
    hipError_t take(void **out, size_t need, size_t *actual, bool *fresh = nullptr);
    void discard(void *ptr) { raw_free(ptr); } /* a buffer that will not be parked */
    void park(void *ptr, size_t bytes);
    void drain();

private:
    struct Entry { void *ptr; size_t bytes; int device; };
    hipError_t raw_alloc(void **out, size_t bytes) const {
        return kind_ == Device ? hipMalloc(out, bytes) : kind_ == DevicePool ? pool_alloc(out, bytes) : hipHostMalloc(out, bytes, hipHostMallocDefault);
    }
    void raw_free(void *p) const {
        if (!p) return;
        if (kind_ == DevicePool) pool_free(p);
        else (void)(kind_ == Device ? hipFree(p) : hipHostFree(p));
    }
    const Kind kind_;
    const size_t maxEntries_, maxBytes_;
    std::mutex mu_;
    std::vector<Entry> parked_; /* oldest first */
    size_t total_ = 0;
};

void trim_all_caches();

hipError_t BufCache::take(void **out, size_t need, size_t *actual, bool *fresh) {
    if (fresh) *fresh = false;
    {
        std::lock_guard<std::mutex> lk(mu_);
        size_t best = parked_.size();
        for (size_t i = 0; i < parked_.size(); i++) {
            const Entry &e = parked_[i];
            /* (a parked matrix pool of up to 13 GiB serves any smaller batch: a driver that cuts a file into batches of one pool
             * budget ends with a short batch, and a pool reserved ahead of time -- dpx_pool_reserve -- is sized by the budget) */
            /* (a parked pinned buffer of up to 32 MiB -- dpx_text_reserve -- serves any smaller text) */
            /* (... but not a tiny one: the class-per-pair drivers create thousands of batches of a few MiB, which stay on hipMalloc) */
            const size_t roof = (kind_ == DevicePool && need >= ((size_t)64 << 20)) ? std::max(need + need / 2 + (1u << 20), (size_t)13 << 30)
                                : (kind_ == PinnedHost && need >= ((size_t)2 << 20)) ? std::max(need + need / 2 + (1u << 20), (size_t)32 << 20) : need + need / 2 + (1u << 20);
            if (e.device != t_device || e.bytes < need || e.bytes > roof) continue;
            if (best == parked_.size() || e.bytes < parked_[best].bytes) best = i;
        }
        if (best != parked_.size()) {
            *out = parked_[best].ptr;
            *actual = parked_[best].bytes;
            total_ -= parked_[best].bytes;
            parked_.erase(parked_.begin() + (long)best);
            return hipSuccess;
        }
    }
    /* a fresh buffer gets 1/8 of headroom (and a 64 KiB granule) so that the next batch of about the same size can take
     * it over: batches of one file differ by a few per cent, and pinning 8 MB costs ~1 ms every time it misses */
    const size_t want = need < ((size_t)1 << 30) ? align_up(need + need / 8, (size_t)64 << 10) : need;
    *actual = want;
    if (fresh) *fresh = true;
    hipError_t e = raw_alloc(out, want);
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        trim_all_caches();
        *actual = need;
        e = raw_alloc(out, need);
    }
    return e;
}

void BufCache::park(void *ptr, size_t bytes) {
    if (!ptr) return;
    std::vector<void *> evicted;
    {
        std::lock_guard<std::mutex> lk(mu_);
        if (t_device < 0 || bytes > maxBytes_) {
            evicted.push_back(ptr);
        } else {
            /* per device: at most one parked buffer of 16 GiB or more, at most eight of a GiB or more and 48 GiB of them (a pipelined driver
             * keeps up to eight batches in flight on pools of a few GiB each -- dpx_main -inflight; tens of GB twice over is not worth holding) */
            const size_t big = (size_t)1 << 30, huge = (size_t)16 << 30;
            size_t bigOnes = 0, bigBytes = bytes;
            for (size_t i = parked_.size(); i-- > 0;) { /* newest first: the oldest go */
                if (parked_[i].device != t_device || parked_[i].bytes < big || bytes < big) continue;
                bigBytes += parked_[i].bytes;
                const bool drop = bytes >= huge || parked_[i].bytes >= huge || ++bigOnes >= 8 || bigBytes > ((size_t)48 << 30);
                if (drop) { evicted.push_back(parked_[i].ptr); total_ -= parked_[i].bytes; parked_.erase(parked_.begin() + (long)i); }
            }
            while (!parked_.empty() && (parked_.size() >= maxEntries_ || total_ + bytes > maxBytes_)) {
                evicted.push_back(parked_.front().ptr);
                total_ -= parked_.front().bytes;
                parked_.erase(parked_.begin());
            }
            parked_.push_back(Entry{ptr, bytes, t_device});
            total_ += bytes;
        }
    }
    for (void *p : evicted) raw_free(p);
}

void BufCache::drain() {
    std::vector<Entry> gone;
    {
        std::lock_guard<std::mutex> lk(mu_);
        gone.swap(parked_);
        total_ = 0;
    }
    for (const Entry &e : gone) raw_free(e.ptr);
}

/* what a batch allocates: the int16 matrices, the arena of small arrays, the traceback line buffers (device + pinned) */
BufCache g_matCache(BufCache::DevicePool, 64, (size_t)96 << 30), g_arenaCache(BufCache::Device, 64, (size_t)2 << 30),
    g_tbDevCache(BufCache::Device, 64, (size_t)8 << 30), g_tbHostCache(BufCache::PinnedHost, 64, (size_t)2 << 30),
    g_stageCache(BufCache::PinnedHost, 64, (size_t)64 << 20); /* upload images of small batches (dpx_batch_create: one H2D instead of five) */

/* hipStreamCreate / hipStreamDestroy cost ~2 ms each on this stack: a finished batch parks its (idle) stream */
struct StreamCache {
    std::mutex mu;
    std::vector<std::pair<hipStream_t, int>> parked; /* (stream, device) */
} g_streams;

hipError_t stream_take(hipStream_t *out) {
    {
        std::lock_guard<std::mutex> lk(g_streams.mu);
        /* the most recently parked one first: a pipeline of two batches in flight then keeps using the same two streams.  The runtime
         * maps streams onto four hardware queues; cycling through six parked streams put the fill of batch k+1 on the queue of batch
         * k's traceback every few batches, where it waited for it (profiles/r04/e2e_long_timeline_*.txt) */
        for (size_t i = g_streams.parked.size(); i-- > 0;)
            if (g_streams.parked[i].second == t_device) {
                *out = g_streams.parked[i].first;
                g_streams.parked.erase(g_streams.parked.begin() + (long)i);
                return hipSuccess;
            }
    }
    return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
}

void stream_park(hipStream_t s) {
    if (!s) return;
    {
        std::lock_guard<std::mutex> lk(g_streams.mu);
        if (g_streams.parked.size() < 256 && t_device >= 0) { g_streams.parked.emplace_back(s, t_device); return; }
    }
    (void)hipStreamDestroy(s);
}

void trim_all_caches() {
    std::vector<std::pair<hipStream_t, int>> st;
    { std::lock_guard<std::mutex> lk(g_streams.mu); st.swap(g_streams.parked); }
    for (auto &e : st) (void)hipStreamDestroy(e.first);
    g_matCache.drain();
    g_arenaCache.drain();
    g_tbDevCache.drain();
    g_tbHostCache.drain();
    g_stageCache.drain();
}

} // namespace

namespace {
/* DPX_TRACE=1: phase timings of dpx_batch_create / destroy on stderr (development aid) */
struct PhaseTrace {
    bool on = knobs().trace;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void mark(const char *what) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[dpx] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t).count());
        t = now;
    }
};
} // namespace

/* The record of a matrix pool: how it was built and how fast hipMemset writes it (dpx_batch_describe -> bench.py's roofline.pool),
 * so that a slow run can be attributed to the pool or to something else.  Kept per pool address for the life of the pool (a
 * parked pool keeps its record for the next batch). */
struct PoolRecord {
    std::string mode = "malloc";
    size_t bytes = 0, chunkBytes = 0;
    std::vector<float> candidatesMs; /* hipMemset time of every candidate allocation (empty: never timed) */
    std::vector<float> fillMs;       /* time of one fill of the batch on every candidate (empty: never shopped) */
    std::vector<std::string> kinds;  /* how every candidate was built: "vmm256", "malloc" ... (empty: never shopped) */
    std::vector<std::string> ranges; /* "address+bytes" of every candidate (a GPU fault address can be placed against them) */
    int kept = 0;
};
static std::mutex g_poolRecMu;
static std::map<void *, PoolRecord> g_poolRecords;
namespace { void forget_pool_record(void *pool) { std::lock_guard<std::mutex> lk(g_poolRecMu); g_poolRecords.erase(pool); } }
/* the record of a pool nobody has timed yet: how it was built (looked up by address: the pool may have been built by another thread) */
static PoolRecord fresh_pool_record(void *pool, size_t bytes) {
    PoolRecord rec;
    const size_t chunk = pool_chunk_bytes(pool);
    rec.mode = chunk ? "vmm" : "malloc";
    rec.chunkBytes = chunk;
    rec.bytes = bytes;
    return rec;
}

/* A batch is its plan (dpx_plan.h: what was decided, the pair table, the launch arguments) plus everything that lives on the device. */
struct dpx_batch : dpx_plan {
    int device = -1; /* the device the batch lives on */
    bool filled = false;
    size_t matPoolBytes = 0; /* bytes of the block behind dMat (may exceed matElems*2 when a parked pool was reused) */
    size_t guardBytes = 0;   /* DPX_POOL_GUARD: pattern bytes behind the matrices, checked by dpx_batch_sync() */
    bool guardSelfTest = false;
    char *dSeq = nullptr;
    dpx_pair_dev *dPairs = nullptr;
    int32_t *dOrder = nullptr;
    char *arena = nullptr;   /* one device allocation behind dSeq, dPairs, dScore/dEndRow/dEndCol, dOrder, dCouples, dTbOff, dTbLen
                                (parked and reused across batches like the matrix pool: 9 hipMalloc/hipFree pairs per batch otherwise) */
    size_t arenaCap = 0;
    int16_t *dMat = nullptr;
    int32_t *dScore = nullptr, *dEndRow = nullptr, *dEndCol = nullptr;
    hipStream_t stream = nullptr;     /* the batch's own stream */
    hipStream_t sideStream = nullptr; /* secondary kernels of a fill run here, concurrently with the main one (launch_all) */
    hipEvent_t evFork = nullptr, evJoin = nullptr;
    hipEvent_t evT0 = nullptr, evT1 = nullptr; /* DPX_TIME_FILLS: recorded around every dpx_batch_fill() */
    hipEvent_t evOrder = nullptr;              /* orders the output path behind a fill that ran on a caller's stream */
    hipEvent_t evOut0 = nullptr, evOut1 = nullptr; /* DPX_TIME_FILLS: around the traceback + text kernels of dpx_batch_output_begin() */
    bool outTimed = false;
    bool fillTimed = false;
    hipStream_t lastStream = nullptr; /* stream of the most recent fill (caller's or own) */
    int32_t *dCouples = nullptr; /* the couples of the packed kernels, or the wave descriptors of the lane-packed ones */
    /* result text (lazy): device line buffers of k_traceback, the packed blocks built from them, pinned host mirrors */
    uint64_t *dTbOff = nullptr;
    char *dTb = nullptr;
    int32_t *dTbLen = nullptr;
    uint64_t *dOutOff = nullptr, *dOutScratch = nullptr; /* per-pair byte offsets of the blocks (+ total), scan scratch */
    char *dOut = nullptr;
    char *hStage = nullptr; /* pinned image of the arena's uploaded front (small batches), alive until the batch is destroyed */
    size_t hStageCap = 0;
    bool resultsCopied = false; /* ... and of score / end row / end column, into the tail of hMeta */
    bool textCopied = false;    /* dpx_batch_output_begin() has queued the text's D2H itself (small batches) */
    bool uploadPending = false; /* ... and its one asynchronous H2D on b->stream has not been waited for by anybody yet */
    char *hMeta = nullptr; /* pinned: uint64 offsets[numPairs + 1], then int32 alignment lengths[numPairs] */
    char *hOut = nullptr;  /* pinned: the packed text */
    size_t hOutBytes = 0;
    size_t dTbCap = 0, dOutCap = 0, hMetaCap = 0, hOutCap = 0; /* capacities of the (possibly recycled) buffers */
    bool tbLinesValid = false; /* k_traceback has run since the last fill */
    int outState = 0;          /* 0 none, 1 dpx_batch_output_begin() in flight, 2 text on the host */
    uint64_t outFirst = 0;     /* pair number of the batch's first pair in the text */
    /* CIGARs (dpx_batch_cigars_begin / _end): built from the same traceback lines as the text, with buffers of their own so that the
     * two output paths may follow one fill in either order */
    int cigarState = 0;        /* 0 none, 1 dpx_batch_cigars_begin() in flight, 2 records and ops on the host */
    unsigned cigarFlags = 0;
    char *dCigar = nullptr;    /* device: dpx_alignment[numPairs], uint64 total, uint64 tile sums of the scan */
    uint32_t *dCigarOps = nullptr; /* device: one op per column at worst */
    char *hCigar = nullptr;    /* pinned: dpx_alignment[numPairs], uint64 total */
    uint32_t *hCigarOps = nullptr; /* pinned: exactly the ops */
    size_t dCigarCap = 0, dCigarOpsCap = 0, hCigarCap = 0, hCigarOpsCap = 0;
    uint64_t cigarOps = 0;     /* total number of ops (state 2) */
    /* difference strings (dpx_batch_diffs_begin / _end), index 0: MD, 1: cs -- from the same lines again, with buffers of their own per kind */
    int diffState[2] = {0, 0};             /* 0 none, 1 dpx_batch_diffs_begin() in flight, 2 text on the host */
    char *dDiffOff[2] = {nullptr, nullptr};  /* device: uint64 offsets[numPairs + 1], uint64 tile sums of the scan */
    char *dDiffText[2] = {nullptr, nullptr}; /* device: the size of the line buffer (three times the line capacity per pair at worst) */
    char *hDiffOff[2] = {nullptr, nullptr};  /* pinned: uint64 offsets[numPairs + 1] */
    char *hDiffText[2] = {nullptr, nullptr}; /* pinned: exactly the strings and one NUL */
    size_t dDiffOffCap[2] = {0, 0}, dDiffTextCap[2] = {0, 0}, hDiffOffCap[2] = {0, 0}, hDiffTextCap[2] = {0, 0};
    /* BAXT's extension mode (dpx_batch_set_extension): the next fill runs k_zext_fill while either value is >= 0 */
    int32_t zdrop = -1, endBonus = -1;
    bool extFilled = false;    /* the last fill ran the extension scan (k_zext_fill, k_zsub_fill, k_bdx_fill with zdrop or endBonus on): dExt holds its
                                  records, and dpx_batch_matrix / dpx_batch_directions mask behind lastDiag */
    int32_t *dExt = nullptr;   /* device: dpx_extension[numPairs] */
    size_t dExtCap = 0;
    /* substitution table (dpx_batch_set_substitution): while substAlphabet > 0 the fills run k_subst_fill and the walks k_subst_traceback*
     * (band-direction batches: k_bdx_fill; ANW / ASW / ASG direction batches, dpx_batch_set_direction_table: k_dirtab_fill, the walk stays;
     * their score-only batches, dpx_batch_set_score_table: k_scoretab_fill / k_scoretab_lanes) */
    int substAlphabet = 0;
    unsigned char *dSubst = nullptr; /* device: the table at row stride 32 (DPX_SUBST_TABLE_BYTES), then codeOf[256] */
    size_t dSubstCap = 0;
    std::vector<unsigned char> tableImage; /* the image dSubst holds while substAlphabet != 0 (every table setter keeps it, every clear drops it) */
    /* orientation (dpx_batch_set_reversed): while revCount > 0 dSeq points at dRev, the setter's own allocation -- [the arena's sequence
     * bytes][reversed copies of the flagged pairs' strings][the kernel's job list][the flagged pairs' numbers] -- and the flagged pairs'
     * indices in `pairs` / dPairs at the copies.  The fills, walks and exports know nothing of it. */
    char *dSeqOwn = nullptr;     /* the arena's sequence bytes (== dSeq while no mask is set) */
    size_t seqBytes = 0;         /* ... and their padded size */
    char *dRev = nullptr;
    size_t dRevCap = 0;
    const int32_t *dFlagged = nullptr; /* inside dRev: revCount pair numbers, ascending */
    size_t revCount = 0;
    struct RevSaved { int32_t pair, refIdx, qryIdx; };
    std::vector<RevSaved> revSaved;    /* the flagged pairs' own indices, for the next call of the setter */
    PoolRecord poolRec;    /* how the matrix pool behind dMat was built / timed */
    bool tunePool = false, tuneShop = false; /* DPX_TUNE_PLACEMENT: the pool is timed / shopped for at the end of dpx_batch_create */
};

extern "C" {

int dpx_abi_version(void) { return DPX_ABI_VERSION; }

const char *dpx_strerror(int status) {
    switch (status) {
    case DPX_OK: return "ok";
    case DPX_ERR_INVALID: return "invalid argument";
    case DPX_ERR_NO_DEVICE: return "no usable HIP device (this library has no CPU fallback)";
    case DPX_ERR_HIP: return "HIP runtime error";
    case DPX_ERR_RANGE: return "scores of this batch do not fit the int16 matrix cells";
    case DPX_ERR_NOMEM: return "out of memory";
    case DPX_ERR_NOT_FILLED: return "batch has not been filled yet";
    case DPX_ERR_NO_MATRIX: return "batch was created with DPX_SCORE_ONLY";
    case DPX_ERR_UNSUPPORTED: return "unsupported parameter combination";
    default: return "unknown status";
    }
}

const char *dpx_last_error(void) { return t_err.c_str(); }

int dpx_device_count(int *count) {
    if (!count) return DPX_ERR_INVALID;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { (void)hipGetLastError(); *count = 0; return DPX_ERR_NO_DEVICE; }
    *count = n;
    return DPX_OK;
}

int dpx_init(int device) {
    refresh_knobs();
    std::lock_guard<std::mutex> lk(g_mu);
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        t_err = "hipGetDeviceCount found no device";
        return DPX_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= n) return DPX_ERR_INVALID;
    e = hipSetDevice(device);
    if (e != hipSuccess) { hip_fail(e, "hipSetDevice"); return DPX_ERR_NO_DEVICE; }
    const bool first = g_device != device;
    g_device = device;
    t_device = device;
    if (first) {
        /* One-time costs of the HIP runtime belong to device initialisation (the reference's mains likewise create their
         * context and query the device before they start their timer, cuda/LNW/LinearNeedlemanWunschV19.cu:357-409):
         * the first hipStreamCreate costs ~9 ms, the first pageable H2D / D2H another ~9 ms (runtime staging buffers).
         * Two streams go to the stream cache, and a small copy runs in each direction.  The first ASYNCHRONOUS copy into pinned host
         * memory on a stream costs another ~18 ms (round 3, DPX_TRACE of dpx_main: "output: D2H text 18.7 ms" for the first batch's
         * 5 MB, 0.3 ms for every later one): one such copy of 4 MiB runs here, in both directions, on both parked streams. */
        hipStream_t s0 = nullptr, s1 = nullptr;
        const bool have0 = hipStreamCreateWithFlags(&s0, hipStreamNonBlocking) == hipSuccess;
        const bool have1 = hipStreamCreateWithFlags(&s1, hipStreamNonBlocking) == hipSuccess;
        void *d = nullptr;
        std::vector<char> h((size_t)1 << 20, 0);
        const size_t warm = (size_t)4 << 20;
        if (hipMalloc(&d, warm) == hipSuccess) {
            (void)hipMemcpy(d, h.data(), h.size(), hipMemcpyHostToDevice);
            (void)hipMemcpy(h.data(), d, h.size(), hipMemcpyDeviceToHost);
            void *pinned = nullptr;
            if (hipHostMalloc(&pinned, warm, hipHostMallocDefault) == hipSuccess) {
                for (hipStream_t s : {have0 ? s0 : nullptr, have1 ? s1 : nullptr}) {
                    if (!s) continue;
                    (void)hipMemcpyAsync(pinned, d, warm, hipMemcpyDeviceToHost, s);
                    (void)hipMemcpyAsync(d, pinned, warm, hipMemcpyHostToDevice, s);
                    (void)hipStreamSynchronize(s);
                }
                (void)hipHostFree(pinned);
            }
            (void)hipFree(d);
        }
        if (have0) stream_park(s0);
        if (have1) stream_park(s1);
        (void)hipGetLastError();
    }
    return DPX_OK;
}

int dpx_device_info(char *name, size_t nameCap, int *computeUnits, size_t *hbmBytes) {
    int rc = bind_device();
    if (rc != DPX_OK) return rc;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, t_device));
    if (name && nameCap) { snprintf(name, nameCap, "%s (%s)", prop.name, prop.gcnArchName); }
    if (computeUnits) *computeUnits = prop.multiProcessorCount;
    if (hbmBytes) *hbmBytes = prop.totalGlobalMem;
    return DPX_OK;
}

/* Allocate `count` matrix pools of `bytes` on the default device and park them for the batches to come.  A driver calls this
 * on a helper thread while it is still parsing its input: building a pool costs tens of ms per GiB (the reference's V9 / V14
 * lesson: size the buffers once, outside the loop -- cuda/LNW/LinearNeedlemanWunschV9.cu:26-46, V14.cu:144-213). */
int dpx_pool_reserve(size_t bytes, int count) {
    if (count < 1 || count > 8 || bytes == 0) return DPX_ERR_INVALID;
    if (bytes >= ((size_t)16 << 30)) count = 1; /* (only one pool of 16 GiB or more stays parked per device: a second one would be built and dropped at once) */
    int rc = bind_device();
    if (rc != DPX_OK) return rc;
    void *p[8] = {nullptr};
    size_t got[8] = {0};
    for (int k = 0; k < count; k++) {
        bool fresh = false;
        hipError_t e = g_matCache.take(&p[k], bytes, &got[k], &fresh);
        if (e != hipSuccess) { for (int j = 0; j < k; j++) g_matCache.park(p[j], got[j]); return hip_fail(e, "dpx_pool_reserve"); }
    }
    for (int k = 0; k < count; k++) {
        { /* the pool's record, for the batch (of whatever thread) that takes it */
            std::lock_guard<std::mutex> lk(g_poolRecMu);
            if (!g_poolRecords.count(p[k])) g_poolRecords[p[k]] = fresh_pool_record(p[k], got[k]);
        }
        g_matCache.park(p[k], got[k]);
    }
    /* ... and the streams of the batches that will take the pools: a batch runs on its own stream plus a side stream for the pairs its
     * main kernel leaves over (an odd pair beside the couples of the packed kernel), and creating a stream costs ~10 ms each time the
     * cache is empty (DPX_TRACE of the batched driver: "create: stream 9.6 ms" twice for two batches in flight) */
    {
        hipStream_t extra[10] = {nullptr};
        int made = 0;
        for (int k = 0; k < count + 2; k++) /* (one per batch in flight + two for side kernels) */
            if (hipStreamCreateWithFlags(&extra[made], hipStreamNonBlocking) == hipSuccess) made++;
            else (void)hipGetLastError();
        for (int k = 0; k < made; k++) stream_park(extra[k]);
    }
    return DPX_OK;
}

/* The same for the pinned host buffers that the result text of a batch is copied into (dpx_batch_output_end / _take): pinning
 * 8 MB costs 1-2 ms, and a pipelined driver holds up to three of them (one being printed, two batches in flight). */
int dpx_text_reserve(size_t bytes, int count) {
    if (count < 1 || count > 9 || bytes == 0 || bytes > ((size_t)1 << 30)) return DPX_ERR_INVALID;
    int rc = bind_device();
    if (rc != DPX_OK) return rc;
    void *p[9] = {nullptr};
    size_t got[9] = {0};
    for (int k = 0; k < count; k++) {
        hipError_t e = g_tbHostCache.take(&p[k], bytes, &got[k]);
        if (e != hipSuccess) { for (int j = 0; j < k; j++) g_tbHostCache.park(p[j], got[j]); return hip_fail(e, "dpx_text_reserve"); }
    }
    for (int k = 0; k < count; k++) g_tbHostCache.park(p[k], got[k]);
    return DPX_OK;
}

int dpx_shutdown(void) {
    trim_all_caches();
    std::lock_guard<std::mutex> lk(g_mu);
    g_device = -1;
    return DPX_OK;
}

/* ------------------------------------------------------------------------------------------ batch */

/* hipMemset time of a pool (the record of a pool that a resident-batch caller is going to fill many times; 2 x 3.5 ms for 22 GB) */
static float time_memset(void *p, size_t bytes, hipStream_t s) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (hipEventCreate(&e0) != hipSuccess) { (void)hipGetLastError(); return -1.f; }
    if (hipEventCreate(&e1) != hipSuccess) { (void)hipGetLastError(); (void)hipEventDestroy(e0); return -1.f; }
    float best = 1e30f;
    for (int k = 0; k < 2; k++) {
        float ms = 1e30f;
        if (hipEventRecord(e0, s) != hipSuccess || hipMemsetAsync(p, 0, bytes, s) != hipSuccess || hipEventRecord(e1, s) != hipSuccess ||
            hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) { (void)hipGetLastError(); best = -1.f; break; }
        best = std::min(best, ms);
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return best;
}

static dpx_route route_of(const dpx_batch *b);
static hipError_t launch_all(dpx_batch *b, const dpx_route &r, hipStream_t s);

/* DPX_TUNE_PLACEMENT (callers that fill a resident batch many times: bench.py, iterative drivers).  The same fill runs up to
 * 27 % apart on two pools of the same construction (ANW 1000 x 1024^2: 1.05 vs 1.20 ms, alternating from one allocation to the
 * next while hipMemset sees no difference; LSW 10k x 1024^2: +-2 %; tools/mode_watch.py, profiles/r03/): the mode belongs to the
 * allocation -- where its physical chunks lie -- and only the fill itself shows it.  So the batch shops with its own fill: up to five
 * candidate pools of the SAME construction, one warm-up + three timed fills each, the fastest is kept (and parked for later batches),
 * the losers are freed together when the last candidate has been timed.  Every candidate's address range and times go into the pool
 * record (dpx_batch_describe -> bench.py roofline.pool; fillMs[0] is the pool a caller without the flag would have got).
 * Round 3 also compared CONSTRUCTIONS here (candidates of 512-MiB, 1-GiB and 2-GiB chunks): twice in ~60 runs a process died with a GPU
 * memory access fault while such a candidate was being filled (profiles/r03/gpu_fault_while_shopping.txt), never in hundreds of runs on
 * 256-MiB chunks.  Those ranges were reserved with alignment 0 and their chunks mapped at offsets that were multiples of 2 MiB only, not
 * of the chunk size or of the queried granularity (pool_alloc now reserves with the chunk size as alignment); whether that was the
 * cause cannot be shown from one clean run, so the branch is gone (round 4) rather than shipped on trust. */
static void shop_pool_by_fill(dpx_batch *b, PoolRecord &rec, PhaseTrace &trace) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (hipEventCreate(&e0) != hipSuccess) { (void)hipGetLastError(); return; }
    if (hipEventCreate(&e1) != hipSuccess) { (void)hipGetLastError(); (void)hipEventDestroy(e0); return; }
    auto set_pool = [&](void *p) {
        b->dMat = (int16_t *)p; b->args.mat = b->dMat; b->pkArgs.mat = b->dMat;
        if (b->dirs) { /* the codes and the long-reference area live in the pool as well */
            b->dirArgs.codes = reinterpret_cast<uint8_t *>(p);
            b->dirArgs.scratch = b->dirScratch ? reinterpret_cast<unsigned char *>(p) + b->matElems * sizeof(int16_t) : nullptr;
        }
    };
    const dpx_route route = route_of(b);
    auto time_fill = [&]() -> float {
        float ms = -1.f;
        hipError_t e = launch_all(b, route, b->stream);
        if (e == hipSuccess) e = hipEventRecord(e0, b->stream);
        for (int i = 0; i < 3 && e == hipSuccess; i++) e = launch_all(b, route, b->stream);
        if (e == hipSuccess) e = hipEventRecord(e1, b->stream);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        if (e != hipSuccess) { (void)hipGetLastError(); return -1.f; }
        return ms / 3.f;
    };
    auto kind_of = [](void *pool) { const size_t c = pool_chunk_bytes(pool); return c ? "vmm" + std::to_string(c >> 20) : std::string("malloc"); };
    auto range_of = [&](void *pool) { char t[64]; snprintf(t, sizeof t, "%p+%zu", pool, b->matPoolBytes); return std::string(t); };
    const size_t bytes = b->matPoolBytes;
    void *best = b->dMat;
    float bestMs = time_fill();
    rec.fillMs.assign(1, bestMs);
    rec.kept = 0;
    rec.kinds.assign(1, kind_of(best));
    rec.ranges.assign(1, range_of(best));
    /* NO pool is unmapped before the last candidate has been filled: the losers are freed together at the end (memory permitting -- the
     * loop stops when the next candidate would not leave 8 GiB of THIS device's memory free; every rank of a multi-GPU job shops on its
     * own device only).  Five candidates in all, no early stop: a rehearsal that stopped after [3.73, 3.59] -- "both modes seen" -- ran
     * at 2907 GCUPS, the next one found 3.40 with its fourth candidate after [3.82, 3.80, 3.76]. */
    std::vector<void *> losers;
    for (int k = 1; k < 5 && bestMs > 0.f; k++) {
        size_t freeB = 0, totalB = 0;
        if (hipMemGetInfo(&freeB, &totalB) != hipSuccess || freeB < bytes + ((size_t)8 << 30)) { (void)hipGetLastError(); break; }
        void *cand = nullptr;
        if (pool_alloc(&cand, bytes) != hipSuccess) { (void)hipGetLastError(); break; }
        rec.kinds.push_back(kind_of(cand));
        rec.ranges.push_back(range_of(cand));
        if (trace.on) { fprintf(stderr, "[dpx] pool candidate %d: %s %s\n", k, rec.kinds.back().c_str(), rec.ranges.back().c_str()); fflush(stderr); }
        set_pool(cand);
        const float ms = time_fill();
        rec.fillMs.push_back(ms);
        rec.candidatesMs.push_back(time_memset(cand, bytes, b->stream));
        if (ms > 0.f && ms < bestMs) { losers.push_back(best); best = cand; bestMs = ms; rec.kept = k; rec.mode = pool_chunk_bytes(cand) ? "vmm" : "malloc"; rec.chunkBytes = pool_chunk_bytes(cand); }
        else losers.push_back(cand);
    }
    set_pool(best);
    (void)hipStreamSynchronize(b->stream);
    for (void *p : losers) pool_free(p);
    if (trace.on) for (size_t k = 0; k < rec.fillMs.size(); k++) fprintf(stderr, "[dpx] pool candidate %zu (%s): fill %.3f ms%s\n", k, rec.kinds[k].c_str(), rec.fillMs[k], (int)k == rec.kept ? "  <- kept" : "");
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
}

static int check_guard(dpx_batch *b);

int dpx_batch_destroy(dpx_batch *b) {
    if (!b) return DPX_OK;
    PhaseTrace trace;
    if (b->device >= 0) { (void)hipSetDevice(b->device); t_device = b->device; }
    /* buffers are parked for the next batch, not freed: nothing of this batch may still be running on them */
    if (b->lastStream && b->lastStream != b->stream) (void)hipStreamSynchronize(b->lastStream);
    if (b->stream) { (void)hipStreamSynchronize(b->stream); stream_park(b->stream); }
    if (b->sideStream) { (void)hipStreamSynchronize(b->sideStream); stream_park(b->sideStream); }
    if (b->guardBytes && !b->guardSelfTest && check_guard(b) != DPX_OK) { fprintf(stderr, "[dpx] %s\n", t_err.c_str()); abort(); }
    if (b->evT0) (void)hipEventDestroy(b->evT0);
    if (b->evT1) (void)hipEventDestroy(b->evT1);
    if (b->evFork) (void)hipEventDestroy(b->evFork);
    if (b->evJoin) (void)hipEventDestroy(b->evJoin);
    if (b->evOrder) (void)hipEventDestroy(b->evOrder);
    if (b->evOut0) (void)hipEventDestroy(b->evOut0);
    if (b->evOut1) (void)hipEventDestroy(b->evOut1);
    g_arenaCache.park(b->arena, b->arenaCap);
    g_matCache.park(b->dMat, b->matPoolBytes);
    g_tbDevCache.park(b->dTb, b->dTbCap);
    g_tbDevCache.park(b->dOut, b->dOutCap);
    g_tbHostCache.park(b->hMeta, b->hMetaCap);
    g_tbHostCache.park(b->hOut, b->hOutCap);
    g_tbDevCache.park(b->dCigar, b->dCigarCap);
    g_tbDevCache.park(b->dCigarOps, b->dCigarOpsCap);
    g_tbHostCache.park(b->hCigar, b->hCigarCap);
    g_tbHostCache.park(b->hCigarOps, b->hCigarOpsCap);
    for (int k = 0; k < 2; k++) {
        g_tbDevCache.park(b->dDiffOff[k], b->dDiffOffCap[k]);
        g_tbDevCache.park(b->dDiffText[k], b->dDiffTextCap[k]);
        g_tbHostCache.park(b->hDiffOff[k], b->hDiffOffCap[k]);
        g_tbHostCache.park(b->hDiffText[k], b->hDiffTextCap[k]);
    }
    g_tbDevCache.park(b->dExt, b->dExtCap);
    g_tbDevCache.park(b->dSubst, b->dSubstCap);
    g_arenaCache.park(b->dRev, b->dRevCap);
    g_stageCache.park(b->hStage, b->hStageCap);
    delete b;
    trace.mark("destroy");
    return DPX_OK;
}

int dpx_batch_create(const dpx_params *params, const char *sequences, size_t numBytes, const dpx_seq_pair *pairs,
                     size_t firstPair, size_t numPairs, unsigned flags, dpx_batch **out) {
    return dpx_batch_create_on(-1, params, sequences, numBytes, pairs, firstPair, numPairs, flags, out);
}

/* `alphabet` == nullptr: `sequences` are numBytes plain bytes.  Otherwise `sequences` holds numBytes BASES, four per byte (base k in
 * bits 2*(k%4) of byte k/4), alphabet[code] is the byte a code stands for, and the pairs' indices count bases. */
static int create_impl(int device, const dpx_params *params, const char *sequences, size_t numBytes, const uint8_t *alphabet,
                       const dpx_seq_pair *pairs, size_t firstPair, size_t numPairs, unsigned flags, dpx_batch **out);

int dpx_batch_create_on(int device, const dpx_params *params, const char *sequences, size_t numBytes, const dpx_seq_pair *pairs,
                        size_t firstPair, size_t numPairs, unsigned flags, dpx_batch **out) {
    return create_impl(device, params, sequences, numBytes, nullptr, pairs, firstPair, numPairs, flags, out);
}

int dpx_batch_create_packed2(int device, const dpx_params *params, const uint8_t *packed, size_t numBases, const uint8_t alphabet[4],
                             const dpx_seq_pair *pairs, size_t firstPair, size_t numPairs, unsigned flags, dpx_batch **out) {
    if (!alphabet) return DPX_ERR_INVALID;
    return create_impl(device, params, reinterpret_cast<const char *>(packed), numBases, alphabet, pairs, firstPair, numPairs, flags, out);
}

/* Host side of the 2-bit input: the distinct byte values inside the pairs' ranges become the alphabet (in order of first appearance;
 * more than four: DPX_ERR_UNSUPPORTED, the caller keeps its bytes), every byte of `sequences` its 2-bit code (bytes outside
 * every pair -- parseInput's separators -- and bytes of other values: code 0, never read).  packed: (numBytes + 3) / 4 bytes. */
int dpx_pack2(const char *sequences, size_t numBytes, const dpx_seq_pair *pairs, size_t numPairs, uint8_t alphabet[4], uint8_t *packed) {
    if ((numBytes && !sequences) || (numPairs && !pairs) || !alphabet || (numBytes && !packed)) return DPX_ERR_INVALID;
    int code[256];
    for (int &c : code) c = -1;
    int used = 0;
    const unsigned char *sq = reinterpret_cast<const unsigned char *>(sequences);
    for (size_t i = 0; i < numPairs; i++) {
        const dpx_seq_pair &sp = pairs[i];
        if (sp.referenceSize < 0 || sp.querySize < 0 || sp.referenceIdx < 0 || sp.queryIdx < 0 ||
            (size_t)sp.referenceIdx + (size_t)sp.referenceSize > numBytes || (size_t)sp.queryIdx + (size_t)sp.querySize > numBytes)
            return DPX_ERR_INVALID;
        for (int side = 0; side < 2; side++) {
            const unsigned char *p = sq + (side ? sp.queryIdx : sp.referenceIdx);
            const size_t len = (size_t)(side ? sp.querySize : sp.referenceSize);
            for (size_t k = 0; k < len; k++) {
                if (code[p[k]] >= 0) continue;
                if (used == 4) return DPX_ERR_UNSUPPORTED;
                alphabet[used] = p[k];
                code[p[k]] = used++;
            }
        }
    }
    for (int k = used; k < 4; k++) alphabet[k] = used ? alphabet[0] : (uint8_t)'0';
    uint8_t lut[256];
    for (int v = 0; v < 256; v++) lut[v] = (uint8_t)(code[v] < 0 ? 0 : code[v]);
    const size_t whole = numBytes / 4;
    for (size_t q = 0; q < whole; q++)
        packed[q] = (uint8_t)(lut[sq[4 * q]] | (lut[sq[4 * q + 1]] << 2) | (lut[sq[4 * q + 2]] << 4) | (lut[sq[4 * q + 3]] << 6));
    if (numBytes & 3) {
        uint8_t v = 0;
        for (size_t k = 4 * whole; k < numBytes; k++) v = (uint8_t)(v | (lut[sq[k]] << (2 * (k & 3))));
        packed[whole] = v;
    }
    return DPX_OK;
}

static int create_impl(int device, const dpx_params *params, const char *sequences, size_t numBytes, const uint8_t *alphabet,
                       const dpx_seq_pair *pairs, size_t firstPair, size_t numPairs, unsigned flags, dpx_batch **out) {
    if (!out) return DPX_ERR_INVALID;
    *out = nullptr;
    int rc = validate_params(params);
    if (rc != DPX_OK) return rc;
    if ((numPairs && (!pairs || !sequences)) || numPairs > 0x7fffffffu) return DPX_ERR_INVALID;
    if (device >= 0) { /* an explicit device: must exist (-1 = the default device of dpx_init) */
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { (void)hipGetLastError(); return DPX_ERR_NO_DEVICE; }
        if (device >= n) return DPX_ERR_INVALID;
    } else if (device != -1) return DPX_ERR_INVALID;
    const bool dirFlag = (flags & DPX_KEEP_DIRECTIONS) != 0, bandDirFlag = (flags & DPX_KEEP_BAND_DIRECTIONS) != 0;
    const bool localFlag = (flags & DPX_KEEP_LOCAL_BAND_DIRECTIONS) != 0; /* (its algorithm rule is the planner's) */
    if ((dirFlag || bandDirFlag || localFlag) && (flags & DPX_SCORE_ONLY)) return DPX_ERR_INVALID;
    if (localFlag && (flags & (DPX_KEEP_BAND_DIRECTIONS | DPX_TWO_PIECE_GAPS))) return DPX_ERR_INVALID;
    if (dirFlag && is_banded(params->algo)) return DPX_ERR_UNSUPPORTED; /* 0x8 on a banded algorithm stays refused, with or without 0x10 */
    if ((flags & DPX_TWO_PIECE_GAPS) && !bandDirFlag) return DPX_ERR_INVALID; /* the second gap piece exists on band-direction batches only */
    if (bandDirFlag && params->algo != DPX_ALGO_BANW && params->algo != DPX_ALGO_BAXT) return DPX_ERR_UNSUPPORTED; /* (BSW / BASW: DPX_KEEP_LOCAL_BAND_DIRECTIONS is their flag) */
    rc = bind_device(device);
    if (rc != DPX_OK) return rc;

    refresh_knobs();
    const Knobs kn = knobs();
    PhaseTrace trace;
    dpx_batch *b = new (std::nothrow) dpx_batch();
    if (!b) return DPX_ERR_NOMEM;
    rc = dpx_plan_batch(*params, pairs, firstPair, numPairs, numBytes, alphabet != nullptr, flags, kn, *b, t_err); /* (the batch IS the plan) */
    if (rc != DPX_OK) { delete b; return rc; }
    b->device = t_device;
    trace.mark("create: validate+geometry+launch lists"); /* (the planner marks no phases of its own) */

#define CREATE_TRY(call)                                                      \
    do {                                                                      \
        hipError_t e__ = (call);                                              \
        if (e__ != hipSuccess) { int r__ = hip_fail(e__, #call); dpx_batch_destroy(b); return r__; } \
    } while (0)

    CREATE_TRY(stream_take(&b->stream));
    trace.mark("create: stream");
    sequences += alphabet ? b->seqLo / 4 : b->seqLo; /* the uploaded window of the caller's buffer (dpx_plan.h: seqLo, seqHi) */
    numBytes = b->seqHi - b->seqLo;
    char *dPacked = nullptr;
    size_t stageBytes = 0;
    {
        const size_t np1 = std::max<size_t>(numPairs, 1);
        const size_t szSeq = align_up(std::max<size_t>(std::max(numBytes, b->packedDwords * 16), 16), 256), szPairs = align_up(np1 * sizeof(dpx_pair_dev), 256);
        const size_t szPacked = alphabet ? align_up(std::max<size_t>(b->packedDwords * 4, 16), 256) : 0;
        const size_t szI32 = align_up(np1 * sizeof(int32_t), 256), szOff = align_up((np1 + 1) * sizeof(uint64_t), 256);
        const size_t szCouples = std::max(szI32, align_up(b->waves.size() * sizeof(dpx_wave_desc), 256)); /* couples, or the wave descriptors */
        const size_t szScan = align_up((dpx_out_scan_tiles(np1) + 1) * sizeof(uint64_t), 256);
        const size_t need = szSeq + szPairs + 5 * szI32 + szCouples + 2 * szOff + szScan + szPacked; /* score, endRow, endCol, order, couples, tbLen; tbOff, outOff, scan; 2-bit staging */
        CREATE_TRY(g_arenaCache.take((void **)&b->arena, need, &b->arenaCap));
        char *q = b->arena;
        b->dSeq = q;                  q += szSeq;
        b->dSeqOwn = b->dSeq; b->seqBytes = szSeq;
        b->dPairs = (dpx_pair_dev *)q; q += szPairs;
        b->dScore = (int32_t *)q;     q += szI32;
        b->dEndRow = (int32_t *)q;    q += szI32;
        b->dEndCol = (int32_t *)q;    q += szI32;
        if (!b->singles.empty()) b->dOrder = (int32_t *)q;
        q += szI32;
        if (b->packed || b->lanePacked) b->dCouples = (int32_t *)q;
        q += szCouples;
        b->dTbLen = (int32_t *)q;     q += szI32;
        b->dTbOff = (uint64_t *)q;    q += szOff;
        b->dOutOff = (uint64_t *)q;   q += szOff;
        b->dOutScratch = (uint64_t *)q; q += szScan;
        dPacked = alphabet ? q : nullptr;
        /* Small batches (the class-per-pair drivers send 20 pairs per round trip, most tests a handful): everything the host uploads --
         * sequences, pair table, launch lists, line offsets -- lies in the arena's front, so it is assembled in ONE pinned image and sent
         * with ONE asynchronous copy on the batch's stream instead of five synchronous ones (~15 us each whatever the size: 70 -> 25 us
         * per create).  The fill is ordered behind it by the stream (a fill on a caller's stream waits for it, dpx_batch_fill). */
        const size_t front = (size_t)((char *)b->dTbOff - b->arena) + szOff;
        if (!alphabet && front <= ((size_t)256 << 10)) {
            CREATE_TRY(g_stageCache.take((void **)&b->hStage, align_up(front, (size_t)64 << 10), &b->hStageCap));
            stageBytes = front;
        }
    }
    /* host -> arena: into the image when there is one */
    auto upload = [&](void *dst, const void *src, size_t bytes) -> hipError_t {
        if (!b->hStage) return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
        memcpy(b->hStage + ((char *)dst - b->arena), src, bytes);
        return hipSuccess;
    };
    trace.mark("create: arena");
    if (alphabet) { /* a quarter of the bytes over PCIe, expanded by k_unpack2 into the byte buffer the kernels read */
        if (b->packedCopy) CREATE_TRY(hipMemcpy(dPacked, sequences, b->packedCopy, hipMemcpyHostToDevice));
        const uint32_t alpha = (uint32_t)alphabet[0] | ((uint32_t)alphabet[1] << 8) | ((uint32_t)alphabet[2] << 16) | ((uint32_t)alphabet[3] << 24);
        CREATE_TRY(dpx_launch_unpack2(reinterpret_cast<const uint32_t *>(dPacked), alpha, b->dSeq, b->packedDwords, b->stream));
        CREATE_TRY(hipStreamSynchronize(b->stream)); /* (a fill may run on a caller's stream) */
    } else if (numBytes) CREATE_TRY(upload(b->dSeq, sequences, numBytes));
    trace.mark("create: H2D sequences");
    if (b->lanePacked) CREATE_TRY(upload(b->dCouples, b->waves.data(), b->waves.size() * sizeof(dpx_wave_desc)));
    else if (b->packed) CREATE_TRY(upload(b->dCouples, b->couples.data(), b->couples.size() * sizeof(int32_t)));
    if (b->dOrder) CREATE_TRY(upload(b->dOrder, b->singles.data(), b->singles.size() * sizeof(int32_t)));
    trace.mark("create: H2D launch lists"); /* (placement is the planner's) */
    if (numPairs) CREATE_TRY(upload(b->dPairs, b->pairs.data(), numPairs * sizeof(dpx_pair_dev)));
    if (b->store) CREATE_TRY(upload(b->dTbOff, b->tbOff.data(), (numPairs + 1) * sizeof(uint64_t)));
    if (b->hStage) { /* the one copy; the image stays untouched until dpx_batch_destroy() has waited for the stream */
        CREATE_TRY(hipMemcpyAsync(b->arena, b->hStage, stageBytes, hipMemcpyHostToDevice, b->stream));
        b->uploadPending = true;
    }
    /* (the device, or the image, has the launch lists now; the pair table and the line offsets stay: the output path reads them) */
    b->singles = std::vector<int32_t>(); b->couples = std::vector<int32_t>(); b->waves = std::vector<dpx_wave_desc>();
    /* (a batch whose pairs are all empty has no cells, but k_traceback_wave loads the pool's first 16 bytes in place of every cell without
     * storage and masks them afterwards: such a batch gets a pool of 256 bytes, so that a.mat is an address the device may read) */
    if (b->store && (b->matElems || b->dirScratch || numPairs)) {
        void *pool = nullptr;
        bool fresh = false;
        /* DPX_POOL_GUARD=1 (tests): 4 MiB behind the matrices are filled with a pattern here and checked by dpx_batch_sync() -- a kernel that
         * writes past the end of the batch's matrices fails the test instead of hitting whatever is mapped behind the pool */
        const bool guardOn = kn.poolGuard != 0;
        b->guardBytes = guardOn ? (size_t)4 << 20 : 0;
        const size_t guardAt = b->matElems * sizeof(int16_t) + b->dirScratch;
        CREATE_TRY(g_matCache.take(&pool, std::max<size_t>(guardAt + b->guardBytes, 256), &b->matPoolBytes, &fresh));
        if (b->guardBytes) CREATE_TRY(hipMemset((char *)pool + guardAt, 0xA5, b->guardBytes));
        if (b->guardBytes && kn.poolGuard == 2) { /* (the checker's own test: one byte of the band is already wrong) */
            CREATE_TRY(hipMemset((char *)pool + guardAt + 12345, 0, 1));
            b->guardSelfTest = true;
        }
        /* DPX_TUNE_PLACEMENT (callers that fill the batch many times): the pool is timed with hipMemset and, if it is a fresh one,
         * shopped for with the batch's own fill at the end of this function (shop_pool_by_fill: four more allocations of the
         * pool's size).  DPX_POOL_PROBE=0 / 1 / 2 forces nothing / timing only / timing + shopping, whatever the flag says */
        bool tune = (flags & DPX_TUNE_PLACEMENT) != 0;
        int probeEnv = -1;
        if (kn.poolProbe >= 0) { probeEnv = kn.poolProbe; tune = probeEnv != 0; }
        PoolRecord rec;
        bool known = false;
        if (!fresh) {
            std::lock_guard<std::mutex> lk(g_poolRecMu);
            auto it = g_poolRecords.find(pool);
            if (it != g_poolRecords.end()) { rec = it->second; known = true; }
        }
        if (!known) rec = fresh_pool_record(pool, b->matPoolBytes);
        b->tunePool = tune && rec.candidatesMs.empty() && b->matPoolBytes >= ((size_t)1 << 30) && !b->guardBytes; /* (the memset probe would wipe the band) */
        /* (shopping for a pool nobody has shopped for yet: a fresh one, or one that dpx_pool_reserve built ahead of time) */
        b->tuneShop = b->tunePool && (fresh || rec.fillMs.empty()) && probeEnv != 1; /* DPX_POOL_PROBE=1: time only, no shopping */
        if (b->tunePool) rec.candidatesMs.assign(1, time_memset(pool, b->matPoolBytes, b->stream));
        b->dMat = (int16_t *)pool;
        b->poolRec = rec;
        { std::lock_guard<std::mutex> lk(g_poolRecMu); g_poolRecords[pool] = rec; }
    }
    trace.mark("create: H2D pairs+matrix pool");
#undef CREATE_TRY

    /* the plan's launch arguments get their device pointers */
    for (dpx_fill_args *x : {&b->args, &b->pkArgs}) {
        if (x == &b->pkArgs && !b->packed && !b->lanePacked) break; /* (stays zero) */
        x->seq = b->dSeq; x->pairs = b->dPairs; x->mat = b->dMat;
        x->score = b->dScore; x->endRow = b->dEndRow; x->endCol = b->dEndCol;
    }
    b->args.order = b->dOrder;
    if (b->packed) b->pkArgs.order = b->dCouples;
    if (b->lanePacked) b->pkArgs.waves = reinterpret_cast<const dpx_wave_desc *>(b->dCouples);
    if (b->dirs) {
        dpx_dir_args &d = b->dirArgs;
        d.seq = b->dSeq; d.pairs = b->dPairs; d.order = b->dOrder;
        d.codes = reinterpret_cast<uint8_t *>(b->dMat);
        d.score = b->dScore; d.endRow = b->dEndRow; d.endCol = b->dEndCol;
        d.scratch = b->dirScratch ? reinterpret_cast<unsigned char *>(b->dMat) + b->matElems * sizeof(int16_t) : nullptr;
    }
    if ((b->packed || b->lanePacked) && b->nSingles > 0) {
        /* more than one kernel per fill: a side stream + fork/join events (failure here only costs the overlap) */
        if (stream_take(&b->sideStream) != hipSuccess) { b->sideStream = nullptr; (void)hipGetLastError(); }
        if (b->sideStream && (hipEventCreateWithFlags(&b->evFork, hipEventDisableTiming) != hipSuccess ||
                              hipEventCreateWithFlags(&b->evJoin, hipEventDisableTiming) != hipSuccess)) (void)hipGetLastError();
    }
    if (b->tuneShop && b->dMat && !b->guardBytes) {
        shop_pool_by_fill(b, b->poolRec, trace);
        std::lock_guard<std::mutex> lk(g_poolRecMu);
        g_poolRecords[b->dMat] = b->poolRec;
        trace.mark("create: pool shopped by fill");
    }
    *out = b;
    return DPX_OK;
}

/* One fill = up to two kernels over disjoint pairs (couples or lane-packed waves + leftover singles).  They do not depend
 * on each other, but launches on one stream run one after the other -- and a small one (a few hundred leftover waves on
 * 1024 SIMDs) then costs a latency-bound tail of its own.
 * The secondary kernels therefore go to the batch's side stream between a fork and a join event; on `s` the fill still
 * looks like one operation (events recorded on `s` around it time all of it). */
static bool extension_on(const dpx_batch *b) { return b->zdrop >= 0 || b->endBonus >= 0; }

/* which kernels the batch runs under its present settings (dpx_plan.h: computed at every use, never kept) */
static dpx_route route_of(const dpx_batch *b) { return dpx_plan_route(*b, knobs().tbWalk, b->zdrop, b->endBonus, b->substAlphabet); }

/* what a refill does to lines, text and CIGARs; the results go with them until the next fill */
static void invalidate_fill(dpx_batch *b) {
    b->filled = false; b->extFilled = false; b->tbLinesValid = false; b->outState = 0; b->cigarState = 0; b->diffState[0] = b->diffState[1] = 0;
}
/* ... and that next fill, queued on `s` along route `r` */
static void mark_filled(dpx_batch *b, const dpx_route &r, hipStream_t s) {
    invalidate_fill(b);
    b->filled = true; b->extFilled = r.extRecords; b->lastStream = s;
}

/* the batch's table on the device (dpx_kernels.h: the map behind the table, one allocation) */
static dpx_table_ref table_ref(const dpx_batch *b) { return {reinterpret_cast<const int8_t *>(b->dSubst), b->dSubst + DPX_SUBST_TABLE_BYTES}; }

/* the batch's launch arguments under its substitution table: every wave's LDS slice grows by the table image */
static dpx_subst_args subst_args(const dpx_batch *b) {
    dpx_subst_args sa = {b->args, table_ref(b)};
    sa.f.ldsPerWave += DPX_SUBST_IMAGE_BYTES;
    return sa;
}
static size_t subst_lds_bytes(const dpx_batch *b) { return b->ldsBytes + (size_t)DPX_SUBST_IMAGE_BYTES * (DPX_FILL_THREADS / 64); }

static hipError_t launch_main(dpx_batch *b, const dpx_route &r, hipStream_t s) { /* the one-wave-per-pair kernel of the batch's algorithm */
    switch (r.main) {
    case DPX_MAIN_NONE: return hipSuccess;
    case DPX_MAIN_FILL:
        if (r.scoreTable) { /* (dpx_batch_set_score_table: every wave's LDS slice grows by the image; the workgroup may shrink to one wave) */
            dpx_subst_args ta = {b->args, table_ref(b)};
            ta.f.ldsPerWave = (uint32_t)dpx_plan_scoretab_lds(*b); ta.f.wavesPerBlock = dpx_plan_scoretab_waves(*b);
            return dpx_launch_scoretab_fill(ta, b->kernelAlgo, b->R, s);
        }
        return dpx_launch_fill(b->args, b->kernelAlgo, b->R, b->store, b->ldsBytes, s);
    case DPX_MAIN_BASW: return dpx_launch_basw_fill(b->args, b->R, b->store, b->ldsBytes, s);
    case DPX_MAIN_BANW: return dpx_launch_banw_fill(b->args, b->R, b->store, b->ldsBytes, s);
    case DPX_MAIN_BAXT: return dpx_launch_baxt_fill(b->args, b->R, b->store, b->ldsBytes, s);
    case DPX_MAIN_ZEXT: {
        const dpx_zext_args za = {b->args, {b->zdrop, b->endBonus, b->dExt}};
        return dpx_launch_zext_fill(za, b->R, b->store, b->ldsBytes, s);
    }
    case DPX_MAIN_SUBST: return dpx_launch_subst_fill(subst_args(b), b->R, b->store, r.ext, subst_lds_bytes(b), s);
    case DPX_MAIN_ZSUB: {
        const dpx_zsub_args za = {subst_args(b), {b->zdrop, b->endBonus, b->dExt}};
        return dpx_launch_zsub_fill(za, b->R, b->store, subst_lds_bytes(b), s);
    }
    case DPX_MAIN_BDIR: return dpx_launch_bdir_fill(b->args, b->R, r.ext, s);
    case DPX_MAIN_BDL: return dpx_launch_bdl_fill(b->args, b->R, b->prm.algo == DPX_ALGO_BASW, s);
    case DPX_MAIN_BDX: { /* (dpx_batch_set_direction_scoring: with a table every wave's LDS slice grows by the image, and the workgroup may shrink to one wave) */
        dpx_bdx_args xa = {b->args, {nullptr, nullptr}, {r.ext ? b->zdrop : -1, r.ext ? b->endBonus : -1, b->dExt}};
        if (b->substAlphabet) {
            xa.tab = table_ref(b);
            xa.f.ldsPerWave += DPX_SUBST_IMAGE_BYTES; xa.f.wavesPerBlock = dpx_plan_bdx_waves(*b, true);
        }
        return dpx_launch_bdx_fill(xa, b->R, r.ext, s);
    }
    case DPX_MAIN_BD2: { /* (a two-piece batch: every mode, "nothing on" included, is k_bd2_fill's; the table's LDS as for k_bdx_fill) */
        dpx_bd2_args xa = {b->args, {nullptr, nullptr}, {r.ext ? b->zdrop : -1, r.ext ? b->endBonus : -1, b->dExt}, b->gapOpen2, b->gapExtend2};
        if (b->substAlphabet) {
            xa.tab = table_ref(b);
            xa.f.ldsPerWave += DPX_SUBST_IMAGE_BYTES; xa.f.wavesPerBlock = dpx_plan_bdx_waves(*b, true);
        }
        return dpx_launch_bd2_fill(xa, b->R, r.ext, s);
    }
    }
    return hipErrorInvalidValue;
}

static hipError_t launch_all(dpx_batch *b, const dpx_route &r, hipStream_t s) {
    if (r.dirTable) { /* (dpx_batch_set_direction_table: edge rows in LDS, every wave's slice grows by the image; the workgroup may shrink to one wave) */
        dpx_dirtab_args ta = {b->dirArgs, table_ref(b)};
        if (!ta.d.scratch) ta.d.ldsPerWave += DPX_SUBST_IMAGE_BYTES;
        ta.d.wavesPerBlock = dpx_plan_dirtab_waves(*b);
        return dpx_launch_dirtab_fill(ta, b->kernelAlgo, b->R, s);
    }
    if (r.dirs) return dpx_launch_fill_dir(b->dirArgs, b->kernelAlgo, b->R, s);
    if (r.split) return dpx_launch_fill_split(b->args, b->kernelAlgo, b->R, b->splitWaves, b->splitLds, s);
    hipStream_t side = s;
    bool forked = false;
    if (r.second != DPX_SECOND_NONE && r.main != DPX_MAIN_NONE && b->sideStream && b->evFork && b->evJoin) {
        hipError_t e = hipEventRecord(b->evFork, s);
        if (e == hipSuccess) e = hipStreamWaitEvent(b->sideStream, b->evFork, 0);
        if (e != hipSuccess) return e;
        side = b->sideStream;
        forked = true;
    }
    /* the leftover pairs first (theirs is the short kernel; the packed or lane-packed one then fills the chip around it) */
    hipError_t e = launch_main(b, r, side); /* (beside the lane-packed kernels: the empty pairs) */
    switch (e == hipSuccess ? r.second : DPX_SECOND_NONE) {
    case DPX_SECOND_NONE: break;
    case DPX_SECOND_PACKED: e = dpx_launch_fill_packed(b->pkArgs, b->kernelAlgo, b->R, b->pkLdsBytes, s); break;
    case DPX_SECOND_BANDED_PACKED: e = dpx_launch_banded_packed(b->pkArgs, b->R, b->pkLdsBytes, s); break;
    case DPX_SECOND_LANES:
        if (r.scoreTable) { /* (the image behind the wave's reference area) */
            dpx_subst_args ta = {b->pkArgs, table_ref(b)};
            ta.f.ldsPerWave = (uint32_t)dpx_plan_scoretab_lanes_lds(*b);
            e = dpx_launch_scoretab_lanes(ta, b->kernelAlgo, b->R, s);
            break;
        }
        e = dpx_launch_fill_lanes(b->pkArgs, b->kernelAlgo, b->R, b->store, b->pkLdsBytes, s);
        break;
    case DPX_SECOND_LANES_PK: e = dpx_launch_fill_lanes_packed(b->pkArgs, b->kernelAlgo, b->pkLdsBytes, s); break;
    }
    if (forked) {
        hipError_t j = hipEventRecord(b->evJoin, side);
        if (j == hipSuccess) j = hipStreamWaitEvent(s, b->evJoin, 0);
        if (e == hipSuccess) e = j;
    }
    return e;
}

int dpx_batch_fill(dpx_batch *b, void *stream) {
    if (!b) return DPX_ERR_INVALID;
    int rc = bind_device(b->device);
    if (rc != DPX_OK) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : b->stream;
    if (b->uploadPending) { /* the batch's inputs travel on b->stream (dpx_batch_create, small batches): a caller's stream waits for them once */
        if (s != b->stream) HIP_TRY(hipStreamSynchronize(b->stream));
        b->uploadPending = false;
    }
    const bool timed = (b->flags & DPX_TIME_FILLS) != 0;
    if (timed) {
        if (!b->evT0) HIP_TRY(hipEventCreate(&b->evT0));
        if (!b->evT1) HIP_TRY(hipEventCreate(&b->evT1));
        HIP_TRY(hipEventRecord(b->evT0, s));
    }
    const dpx_route r = route_of(b);
    HIP_TRY(launch_all(b, r, s));
    if (timed) { HIP_TRY(hipEventRecord(b->evT1, s)); b->fillTimed = true; }
    mark_filled(b, r, s);
    return DPX_OK;
}

int dpx_batch_last_fill_usec(dpx_batch *b, double *usec) {
    if (!b || !usec) return DPX_ERR_INVALID;
    if (!b->fillTimed) return DPX_ERR_NOT_FILLED; /* no fill yet, or the batch was created without DPX_TIME_FILLS */
    int rc = bind_device(b->device);
    if (rc != DPX_OK) return rc;
    HIP_TRY(hipEventSynchronize(b->evT1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, b->evT0, b->evT1));
    *usec = (double)ms * 1000.0;
    return DPX_OK;
}

int dpx_batch_last_output_usec(dpx_batch *b, double *usec) {
    if (!b || !usec) return DPX_ERR_INVALID;
    if (!b->outTimed) return DPX_ERR_NOT_FILLED; /* no dpx_batch_output_begin() yet, or the batch was created without DPX_TIME_FILLS */
    int rc = bind_device(b->device);
    if (rc != DPX_OK) return rc;
    HIP_TRY(hipEventSynchronize(b->evOut1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, b->evOut0, b->evOut1));
    *usec = (double)ms * 1000.0;
    return DPX_OK;
}

int dpx_batch_fill_timed(dpx_batch *b, int repeats, double *usecPerFill) {
    if (!b || repeats < 1 || !usecPerFill) return DPX_ERR_INVALID;
    int rc = bind_device(b->device);
    if (rc != DPX_OK) return rc;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    float ms = 0.f;
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess) e = hipEventRecord(e0, b->stream);
    const dpx_route r = route_of(b);
    for (int i = 0; i < repeats && e == hipSuccess; i++) e = launch_all(b, r, b->stream);
    if (e == hipSuccess) e = hipEventRecord(e1, b->stream);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    if (e0) (void)hipEventDestroy(e0); /* on every path */
    if (e1) (void)hipEventDestroy(e1);
    if (e != hipSuccess) return hip_fail(e, "dpx_batch_fill_timed");
    *usecPerFill = (double)ms * 1000.0 / repeats;
    mark_filled(b, r, b->stream);
    return DPX_OK;
}

/* DPX_POOL_GUARD: nothing may have written behind the matrices (checked by dpx_batch_sync, dpx_batch_results and -- fatally, so that a
 * whole test run under the knob cannot miss it -- by dpx_batch_destroy) */
static int check_guard(dpx_batch *b) {
    if (!b->guardBytes || !b->dMat) return DPX_OK;
    std::vector<unsigned char> h(b->guardBytes);
    HIP_TRY(hipMemcpy(h.data(), (const char *)b->dMat + b->matElems * sizeof(int16_t) + b->dirScratch, b->guardBytes, hipMemcpyDeviceToHost));
    for (size_t k = 0; k < h.size(); k++)
        if (h[k] != 0xA5) { t_err = "DPX_POOL_GUARD: byte " + std::to_string(k) + " behind the matrices was overwritten"; return DPX_ERR_HIP; }
    return DPX_OK;
}

int dpx_batch_sync(dpx_batch *b) {
    if (!b) return DPX_ERR_INVALID;
    int rc = bind_device(b->device);
    if (rc != DPX_OK) return rc;
    if (b->lastStream && b->lastStream != b->stream) HIP_TRY(hipStreamSynchronize(b->lastStream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return check_guard(b);
}

int dpx_batch_device_results(dpx_batch *b, void **dScores, void **dEndRow, void **dEndCol) {
    if (!b) return DPX_ERR_INVALID;
    if (dScores) *dScores = b->dScore;
    if (dEndRow) *dEndRow = b->dEndRow;
    if (dEndCol) *dEndCol = b->dEndCol;
    return DPX_OK;
}

int dpx_batch_results(dpx_batch *b, int32_t *scores, int32_t *endRow, int32_t *endCol) {
    if (!b) return DPX_ERR_INVALID;
    if (!b->filled) return DPX_ERR_NOT_FILLED;
    int rc = bind_device(b->device);
    if (rc != DPX_OK) return rc;
    if (b->lastStream && b->lastStream != b->stream) HIP_TRY(hipStreamSynchronize(b->lastStream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    const size_t bytes = b->numPairs * sizeof(int32_t);
    const size_t stride = (size_t)((const char *)b->dEndRow - (const char *)b->dScore); /* the three arrays follow each other in the arena */
    if (bytes && b->resultsCopied && b->outState != 0 && b->hMeta) { /* dpx_batch_output_begin() brought them along (small batches) */
        const char *tail = b->hMeta + (b->numPairs + 1) * sizeof(uint64_t) + b->numPairs * sizeof(int32_t) + 16;
        if (scores) memcpy(scores, tail, bytes);
        if (endRow) memcpy(endRow, tail + stride, bytes);
        if (endCol) memcpy(endCol, tail + 2 * stride, bytes);
        return check_guard(b);
    }
    if (bytes && scores && endRow && endCol && (const char *)b->dEndCol - (const char *)b->dEndRow == (ptrdiff_t)stride && 3 * stride <= 12288) {
        /* small batches (the class-per-pair drivers: 20 pairs per round trip): one copy instead of three -- a synchronous copy costs
         * ~15 us whatever its size */
        char tmp[12288];
        HIP_TRY(hipMemcpy(tmp, b->dScore, 2 * stride + bytes, hipMemcpyDeviceToHost));
        memcpy(scores, tmp, bytes);
        memcpy(endRow, tmp + stride, bytes);
        memcpy(endCol, tmp + 2 * stride, bytes);
    } else if (bytes) {
        if (scores) HIP_TRY(hipMemcpy(scores, b->dScore, bytes, hipMemcpyDeviceToHost));
        if (endRow) HIP_TRY(hipMemcpy(endRow, b->dEndRow, bytes, hipMemcpyDeviceToHost));
        if (endCol) HIP_TRY(hipMemcpy(endCol, b->dEndCol, bytes, hipMemcpyDeviceToHost));
    }
    return check_guard(b);
}

int dpx_batch_directions(dpx_batch *b, size_t pair, int which, uint8_t *out) {
    if (!b || !out || pair >= b->numPairs || which < 0 || which >= (b->twoPiece ? DPX_MAT_H_PIECE + 1 : b->planes)) return DPX_ERR_INVALID;
    if (!b->dirs && !b->bandDirs) return DPX_ERR_NO_MATRIX;
    if (!b->filled) return DPX_ERR_NOT_FILLED;
    int rc = bind_device(b->device);
    if (rc != DPX_OK) return rc;
    const dpx_pair_dev &pd = b->pairs[pair];
    const size_t total = (size_t)(pd.m + 1) * (size_t)(pd.n + 1);
    uint8_t *dOut = nullptr;
    size_t dOutCap = 0;
    if (b->lastStream && b->lastStream != b->stream) HIP_TRY(hipStreamSynchronize(b->lastStream));
    HIP_TRY(g_tbDevCache.take((void **)&dOut, std::max<size_t>(total, 16), &dOutCap)); /* row-major scratch */
    hipError_t e = b->twoPiece ? dpx_launch_bd2_export(reinterpret_cast<const uint8_t *>(b->dMat), pd, b->dSeq, b->prm.band, which, dOut, b->stream)
                   : b->bandLocal ? dpx_launch_bdl_export(reinterpret_cast<const uint8_t *>(b->dMat), pd, b->dSeq, b->prm.band, which, dOut, b->stream)
                   : b->bandDirs ? dpx_launch_bdir_export(reinterpret_cast<const uint8_t *>(b->dMat), pd, b->dSeq, b->prm.band, which, dOut, b->stream)
                                 : dpx_launch_export_dir(reinterpret_cast<const uint8_t *>(b->dMat), pd, b->dSeq, b->kernelAlgo, b->R, which, dOut, b->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    if (e == hipSuccess) e = hipMemcpy(out, dOut, total, hipMemcpyDeviceToHost);
    g_tbDevCache.park(dOut, dOutCap);
    dpx_extension rec{};
    if (e == hipSuccess && b->bandDirs && b->extFilled) e = hipMemcpy(&rec, b->dExt + pair * (sizeof rec / sizeof(int32_t)), sizeof rec, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "dpx_batch_directions");
    if (b->bandDirs && b->extFilled && rec.lastDiag < pd.m + pd.n) {
        /* a z-dropped pair: k_bdx_fill stopped on anti-diagonal lastDiag, and the codes behind it are whatever the pool held before */
        for (int i = 0; i <= pd.m; i++)
            for (int j = std::max(rec.lastDiag - i + 1, 0); j <= pd.n; j++) out[(size_t)i * (size_t)(pd.n + 1) + (size_t)j] = 0;
    }
    return DPX_OK;
}

int dpx_batch_matrix(dpx_batch *b, size_t pair, int which, int16_t *out) {
    if (!b || !out || pair >= b->numPairs || which < 0 || which >= b->planes) return DPX_ERR_INVALID;
    if (!b->store || b->dirs || b->bandDirs) return DPX_ERR_NO_MATRIX;
    if (!b->filled) return DPX_ERR_NOT_FILLED;
    int rc = bind_device(b->device);
    if (rc != DPX_OK) return rc;
    const dpx_pair_dev &pd = b->pairs[pair];
    const size_t total = (size_t)(pd.m + 1) * (size_t)(pd.n + 1);
    int16_t *dOut = nullptr;
    size_t dOutCap = 0;
    if (b->lastStream && b->lastStream != b->stream) HIP_TRY(hipStreamSynchronize(b->lastStream));
    HIP_TRY(g_tbDevCache.take((void **)&dOut, total * sizeof(int16_t), &dOutCap)); /* row-major scratch */
    hipError_t e = hipErrorInvalidValue;
    switch (route_of(b).exportKind) {
    case DPX_EXPORT_PLAIN: e = dpx_launch_export(b->dMat, pd, b->kernelAlgo, b->R, b->planes, which, b->prm.gapOpen, b->prm.gapExtend, b->prm.band, dOut, b->stream); break;
    case DPX_EXPORT_BASW: e = dpx_launch_basw_export(b->dMat, pd, which, b->prm.band, dOut, b->stream); break;
    case DPX_EXPORT_BANW: e = dpx_launch_banw_export(b->dMat, pd, which, b->prm.band, b->prm.gapOpen, b->prm.gapExtend, dOut, b->stream); break;
    }
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    if (e == hipSuccess) e = hipMemcpy(out, dOut, total * sizeof(int16_t), hipMemcpyDeviceToHost);
    g_tbDevCache.park(dOut, dOutCap);
    dpx_extension rec{};
    if (e == hipSuccess && b->extFilled) e = hipMemcpy(&rec, b->dExt + pair * (sizeof rec / sizeof(int32_t)), sizeof rec, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "dpx_batch_matrix");
    if (b->extFilled && rec.lastDiag < pd.m + pd.n) {
        /* a z-dropped pair: k_zext_fill / k_zsub_fill stopped on anti-diagonal lastDiag, and what the pool holds behind it is whatever was there before */
        for (int i = 0; i <= pd.m; i++)
            for (int j = std::max(rec.lastDiag - i + 1, 0); j <= pd.n; j++) out[(size_t)i * (size_t)(pd.n + 1) + (size_t)j] = 0;
    }
    return DPX_OK;
}

/* ---- substitution tables and BAXT's extension mode: what the setters below share ----
 * One copy of every check and of every step that changes the batch.  A setter is its own admission rule, the shared checks in its
 * documented order, then ensure_ext_records / install_table / clear_table: every check comes before the first change. */
static bool ext_bounds_ok(int32_t zdrop, int32_t endBonus) { return zdrop >= -1 && zdrop <= (1 << 30) && endBonus >= -1 && endBonus <= (1 << 30); }
static bool table_args_ok(int32_t alphabet, const uint8_t *codeOf) {
    if (alphabet < 1 || alphabet > 32 || !codeOf) return false;
    for (int x = 0; x < 256; x++) if ((int)codeOf[x] >= alphabet) return false;
    return true;
}
/* the batch's parameters with the table's largest entry in place of match and its smallest in place of mismatch; `entries` is the
 * caller's array (stride = alphabet) or the host image (stride 32) */
static dpx_params table_extremes(const dpx_batch *b, const void *entries, int32_t alphabet, int32_t stride) {
    dpx_params q = b->prm;
    q.match = -128; q.mismatch = 127;
    for (int r = 0; r < alphabet; r++)
        for (int c = 0; c < alphabet; c++) {
            const int32_t v = static_cast<const int8_t *>(entries)[r * stride + c];
            q.match = std::max(q.match, v); q.mismatch = std::min(q.mismatch, v);
        }
    return q;
}
/* the range check of the batch's storage mode (`fits`: fits_int16, fits_dir or a two-piece wrapper of it) over every pair */
static bool pairs_in_range(const dpx_batch *b, const dpx_params &q, const std::function<bool(const dpx_params &, long long, long long)> &fits) {
    for (const dpx_pair_dev &pd : b->pairs) if (!fits(q, pd.m, pd.n)) return false;
    return true;
}
/* fits_dir for a band-direction batch under two gap pieces: on their componentwise minimum and again on their componentwise maximum,
 * valid lower and upper bounds of every cell (equal pieces: fits_dir itself) */
static bool fits_dir_pieces(dpx_params q, int32_t o2, int32_t e2, long long m, long long n) {
    const int32_t o1 = q.gapOpen, e1 = q.gapExtend;
    q.gapOpen = std::min(o1, o2); q.gapExtend = std::min(e1, e2);
    if (!fits_dir(q, m, n)) return false;
    q.gapOpen = std::max(o1, o2); q.gapExtend = std::max(e1, e2);
    return fits_dir(q, m, n);
}
/* the image of dpx_kernels.h: rows of 32, the 256-byte map behind them */
static void build_table_image(unsigned char (&image)[DPX_SUBST_IMAGE_BYTES], const int8_t *scores, int32_t alphabet, const uint8_t *codeOf) {
    memset(image, 0, sizeof image);
    for (int r = 0; r < alphabet; r++) memcpy(image + r * 32, scores + r * alphabet, (size_t)alphabet);
    memcpy(image + DPX_SUBST_TABLE_BYTES, codeOf, 256);
}
/* the batch's device is bound and, with the scan on, its per-pair records exist */
static int ensure_ext_records(dpx_batch *b, bool scan) {
    int rc = bind_device(b->device);
    if (rc != DPX_OK) return rc;
    if (scan && !b->dExt && b->numPairs) HIP_TRY(g_tbDevCache.take((void **)&b->dExt, b->numPairs * sizeof(dpx_extension), &b->dExtCap));
    return DPX_OK;
}
/* the checked table becomes the batch's, on the device and -- to tell a changed table from the same one, and for
 * dpx_batch_set_second_gap's range check -- on the host.  keepIfSame: the same table again invalidates nothing. */
static int install_table(dpx_batch *b, const unsigned char (&image)[DPX_SUBST_IMAGE_BYTES], int32_t alphabet, bool keepIfSame) {
    if (keepIfSame && b->substAlphabet == alphabet && !memcmp(b->tableImage.data(), image, sizeof image)) return DPX_OK;
    int rc = bind_device(b->device);
    if (rc != DPX_OK) return rc;
    if (!b->dSubst) HIP_TRY(g_tbDevCache.take((void **)&b->dSubst, sizeof image, &b->dSubstCap));
    /* a fill or a walk in flight may still read the previous table */
    if (b->lastStream && b->lastStream != b->stream) HIP_TRY(hipStreamSynchronize(b->lastStream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipMemcpy(b->dSubst, image, sizeof image, hipMemcpyHostToDevice));
    b->tableImage.assign(image, image + sizeof image);
    b->substAlphabet = alphabet;
    invalidate_fill(b);
    return DPX_OK;
}
/* scores == NULL: whatever table the batch holds goes, through whichever setter it came (legal on every batch); the batch runs its
 * plain kernels again */
static int clear_table(dpx_batch *b) {
    if (b->substAlphabet) invalidate_fill(b);
    b->substAlphabet = 0;
    b->tableImage.clear();
    return DPX_OK;
}

int dpx_batch_set_extension(dpx_batch *b, int32_t zdrop, int32_t endBonus) {
    if (!b || !ext_bounds_ok(zdrop, endBonus)) return DPX_ERR_INVALID;
    if (b->prm.algo != DPX_ALGO_BAXT) return DPX_ERR_UNSUPPORTED;
    if (b->bandDirs) return DPX_ERR_UNSUPPORTED; /* refused by design (tests pin it): dpx_batch_set_direction_scoring is a band-direction batch's setter */
    if ((zdrop >= 0 || endBonus >= 0) && b->substAlphabet) return DPX_ERR_UNSUPPORTED; /* (the two go together through dpx_batch_set_extension_table only) */
    int rc = ensure_ext_records(b, zdrop >= 0 || endBonus >= 0);
    if (rc != DPX_OK) return rc;
    b->zdrop = zdrop;
    b->endBonus = endBonus;
    return DPX_OK;
}

/* dpx_batch_set_substitution's and dpx_batch_set_extension_table's batches: BANW / BAXT with matrices or score-only.  Band directions are
 * refused by design (dpx_batch_set_direction_scoring is their setter); a covering BANW band runs as ANW, which has no table kernel */
static bool admits_band_table(const dpx_batch *b) {
    return (b->prm.algo == DPX_ALGO_BANW || b->prm.algo == DPX_ALGO_BAXT) && b->kernelAlgo == b->prm.algo && !b->dirs && !b->bandDirs;
}
/* ... and what both check behind it: the image fits beside the staged strings, and fits_int16's BANW / BAXT bounds hold under the table */
static int check_band_table_fit(const dpx_batch *b, const int8_t *scores, int32_t alphabet) {
    if (subst_lds_bytes(b) > 160u * 1024u) return DPX_ERR_UNSUPPORTED;
    return pairs_in_range(b, table_extremes(b, scores, alphabet, alphabet), fits_int16) ? DPX_OK : DPX_ERR_RANGE;
}

int dpx_batch_set_substitution(dpx_batch *b, const int8_t *scores, int32_t alphabet, const uint8_t *codeOf) {
    if (!b) return DPX_ERR_INVALID;
    if (!scores) return clear_table(b);
    if (!table_args_ok(alphabet, codeOf)) return DPX_ERR_INVALID;
    if (!admits_band_table(b) || extension_on(b)) return DPX_ERR_UNSUPPORTED;
    int rc = check_band_table_fit(b, scores, alphabet);
    if (rc != DPX_OK) return rc;
    unsigned char image[DPX_SUBST_IMAGE_BYTES];
    build_table_image(image, scores, alphabet, codeOf);
    return install_table(b, image, alphabet, false);
}

/* both settings at once, the one way to have both */
int dpx_batch_set_extension_table(dpx_batch *b, int32_t zdrop, int32_t endBonus, const int8_t *scores, int32_t alphabet, const uint8_t *codeOf) {
    if (!b || !scores || !codeOf) return DPX_ERR_INVALID;
    if (!ext_bounds_ok(zdrop, endBonus) || (zdrop < 0 && endBonus < 0)) return DPX_ERR_INVALID;
    if (!table_args_ok(alphabet, codeOf)) return DPX_ERR_INVALID;
    if (!admits_band_table(b) || b->prm.algo != DPX_ALGO_BAXT) return DPX_ERR_UNSUPPORTED;
    int rc = check_band_table_fit(b, scores, alphabet);
    if (rc != DPX_OK) return rc;
    unsigned char image[DPX_SUBST_IMAGE_BYTES];
    build_table_image(image, scores, alphabet, codeOf);
    rc = ensure_ext_records(b, true);
    if (rc == DPX_OK) rc = install_table(b, image, alphabet, false);
    if (rc != DPX_OK) return rc;
    b->zdrop = zdrop;
    b->endBonus = endBonus;
    return DPX_OK;
}

/* the second gap piece of a two-piece batch */
int dpx_batch_set_second_gap(dpx_batch *b, int32_t gapOpen2, int32_t gapExtend2) {
    if (!b) return DPX_ERR_INVALID;
    if (!b->twoPiece) return DPX_ERR_UNSUPPORTED;
    const int32_t lim = 1 << 20; /* validate_params' rule */
    if (gapOpen2 > lim || gapOpen2 < -lim || gapExtend2 > lim || gapExtend2 < -lim) return DPX_ERR_RANGE;
    /* under a table: its largest and smallest entries, as its setter checks */
    const dpx_params q = b->substAlphabet ? table_extremes(b, b->tableImage.data(), b->substAlphabet, 32) : b->prm;
    if (!pairs_in_range(b, q, [&](const dpx_params &qq, long long m, long long n) { return fits_dir_pieces(qq, gapOpen2, gapExtend2, m, n); })) return DPX_ERR_RANGE;
    if (gapOpen2 != b->gapOpen2 || gapExtend2 != b->gapExtend2) invalidate_fill(b);
    b->gapOpen2 = gapOpen2;
    b->gapExtend2 = gapExtend2;
    return DPX_OK;
}

/* all scoring of a band-direction batch, the three settings at once */
int dpx_batch_set_direction_scoring(dpx_batch *b, int32_t zdrop, int32_t endBonus, const int8_t *scores, int32_t alphabet, const uint8_t *codeOf) {
    if (!b || !ext_bounds_ok(zdrop, endBonus)) return DPX_ERR_INVALID;
    if (scores && !table_args_ok(alphabet, codeOf)) return DPX_ERR_INVALID;
    if (!b->bandDirs || b->bandLocal) return DPX_ERR_UNSUPPORTED; /* matrix and score-only batches, the other algorithms (BSW / BASW direction batches included), a covering BANW band (k_affine_dir) */
    const bool scan = zdrop >= 0 || endBonus >= 0;
    if (scan && b->prm.algo != DPX_ALGO_BAXT) return DPX_ERR_UNSUPPORTED;
    unsigned char image[DPX_SUBST_IMAGE_BYTES];
    if (scores) {
        if (!dpx_plan_bdx_waves(*b, true)) return DPX_ERR_UNSUPPORTED; /* one wave's staged strings leave no room in LDS for the table image */
        /* fits_dir under the table and the batch's gap pieces.  (With int8 entries and strings that fit LDS this can only refuse a batch
         * that its creation's own check admitted at its very limit.) */
        const int32_t o2 = b->twoPiece ? b->gapOpen2 : b->prm.gapOpen, e2 = b->twoPiece ? b->gapExtend2 : b->prm.gapExtend;
        if (!pairs_in_range(b, table_extremes(b, scores, alphabet, alphabet),
                            [&](const dpx_params &q, long long m, long long n) { return fits_dir_pieces(q, o2, e2, m, n); })) return DPX_ERR_RANGE;
        build_table_image(image, scores, alphabet, codeOf);
    }
    int rc = ensure_ext_records(b, scan);
    if (rc == DPX_OK) rc = scores ? install_table(b, image, alphabet, true) : clear_table(b);
    if (rc != DPX_OK) return rc;
    if (zdrop != b->zdrop || endBonus != b->endBonus) invalidate_fill(b);
    b->zdrop = zdrop;
    b->endBonus = endBonus;
    return DPX_OK;
}

/* dpx_batch_set_direction_table's and dpx_batch_set_score_table's algorithms: the batch's own, not the kernel's -- a covering BANW / BASW
 * band that runs the ANW / ASW kernels is not admitted */
static bool one_of_anw_asw_asg(const dpx_batch *b) { return b->prm.algo == DPX_ALGO_ANW || b->prm.algo == DPX_ALGO_ASW || b->prm.algo == DPX_ALGO_ASG; }

/* the table of an ANW / ASW / ASG direction batch (k_dirtab_fill) */
int dpx_batch_set_direction_table(dpx_batch *b, const int8_t *scores, int32_t alphabet, const uint8_t *codeOf) {
    if (!b) return DPX_ERR_INVALID;
    if (!scores) return clear_table(b);
    if (!table_args_ok(alphabet, codeOf)) return DPX_ERR_INVALID;
    if (!one_of_anw_asw_asg(b) || !b->dirs || !(b->flags & DPX_KEEP_DIRECTIONS)) return DPX_ERR_UNSUPPORTED;
    if (!pairs_in_range(b, table_extremes(b, scores, alphabet, alphabet), fits_dir)) return DPX_ERR_RANGE;
    unsigned char image[DPX_SUBST_IMAGE_BYTES];
    build_table_image(image, scores, alphabet, codeOf);
    return install_table(b, image, alphabet, true);
}

/* the table of an ANW / ASW / ASG score-only batch (k_scoretab_fill / k_scoretab_lanes) */
int dpx_batch_set_score_table(dpx_batch *b, const int8_t *scores, int32_t alphabet, const uint8_t *codeOf) {
    if (!b) return DPX_ERR_INVALID;
    if (!scores) return clear_table(b);
    if (!table_args_ok(alphabet, codeOf)) return DPX_ERR_INVALID;
    if (!one_of_anw_asw_asg(b) || b->store || b->dirs || !(b->flags & DPX_SCORE_ONLY)) return DPX_ERR_UNSUPPORTED;
    if (!dpx_plan_scoretab_fits(*b, t_err)) return DPX_ERR_UNSUPPORTED;
    if (!pairs_in_range(b, table_extremes(b, scores, alphabet, alphabet), fits_int16)) return DPX_ERR_RANGE;
    unsigned char image[DPX_SUBST_IMAGE_BYTES];
    build_table_image(image, scores, alphabet, codeOf);
    return install_table(b, image, alphabet, true);
}

/* ---- orientation: dpx_batch_set_reversed ----
 * The kernels find a pair's strings through the pair table, so the setter builds reversed copies of the flagged pairs' strings on the
 * device (k_reverse_strings) behind a device copy of the batch's bytes, points the flagged pairs at them and the launch arguments'
 * `seq` at the new allocation.  Nothing is reversed in place (pairs share bytes), no sequence byte crosses PCIe and the host reads
 * none.  The plan is a function of sizes and stays. */
static void set_seq_pointer(dpx_batch *b, char *seq) {
    b->dSeq = seq;
    b->args.seq = seq;
    if (b->pkArgs.seq) b->pkArgs.seq = seq;
    if (b->dirs) b->dirArgs.seq = seq;
}

int dpx_batch_set_reversed(dpx_batch *b, const uint8_t *reversed) {
    if (!b) return DPX_ERR_INVALID;
    if (b->prm.algo != DPX_ALGO_BANW && b->prm.algo != DPX_ALGO_BAXT) return DPX_ERR_UNSUPPORTED;
    const size_t np = b->numPairs;
    std::vector<int32_t> flagged;
    for (size_t i = 0; reversed && i < np; i++) if (reversed[i]) flagged.push_back((int32_t)i);
    if (flagged.empty() && !b->revCount) return DPX_OK; /* no mask before, none now */
    PhaseTrace trace;
    /* the layout, from the pairs' own indices (a flagged pair's are in revSaved); every check comes before the first change */
    std::vector<dpx_pair_dev> table = b->pairs;
    for (const dpx_batch::RevSaved &sv : b->revSaved) { table[(size_t)sv.pair].refIdx = sv.refIdx; table[(size_t)sv.pair].qryIdx = sv.qryIdx; }
    std::vector<dpx_rev_job> jobs;
    std::vector<dpx_batch::RevSaved> saved;
    jobs.reserve(2 * flagged.size());
    saved.reserve(flagged.size());
    /* (index, length) -> the job that copies it: a string that many pairs share is copied once.  Open addressing, at most half full. */
    size_t slots = 16;
    while (slots < 4 * flagged.size()) slots <<= 1;
    std::vector<int32_t> jobOf(slots, -1);
    size_t off = b->seqBytes;
    for (const int32_t p : flagged) {
        dpx_pair_dev &pd = table[(size_t)p];
        saved.push_back({p, pd.refIdx, pd.qryIdx});
        for (int side = 0; side < 2; side++) {
            int32_t &idx = side ? pd.qryIdx : pd.refIdx;
            const int32_t len = side ? pd.m : pd.n;
            if (len <= 0) continue; /* (an empty string is never read: its index stays) */
            size_t h = (size_t)((((uint64_t)(uint32_t)idx << 32) | (uint32_t)len) * 0x9E3779B97F4A7C15ull >> 32) & (slots - 1);
            while (jobOf[h] >= 0 && (jobs[(size_t)jobOf[h]].src != idx || jobs[(size_t)jobOf[h]].len != len)) h = (h + 1) & (slots - 1);
            if (jobOf[h] < 0) {
                if (off + dpx_rev_slot_bytes((size_t)len) > (size_t)0x7fffffff) {
                    t_err = "dpx_batch_set_reversed: the reversed copies end beyond byte 2^31 of the sequence buffer (pair " + std::to_string(p) + "), int32 offsets cannot reach them";
                    return DPX_ERR_RANGE;
                }
                jobOf[h] = (int32_t)jobs.size();
                jobs.push_back({idx, (int32_t)off, len, 0});
                off += dpx_rev_slot_bytes((size_t)len);
            }
            idx = jobs[(size_t)jobOf[h]].dst;
        }
    }
    trace.mark("set_reversed: layout");
    const size_t jobsAt = align_up(off, 256), flaggedAt = jobsAt + align_up(jobs.size() * sizeof(dpx_rev_job), 256);
    const size_t need = flaggedAt + align_up(flagged.size() * sizeof(int32_t), 256);
    int rc = bind_device(b->device);
    if (rc != DPX_OK) return rc;
    /* a fill, a walk or an export in flight may still read the present strings and table */
    if (b->lastStream && b->lastStream != b->stream) HIP_TRY(hipStreamSynchronize(b->lastStream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    char *fresh = nullptr;
    size_t freshCap = 0;
    if (!flagged.empty()) {
        HIP_TRY(g_arenaCache.take((void **)&fresh, need, &freshCap));
        trace.mark("set_reversed: allocation");
        hipError_t e = hipMemcpyAsync(fresh, b->dSeqOwn, b->seqBytes, hipMemcpyDeviceToDevice, b->stream);
        if (e == hipSuccess && !jobs.empty()) e = hipMemcpy(fresh + jobsAt, jobs.data(), jobs.size() * sizeof(dpx_rev_job), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(fresh + flaggedAt, flagged.data(), flagged.size() * sizeof(int32_t), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = dpx_launch_reverse_strings(fresh, reinterpret_cast<const dpx_rev_job *>(fresh + jobsAt), (int)jobs.size(), b->stream);
        if (e == hipSuccess && np) e = hipMemcpy(b->dPairs, table.data(), np * sizeof(dpx_pair_dev), hipMemcpyHostToDevice);
        if (e != hipSuccess) { /* (the batch keeps its present mask) */
            (void)hipStreamSynchronize(b->stream);
            if (np) (void)hipMemcpy(b->dPairs, b->pairs.data(), np * sizeof(dpx_pair_dev), hipMemcpyHostToDevice);
            g_arenaCache.park(fresh, freshCap);
            return hip_fail(e, "dpx_batch_set_reversed");
        }
    } else if (np) HIP_TRY(hipMemcpy(b->dPairs, table.data(), np * sizeof(dpx_pair_dev), hipMemcpyHostToDevice));
    g_arenaCache.park(b->dRev, b->dRevCap); /* (idle: both streams were waited for) */
    b->dRev = fresh; b->dRevCap = freshCap;
    b->dFlagged = fresh ? reinterpret_cast<const int32_t *>(fresh + flaggedAt) : nullptr;
    b->revCount = flagged.size();
    b->revSaved = std::move(saved);
    b->pairs = std::move(table);
    set_seq_pointer(b, fresh ? fresh : b->dSeqOwn);
    if (fresh) b->uploadPending = true; /* the copies are being written on b->stream: a fill on a caller's stream waits for it once */
    invalidate_fill(b);
    trace.mark("set_reversed: uploads+launch");
    return DPX_OK;
}

int dpx_batch_extensions(dpx_batch *b, dpx_extension *out) {
    if (!b || !out) return DPX_ERR_INVALID;
    if (!b->filled) return DPX_ERR_NOT_FILLED;
    if (!b->extFilled) return DPX_ERR_UNSUPPORTED;
    int rc = bind_device(b->device);
    if (rc != DPX_OK) return rc;
    if (b->lastStream && b->lastStream != b->stream) HIP_TRY(hipStreamSynchronize(b->lastStream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (b->numPairs) HIP_TRY(hipMemcpy(out, b->dExt, b->numPairs * sizeof(dpx_extension), hipMemcpyDeviceToHost));
    return check_guard(b);
}

/* ---- result text: device traceback -> per-pair block lengths -> exclusive scan -> packed blocks -> D2H of the real bytes ----
 * (the reference's V15 packed variable-length strings, cuda/LNW/LinearNeedlemanWunschV15.cu:168-172,372-425; the blocks are
 * already formatted as c++/main.cpp prints them, so a driver writes a batch with one fwrite) */

/* The device traceback of every pair into the line buffers (b->dTb must exist), on the batch's stream, unless the lines of this fill
 * are there already: the one place that launches the walk, for the text pipeline and the CIGAR path alike. */
static int traceback_lines(dpx_batch *b) {
    if (b->tbLinesValid) return DPX_OK;
    const dpx_route r = route_of(b); /* (which walk, and why: dpx_plan.cpp) */
    const int n = (int)b->numPairs, walk = r.walkMode;
    switch (r.walk) {
    case DPX_WALK_PLAIN: HIP_TRY(dpx_launch_traceback(b->args, n, b->kernelAlgo, b->R, b->planes, walk, b->dTbOff, b->dTb, b->dTbLen, b->stream)); break;
    case DPX_WALK_DIR: HIP_TRY(dpx_launch_traceback_dir(b->dirArgs, n, b->kernelAlgo, b->R, b->dTbOff, b->dTb, b->dTbLen, b->stream)); break;
    case DPX_WALK_BASW: HIP_TRY(dpx_launch_basw_traceback(b->args, n, walk, b->dTbOff, b->dTb, b->dTbLen, b->stream)); break;
    case DPX_WALK_BANW: HIP_TRY(dpx_launch_banw_traceback(b->args, n, walk, b->dTbOff, b->dTb, b->dTbLen, b->stream)); break;
    case DPX_WALK_SUBST: HIP_TRY(dpx_launch_subst_traceback(subst_args(b), n, walk, b->dTbOff, b->dTb, b->dTbLen, b->stream)); break;
    case DPX_WALK_BDIR: HIP_TRY(dpx_launch_bdir_traceback(b->args, n, b->dTbOff, b->dTb, b->dTbLen, b->stream)); break;
    case DPX_WALK_BD2: HIP_TRY(dpx_launch_bd2_traceback(b->args, n, b->dTbOff, b->dTb, b->dTbLen, b->stream)); break;
    case DPX_WALK_BDL: HIP_TRY(dpx_launch_bdl_traceback(b->args, n, b->prm.algo == DPX_ALGO_BASW, b->dTbOff, b->dTb, b->dTbLen, b->stream)); break;
    }
    /* reversed pairs (dpx_batch_set_reversed): their lines come out of the walk in the reversed frame and are turned round here, once */
    if (b->revCount) HIP_TRY(dpx_launch_flip_lines(b->dPairs, b->dFlagged, (int)b->revCount, b->dTbLen, b->dTbOff, b->dTb, b->stream));
    b->tbLinesValid = true;
    return DPX_OK;
}

/* the fill ran on a caller's stream: order the batch's stream behind it without blocking the host */
static int order_behind_fill(dpx_batch *b) {
    if (b->lastStream && b->lastStream != b->stream) {
        if (!b->evOrder) HIP_TRY(hipEventCreateWithFlags(&b->evOrder, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(b->evOrder, b->lastStream));
        HIP_TRY(hipStreamWaitEvent(b->stream, b->evOrder, 0));
    }
    return DPX_OK;
}

/* stage 1, asynchronous on the batch's stream: kernels + D2H of the offsets / lengths */

static int output_begin(dpx_batch *b, uint64_t firstNumber) {
    PhaseTrace trace;
    const size_t np = b->numPairs;
    if (b->outState == 2 && b->outFirst == firstNumber) return DPX_OK; /* already on the host */
    if (b->outState == 1 && b->outFirst == firstNumber) return DPX_OK; /* already in flight */
    if (b->outState == 1) HIP_TRY(hipStreamSynchronize(b->stream));    /* a run with another numbering is in flight: let it finish */
    if (!b->dTb || !b->dOut || !b->hMeta) { /* buffers of the output path, on first use (a failed attempt is simply repeated) */
        const uint64_t lines = b->tbOff[np];
        if (!b->dTb) HIP_TRY(g_tbDevCache.take((void **)&b->dTb, (size_t)std::max<uint64_t>(lines, 16), &b->dTbCap));
        /* packed text, worst case: every alignment m + n long, 20 digits of pair number, 11 of score */
        if (!b->dOut) HIP_TRY(g_tbDevCache.take((void **)&b->dOut, (size_t)(lines + 40ull * np + 16), &b->dOutCap));
        if (!b->hMeta) HIP_TRY(g_tbHostCache.take((void **)&b->hMeta, (np + 1) * sizeof(uint64_t) + np * sizeof(int32_t) + 16 + kSmallResultBytes, &b->hMetaCap));
        trace.mark("output: buffers");
    }
    uint64_t *hOff = reinterpret_cast<uint64_t *>(b->hMeta);
    int32_t *hLen = reinterpret_cast<int32_t *>(hOff + np + 1);
    { const int rc = order_behind_fill(b); if (rc != DPX_OK) return rc; }
    const bool timeOut = (b->flags & DPX_TIME_FILLS) != 0;
    if (timeOut) {
        if (!b->evOut0) HIP_TRY(hipEventCreate(&b->evOut0));
        if (!b->evOut1) HIP_TRY(hipEventCreate(&b->evOut1));
        HIP_TRY(hipEventRecord(b->evOut0, b->stream));
    }
    { const int rc = traceback_lines(b); if (rc != DPX_OK) return rc; }
    HIP_TRY(dpx_launch_output(b->dPairs, b->dScore, b->dTbLen, b->dTbOff, b->dTb, (int)np, (unsigned long long)firstNumber,
                              reinterpret_cast<unsigned long long *>(b->dOutScratch), reinterpret_cast<unsigned long long *>(b->dOutOff), b->dOut,
                              false, false, b->stream));
    if (timeOut) { HIP_TRY(hipEventRecord(b->evOut1, b->stream)); b->outTimed = true; }
    b->textCopied = false;
    b->resultsCopied = false;
    if (np) {
        HIP_TRY(hipMemcpyAsync(hOff, b->dOutOff, (np + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipMemcpyAsync(hLen, b->dTbLen, np * sizeof(int32_t), hipMemcpyDeviceToHost, b->stream));
        /* small batches: the text follows at once, at its worst-case size -- dpx_batch_output_end() then waits once instead of waiting,
         * reading the real size and copying (a second round trip of ~15 us; the class-per-pair drivers pay it 200 times per 4000 pairs) */
        const size_t worst = (size_t)(b->tbOff[np] + 40ull * np + 16);
        if (worst <= ((size_t)256 << 10)) {
            if (!b->hOut || b->hOutCap < worst + 1) {
                g_tbHostCache.park(b->hOut, b->hOutCap);
                b->hOut = nullptr;
                HIP_TRY(g_tbHostCache.take((void **)&b->hOut, worst + 1, &b->hOutCap));
            }
            HIP_TRY(hipMemcpyAsync(b->hOut, b->dOut, worst, hipMemcpyDeviceToHost, b->stream));
            b->textCopied = true;
            /* ... and so do score / end row / end column (they lie side by side in the arena): dpx_batch_results() after this call is a
             * wait and three memcpy instead of a wait and a synchronous copy of its own */
            const size_t stride = (size_t)((const char *)b->dEndRow - (const char *)b->dScore), bytes = np * sizeof(int32_t);
            if ((const char *)b->dEndCol - (const char *)b->dEndRow == (ptrdiff_t)stride && 2 * stride + bytes <= kSmallResultBytes &&
                (!b->lastStream || b->lastStream == b->stream)) {
                char *tail = b->hMeta + (np + 1) * sizeof(uint64_t) + np * sizeof(int32_t) + 16;
                HIP_TRY(hipMemcpyAsync(tail, b->dScore, 2 * stride + bytes, hipMemcpyDeviceToHost, b->stream));
                b->resultsCopied = true;
            }
        }
    } else {
        hOff[0] = 0;
    }
    b->outState = 1;
    b->outFirst = firstNumber;
    trace.mark("output: launches");
    return DPX_OK;
}

/* stage 2: wait, then copy exactly the bytes the blocks occupy */
static int output_end(dpx_batch *b) {
    if (b->outState == 2) return DPX_OK;
    if (b->outState != 1) return DPX_ERR_INVALID;
    PhaseTrace trace;
    HIP_TRY(hipStreamSynchronize(b->stream));
    trace.mark("output: wait for device");
    const uint64_t total = reinterpret_cast<const uint64_t *>(b->hMeta)[b->numPairs];
    if (b->textCopied) { /* (the text came with the offsets) */
        b->hOut[total] = 0;
        b->hOutBytes = (size_t)total;
        b->outState = 2;
        trace.mark("output: D2H text");
        return DPX_OK;
    }
    if (!b->hOut || b->hOutCap < total + 1) {
        g_tbHostCache.park(b->hOut, b->hOutCap);
        b->hOut = nullptr;
        HIP_TRY(g_tbHostCache.take((void **)&b->hOut, (size_t)total + 1, &b->hOutCap));
        trace.mark("output: pinned text buffer");
    }
    if (total) {
        HIP_TRY(hipMemcpyAsync(b->hOut, b->dOut, (size_t)total, hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));
    }
    b->hOut[total] = 0;
    b->hOutBytes = (size_t)total;
    b->outState = 2;
    trace.mark("output: D2H text");
    return DPX_OK;
}

int dpx_batch_output_begin(dpx_batch *b, uint64_t firstPairNumber) {
    if (!b) return DPX_ERR_INVALID;
    if (!b->store) return DPX_ERR_NO_MATRIX;
    if (!b->filled) return DPX_ERR_NOT_FILLED;
    int rc = bind_device(b->device);
    if (rc != DPX_OK) return rc;
    return output_begin(b, firstPairNumber);
}

int dpx_batch_output_end(dpx_batch *b, const char **text, size_t *bytes, const uint64_t **offsets) {
    if (!b) return DPX_ERR_INVALID;
    if (b->outState == 0) return DPX_ERR_NOT_FILLED; /* no dpx_batch_output_begin() since the last fill */
    int rc = bind_device(b->device);
    if (rc != DPX_OK) return rc;
    rc = output_end(b);
    if (rc != DPX_OK) return rc;
    if (text) *text = b->hOut;
    if (bytes) *bytes = b->hOutBytes;
    if (offsets) *offsets = reinterpret_cast<const uint64_t *>(b->hMeta);
    return DPX_OK;
}

/* pinned text buffers handed to the caller by dpx_batch_output_take(): pointer -> capacity, for dpx_text_free() */
namespace { struct Taken { void *ptr; size_t cap; int device; }; std::mutex g_takenMu; std::vector<Taken> g_taken; }

int dpx_batch_output_take(dpx_batch *b, char **text, size_t *bytes) {
    if (!b || !text) return DPX_ERR_INVALID;
    if (b->outState == 0) return DPX_ERR_NOT_FILLED;
    int rc = bind_device(b->device);
    if (rc != DPX_OK) return rc;
    rc = output_end(b);
    if (rc != DPX_OK) return rc;
    { std::lock_guard<std::mutex> lk(g_takenMu); g_taken.push_back(Taken{(void *)b->hOut, b->hOutCap, b->device}); }
    *text = b->hOut;
    if (bytes) *bytes = b->hOutBytes;
    b->hOut = nullptr; /* the batch no longer owns it; a later dpx_batch_traceback() / _output_end() rebuilds the text */
    b->hOutCap = 0;
    b->outState = 0;
    return DPX_OK;
}

int dpx_text_free(char *text) {
    if (!text) return DPX_OK;
    size_t cap = 0;
    int dev = -1;
    {
        std::lock_guard<std::mutex> lk(g_takenMu);
        for (size_t i = 0; i < g_taken.size(); i++)
            if (g_taken[i].ptr == (void *)text) { cap = g_taken[i].cap; dev = g_taken[i].device; g_taken.erase(g_taken.begin() + (long)i); break; }
    }
    if (!cap) return DPX_ERR_INVALID; /* not a buffer dpx_batch_output_take() handed out */
    if (dev >= 0) { (void)hipSetDevice(dev); t_device = dev; }
    g_tbHostCache.park(text, cap);
    return DPX_OK;
}

int dpx_batch_traceback(dpx_batch *b, size_t pair, char *refLine, char *relLine, char *qryLine, int32_t *len) {
    if (!b || pair >= b->numPairs) return DPX_ERR_INVALID;
    if (!b->store) return DPX_ERR_NO_MATRIX;
    if (!b->filled) return DPX_ERR_NOT_FILLED;
    if (b->outState != 2) { /* first call after a fill walks every pair of the batch on the device; later calls only copy lines */
        int rc = bind_device(b->device);
        if (rc != DPX_OK) return rc;
        rc = output_begin(b, b->outState == 1 ? b->outFirst : 0);
        if (rc == DPX_OK) rc = output_end(b);
        if (rc != DPX_OK) return rc;
    }
    const uint64_t *hOff = reinterpret_cast<const uint64_t *>(b->hMeta);
    const int32_t *hLen = reinterpret_cast<const int32_t *>(hOff + b->numPairs + 1);
    const int k = hLen[pair];
    /* the pair's block ends with its three lines, each k characters + '\n' */
    const char *lines = b->hOut + hOff[pair + 1] - 3 * (size_t)(k + 1);
    char *dst[3] = {refLine, relLine, qryLine};
    for (int l = 0; l < 3; l++)
        if (dst[l]) { memcpy(dst[l], lines + (size_t)l * (size_t)(k + 1), (size_t)k); dst[l][k] = 0; }
    if (len) *len = k;
    return DPX_OK;
}

/* ---- CIGARs: the same traceback lines, run-length encoded on the device (dpx_cigar_kernels.hip) -> D2H of one record per pair,
 * then of exactly the ops.  Buffers of its own, so the text pipeline and this one may follow the same fill in either order. */

int dpx_batch_cigars_begin(dpx_batch *b, unsigned flags) {
    if (!b || (flags & ~DPX_CIGAR_M) != 0) return DPX_ERR_INVALID;
    if (!b->store) return DPX_ERR_NO_MATRIX;
    if (!b->filled) return DPX_ERR_NOT_FILLED;
    int rc = bind_device(b->device);
    if (rc != DPX_OK) return rc;
    const size_t np = b->numPairs, recBytes = np * sizeof(dpx_alignment);
    const uint64_t lines = b->tbOff[np];
    /* buffers, on first use (a failed attempt is simply repeated); ops, worst case: one per column of every line capacity */
    if (!b->dTb) HIP_TRY(g_tbDevCache.take((void **)&b->dTb, (size_t)std::max<uint64_t>(lines, 16), &b->dTbCap));
    if (!b->dCigar) HIP_TRY(g_tbDevCache.take((void **)&b->dCigar, recBytes + (1 + dpx_cigar_scan_tiles(np)) * sizeof(uint64_t) + 16, &b->dCigarCap));
    if (!b->dCigarOps) HIP_TRY(g_tbDevCache.take((void **)&b->dCigarOps, (size_t)(lines / 3) * sizeof(uint32_t) + 16, &b->dCigarOpsCap));
    if (!b->hCigar) HIP_TRY(g_tbHostCache.take((void **)&b->hCigar, recBytes + sizeof(uint64_t) + 16, &b->hCigarCap));
    unsigned long long *dTotal = reinterpret_cast<unsigned long long *>(b->dCigar + recBytes); /* (48 bytes per record: 8-byte aligned) */
    if (np) {
        rc = order_behind_fill(b);
        if (rc == DPX_OK) rc = traceback_lines(b);
        if (rc != DPX_OK) return rc;
        HIP_TRY(dpx_launch_cigars(b->dPairs, b->dEndRow, b->dEndCol, b->dTbLen, b->dTbOff, b->dTb, (int)np, flags,
                                  reinterpret_cast<dpx_alignment *>(b->dCigar), dTotal + 1, dTotal, b->dCigarOps, b->stream));
        if (b->revCount) HIP_TRY(dpx_launch_map_records(b->dPairs, b->dFlagged, (int)b->revCount, reinterpret_cast<dpx_alignment *>(b->dCigar), b->stream));
        HIP_TRY(hipMemcpyAsync(b->hCigar, b->dCigar, recBytes + sizeof(uint64_t), hipMemcpyDeviceToHost, b->stream));
    } else {
        memset(b->hCigar, 0, sizeof(uint64_t)); /* a batch without pairs: no records, no ops */
    }
    b->cigarFlags = flags;
    b->cigarState = 1;
    return DPX_OK;
}

int dpx_batch_cigars_end(dpx_batch *b, const dpx_alignment **records, const uint32_t **ops, uint64_t *numOps) {
    if (!b) return DPX_ERR_INVALID;
    if (b->cigarState == 0) return DPX_ERR_NOT_FILLED; /* no dpx_batch_cigars_begin() since the last fill */
    int rc = bind_device(b->device);
    if (rc != DPX_OK) return rc;
    if (b->cigarState == 1) {
        HIP_TRY(hipStreamSynchronize(b->stream));
        uint64_t total = 0;
        memcpy(&total, b->hCigar + b->numPairs * sizeof(dpx_alignment), sizeof total);
        const size_t bytes = (size_t)total * sizeof(uint32_t);
        if (!b->hCigarOps || b->hCigarOpsCap < bytes + 16) {
            g_tbHostCache.park(b->hCigarOps, b->hCigarOpsCap);
            b->hCigarOps = nullptr;
            HIP_TRY(g_tbHostCache.take((void **)&b->hCigarOps, bytes + 16, &b->hCigarOpsCap));
        }
        if (bytes) {
            HIP_TRY(hipMemcpyAsync(b->hCigarOps, b->dCigarOps, bytes, hipMemcpyDeviceToHost, b->stream));
            HIP_TRY(hipStreamSynchronize(b->stream));
        }
        b->cigarOps = total;
        b->cigarState = 2;
    }
    if (records) *records = reinterpret_cast<const dpx_alignment *>(b->hCigar);
    if (ops) *ops = b->hCigarOps;
    if (numOps) *numOps = b->cigarOps;
    return DPX_OK;
}

/* ---- difference strings: the same traceback lines once more, as MD or cs text per pair (dpx_diff_kernels.hip) -> D2H of the
 * numPairs + 1 offsets, then of exactly the bytes.  Buffers of their own per kind, so text, CIGARs and these may follow the same fill
 * in any order. */

int dpx_batch_diffs_begin(dpx_batch *b, unsigned kinds) {
    if (!b || kinds == 0 || (kinds & ~(DPX_DIFF_MD | DPX_DIFF_CS)) != 0) return DPX_ERR_INVALID;
    if (!b->store) return DPX_ERR_NO_MATRIX;
    if (!b->filled) return DPX_ERR_NOT_FILLED;
    int rc = bind_device(b->device);
    if (rc != DPX_OK) return rc;
    const size_t np = b->numPairs, offBytes = (np + 1) * sizeof(uint64_t);
    const uint64_t lines = b->tbOff[np];
    if (!b->dTb) HIP_TRY(g_tbDevCache.take((void **)&b->dTb, (size_t)std::max<uint64_t>(lines, 16), &b->dTbCap));
    if (np) {
        rc = order_behind_fill(b);
        if (rc == DPX_OK) rc = traceback_lines(b);
        if (rc != DPX_OK) return rc;
    }
    for (int k = 0; k < 2; k++) {
        const unsigned kind = k == 0 ? DPX_DIFF_MD : DPX_DIFF_CS;
        if (!(kinds & kind)) continue;
        /* buffers, on first use (a failed attempt is simply repeated); text, worst case: three bytes per column of every line capacity */
        if (!b->dDiffOff[k]) HIP_TRY(g_tbDevCache.take((void **)&b->dDiffOff[k], offBytes + dpx_diff_scan_tiles(np) * sizeof(uint64_t) + 16, &b->dDiffOffCap[k]));
        if (!b->dDiffText[k]) HIP_TRY(g_tbDevCache.take((void **)&b->dDiffText[k], (size_t)lines + 16, &b->dDiffTextCap[k]));
        if (!b->hDiffOff[k]) HIP_TRY(g_tbHostCache.take((void **)&b->hDiffOff[k], offBytes + 16, &b->hDiffOffCap[k]));
        if (np) {
            unsigned long long *dOff = reinterpret_cast<unsigned long long *>(b->dDiffOff[k]);
            HIP_TRY(dpx_launch_diffs(kind, b->dPairs, b->dTbLen, b->dTbOff, b->dTb, (int)np, dOff, dOff + np + 1, b->dDiffText[k], b->stream));
            HIP_TRY(hipMemcpyAsync(b->hDiffOff[k], b->dDiffOff[k], offBytes, hipMemcpyDeviceToHost, b->stream));
        } else {
            memset(b->hDiffOff[k], 0, sizeof(uint64_t)); /* a batch without pairs: one offset of 0, no bytes */
        }
        b->diffState[k] = 1;
    }
    return DPX_OK;
}

int dpx_batch_diffs_end(dpx_batch *b, unsigned kind, const char **text, size_t *bytes, const uint64_t **offsets) {
    if (!b || (kind != DPX_DIFF_MD && kind != DPX_DIFF_CS)) return DPX_ERR_INVALID;
    const int k = kind == DPX_DIFF_MD ? 0 : 1;
    if (b->diffState[k] == 0) return DPX_ERR_NOT_FILLED; /* no dpx_batch_diffs_begin() of this kind since the last fill */
    int rc = bind_device(b->device);
    if (rc != DPX_OK) return rc;
    const uint64_t *hOff = reinterpret_cast<const uint64_t *>(b->hDiffOff[k]);
    if (b->diffState[k] == 1) {
        HIP_TRY(hipStreamSynchronize(b->stream));
        const size_t total = (size_t)hOff[b->numPairs];
        if (!b->hDiffText[k] || b->hDiffTextCap[k] < total + 1 + 16) {
            g_tbHostCache.park(b->hDiffText[k], b->hDiffTextCap[k]);
            b->hDiffText[k] = nullptr;
            HIP_TRY(g_tbHostCache.take((void **)&b->hDiffText[k], total + 1 + 16, &b->hDiffTextCap[k]));
        }
        if (total) {
            HIP_TRY(hipMemcpyAsync(b->hDiffText[k], b->dDiffText[k], total, hipMemcpyDeviceToHost, b->stream));
            HIP_TRY(hipStreamSynchronize(b->stream));
        }
        b->hDiffText[k][total] = 0;
        b->diffState[k] = 2;
    }
    if (text) *text = b->hDiffText[k];
    if (bytes) *bytes = (size_t)hOff[b->numPairs];
    if (offsets) *offsets = hOff;
    return DPX_OK;
}

int dpx_cigar_text(const uint32_t *ops, size_t numOps, char *out, size_t cap, size_t *len) {
    if ((!ops && numOps) || (!out && cap)) return DPX_ERR_INVALID;
    static const char letters[] = "MID....=X"; /* BAM's numbering; 3..6 (N S H P) never come out of the engine */
    size_t need = numOps ? 0 : 1; /* "*" */
    for (size_t k = 0; k < numOps; k++) {
        const uint32_t code = ops[k] & 0xFu;
        if (code > 8u || letters[code] == '.') return DPX_ERR_INVALID;
        uint32_t v = ops[k] >> 4;
        do { need++; v /= 10u; } while (v);
        need++;
    }
    if (len) *len = need;
    if (cap < need + 1) return DPX_ERR_INVALID;
    char *q = out;
    if (!numOps) *q++ = '*';
    for (size_t k = 0; k < numOps; k++) {
        char digits[10];
        int d = 0;
        uint32_t v = ops[k] >> 4;
        do { digits[d++] = (char)('0' + (int)(v % 10u)); v /= 10u; } while (v);
        while (d) *q++ = digits[--d];
        *q++ = letters[ops[k] & 0xFu];
    }
    *q = 0;
    return DPX_OK;
}

int dpx_batch_describe(dpx_batch *b, char *buf, size_t cap) {
    if (!b || !buf || !cap) return DPX_ERR_INVALID;
    int len = dpx_plan_describe(*b, knobs().tbWalk, b->zdrop, b->endBonus, b->substAlphabet, buf, cap);
    if (b->revCount && len > 0 && (size_t)len < cap) /* (the two blocks are diagnostics like pool_addr: the tests overwrite them between calls) */
        len += snprintf(buf + len, cap - (size_t)len, " reversed=%zu rev_addr=0x%llx rev_bytes=%zu lines_addr=0x%llx lines_bytes=%zu", b->revCount,
                        (unsigned long long)(uintptr_t)b->dRev, b->dRevCap, (unsigned long long)(uintptr_t)b->dTb, b->dTbCap);
    if (b->dMat && len > 0 && (size_t)len < cap) { /* the matrix pool: how it was built, and the memset time of every candidate that was timed */
        const PoolRecord &r = b->poolRec;
        len += snprintf(buf + len, cap - (size_t)len, " pool=%s pool_bytes=%zu pool_addr=0x%llx pool_chunk_mb=%zu pool_kept=%d pool_memset_ms=", r.mode.c_str(), b->matPoolBytes,
                        (unsigned long long)(uintptr_t)b->dMat, r.chunkBytes >> 20, r.kept);
        for (size_t k = 0; k < r.candidatesMs.size() && (size_t)len < cap; k++)
            len += snprintf(buf + len, cap - (size_t)len, "%s%.3f", k ? "," : "", r.candidatesMs[k]);
        if (r.candidatesMs.empty() && (size_t)len < cap) len += snprintf(buf + len, cap - (size_t)len, "untimed");
        if ((size_t)len < cap) len += snprintf(buf + len, cap - (size_t)len, " pool_fill_ms=");
        for (size_t k = 0; k < r.fillMs.size() && (size_t)len < cap; k++)
            len += snprintf(buf + len, cap - (size_t)len, "%s%.3f", k ? "," : "", r.fillMs[k]);
        if (r.fillMs.empty() && (size_t)len < cap) len += snprintf(buf + len, cap - (size_t)len, "unshopped");
        if (!r.kinds.empty() && (size_t)len < cap) {
            len += snprintf(buf + len, cap - (size_t)len, " pool_kinds=");
            for (size_t k = 0; k < r.kinds.size() && (size_t)len < cap; k++) len += snprintf(buf + len, cap - (size_t)len, "%s%s", k ? "," : "", r.kinds[k].c_str());
        }
        if (!r.ranges.empty() && (size_t)len < cap) {
            len += snprintf(buf + len, cap - (size_t)len, " pool_ranges=");
            for (size_t k = 0; k < r.ranges.size() && (size_t)len < cap; k++) len += snprintf(buf + len, cap - (size_t)len, "%s%s", k ? "," : "", r.ranges[k].c_str());
        }
    } else if (!b->dMat && len > 0 && (size_t)len < cap) len += snprintf(buf + len, cap - (size_t)len, " pool_addr=0x0"); /* no pool: a score-only batch */
    return DPX_OK;
}

int dpx_batch_info(dpx_batch *b, size_t *numPairs, uint64_t *cells, uint64_t *matrixBytes, uint64_t *algorithmicBytes) {
    if (!b) return DPX_ERR_INVALID;
    if (numPairs) *numPairs = b->numPairs;
    if (cells) *cells = b->cells;
    if (matrixBytes) *matrixBytes = b->matElems * sizeof(int16_t);
    if (algorithmicBytes) *algorithmicBytes = b->algBytes;
    return DPX_OK;
}

/* ------------------------------------------------------------------------------------------ one-shot */

int dpx_align_batch(const dpx_params *params, const char *sequences, size_t numBytes, const dpx_seq_pair *pairs,
                    size_t numPairs, int32_t *scores, int32_t *endRow, int32_t *endCol, int16_t **H, int16_t **I,
                    int16_t **D) {
    const bool wantMat = H || I || D;
    dpx_batch *b = nullptr;
    int rc = dpx_batch_create(params, sequences, numBytes, pairs, 0, numPairs, wantMat ? DPX_KEEP_MATRICES : DPX_SCORE_ONLY, &b);
    if (rc != DPX_OK) return rc;
    rc = dpx_batch_fill(b, nullptr);
    if (rc == DPX_OK) rc = dpx_batch_results(b, scores, endRow, endCol);
    for (size_t p = 0; rc == DPX_OK && wantMat && p < numPairs; p++) {
        if (H && H[p]) rc = dpx_batch_matrix(b, p, DPX_MAT_H, H[p]);
        if (rc == DPX_OK && I && I[p] && b->planes == 3) rc = dpx_batch_matrix(b, p, DPX_MAT_I, I[p]);
        if (rc == DPX_OK && D && D[p] && b->planes == 3) rc = dpx_batch_matrix(b, p, DPX_MAT_D, D[p]);
    }
    dpx_batch_destroy(b);
    return rc;
}

/* ------------------------------------------------------------------------------------------ primitives */

int dpx_prim_eval(const int32_t *op, const uint32_t *a, const uint32_t *b, const uint32_t *c, size_t count,
                  uint32_t *result, uint32_t *pred) {
    if (count && (!op || !a || !b || !c || !result || !pred)) return DPX_ERR_INVALID;
    int rc = bind_device();
    if (rc != DPX_OK) return rc;
    if (!count) return DPX_OK;
    void *d[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const size_t bytes = count * 4;
    hipError_t e = hipSuccess;
    for (int i = 0; i < 6 && e == hipSuccess; i++) e = hipMalloc(&d[i], bytes);
    if (e == hipSuccess) e = hipMemcpy(d[0], op, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d[1], a, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d[2], b, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d[3], c, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = dpx_launch_prim_eval((const int32_t *)d[0], (const uint32_t *)d[1], (const uint32_t *)d[2], (const uint32_t *)d[3],
                                 count, (uint32_t *)d[4], (uint32_t *)d[5], nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(result, d[4], bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(pred, d[5], bytes, hipMemcpyDeviceToHost);
    for (int i = 0; i < 6; i++) (void)hipFree(d[i]);
    if (e != hipSuccess) return hip_fail(e, "dpx_prim_eval");
    return DPX_OK;
}

} /* extern "C" */
