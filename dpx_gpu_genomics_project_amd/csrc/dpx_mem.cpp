/* dpx_mem.cpp -- device and pinned memory of libdpxalign.so (dpx_mem.h): the matrix-pool allocator, the pool records, the buffer and
 * stream caches.  Needs the HIP runtime and dpx_host.cpp only. */
#include "dpx_mem.h"

#include <algorithm>
#include <cstring>

#pragma GCC visibility push(hidden) /* (the helpers below that dpx_mem.h does not declare are internal too) */
namespace dpx_host {

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

std::mutex g_poolRecMu;
std::map<void *, PoolRecord> g_poolRecords;
static void forget_pool_record(void *pool) { std::lock_guard<std::mutex> lk(g_poolRecMu); g_poolRecords.erase(pool); }
PoolRecord fresh_pool_record(void *pool, size_t bytes) {
    PoolRecord rec;
    const size_t chunk = pool_chunk_bytes(pool);
    rec.mode = chunk ? "vmm" : "malloc";
    rec.chunkBytes = chunk;
    rec.bytes = bytes;
    return rec;
}

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

/* every cache alive, newest first: what trim_all_caches drains */
static std::mutex g_cachesMu;
static BufCache *g_caches = nullptr;

BufCache::BufCache(AllocFn alloc, FreeFn free, size_t largeNeed, size_t largeRoof, size_t maxEntries, size_t maxBytes)
    : alloc_(alloc), free_(free), largeNeed_(largeNeed), largeRoof_(largeRoof), maxEntries_(maxEntries), maxBytes_(maxBytes) {
    std::lock_guard<std::mutex> lk(g_cachesMu);
    next_ = g_caches;
    g_caches = this;
}
BufCache::~BufCache() {
    std::lock_guard<std::mutex> lk(g_cachesMu);
    for (BufCache **c = &g_caches; *c; c = &(*c)->next_)
        if (*c == this) { *c = next_; break; }
}

hipError_t BufCache::take(void **out, size_t need, size_t *actual, bool *fresh) {
    if (fresh) *fresh = false;
    {
        std::lock_guard<std::mutex> lk(mu_);
        size_t best = parked_.size();
        const size_t window = need + need / 2 + (1u << 20), roof = need >= largeNeed_ ? std::max(window, largeRoof_) : window;
        for (size_t i = 0; i < parked_.size(); i++) {
            const Entry &e = parked_[i];
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
    hipError_t e = alloc_(out, want);
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        trim_all_caches();
        *actual = need;
        e = alloc_(out, need);
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
            /* per device, among the buffers of a GiB or more: one of 16 GiB or more stays alone (its arrival drops every other one, and the
             * next arrival of a GiB or more drops it); else at most eight, the arrival included, and 48 GiB of them (a pipelined driver
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
    for (void *p : evicted) free_(p);
}

void BufCache::drain() {
    std::vector<Entry> gone;
    {
        std::lock_guard<std::mutex> lk(mu_);
        gone.swap(parked_);
        total_ = 0;
    }
    for (const Entry &e : gone) free_(e.ptr);
}

static hipError_t device_alloc(void **out, size_t bytes) { return hipMalloc(out, bytes); }
static void device_free(void *p) { (void)hipFree(p); }
static hipError_t pinned_alloc(void **out, size_t bytes) { return hipHostMalloc(out, bytes, hipHostMallocDefault); }
static void pinned_free(void *p) { (void)hipHostFree(p); }

/* The three policies.  Matrix pools: a parked pool of up to 13 GiB serves any smaller batch (a driver that cuts a file into batches of one
 * pool budget ends with a short batch, and a pool reserved ahead of time -- dpx_pool_reserve -- is sized by the budget), but not a tiny
 * one: the class-per-pair drivers create thousands of batches of a few MiB, which stay on hipMalloc.  Pinned host memory: a parked
 * buffer of up to 32 MiB -- dpx_text_reserve -- serves any smaller text from 2 MiB on.  Plain device memory: the window, never wider. */
constexpr size_t MiB = (size_t)1 << 20, GiB = (size_t)1 << 30;
/* what a batch allocates: the int16 matrices, the arena of small arrays, the traceback line buffers (device + pinned) */
/*                   allocate      free         large need  its roof  entries  bytes */
BufCache g_matCache(pool_alloc, pool_free, 64 * MiB, 13 * GiB, 64, 96 * GiB);
BufCache g_arenaCache(device_alloc, device_free, 0, 0, 64, 2 * GiB);
BufCache g_tbDevCache(device_alloc, device_free, 0, 0, 64, 8 * GiB);
BufCache g_tbHostCache(pinned_alloc, pinned_free, 2 * MiB, 32 * MiB, 64, 2 * GiB);
BufCache g_stageCache(pinned_alloc, pinned_free, 2 * MiB, 32 * MiB, 64, 64 * MiB); /* upload images of small batches (dpx_batch_create: one H2D instead of five) */

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
    std::lock_guard<std::mutex> lk(g_cachesMu);
    for (BufCache *c = g_caches; c; c = c->next_) c->drain();
}

} // namespace dpx_host
#pragma GCC visibility pop
