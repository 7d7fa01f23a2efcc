/* dpx_mem.h -- everything a batch allocates and what becomes of it afterwards: the matrix-pool allocator on the virtual-memory API, the
 * record of every pool, the caches that park buffers and streams between batches, and Buf, the handle through which a batch owns one
 * cached buffer.  dpx_mem.cpp needs the HIP runtime and dpx_host.cpp, no kernel unit (tests/bufcache_main.cpp runs it on the CPU). */
#ifndef DPX_MEM_H
#define DPX_MEM_H

#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "dpx_host.h"

#pragma GCC visibility push(hidden) /* (internal to libdpxalign.so: not part of its ABI) */
namespace dpx_host {

/* the matrix pool: a chunked virtual range from 64 MiB on, one hipMalloc below (dpx_mem.cpp has the reasons) */
hipError_t pool_alloc(void **out, size_t bytes);
void pool_free(void *p);
size_t pool_chunk_bytes(void *p); /* how the pool at `p` was built: chunk size of a virtual range, 0 for one hipMalloc */

/* The record of a matrix pool: how it was built and how fast hipMemset writes it (dpx_batch_describe -> bench.py's roofline.pool),
 * so that a slow run can be attributed to the pool or to something else.  Kept per pool address for the life of the pool (a
 * parked pool keeps its record for the next batch; pool_free forgets it). */
struct PoolRecord {
    std::string mode = "malloc";
    size_t bytes = 0, chunkBytes = 0;
    std::vector<float> candidatesMs; /* hipMemset time of every candidate allocation (empty: never timed) */
    std::vector<float> fillMs;       /* time of one fill of the batch on every candidate (empty: never shopped) */
    std::vector<std::string> kinds;  /* how every candidate was built: "vmm256", "malloc" ... (empty: never shopped) */
    std::vector<std::string> ranges; /* "address+bytes" of every candidate (a GPU fault address can be placed against them) */
    int kept = 0;
};
extern std::mutex g_poolRecMu;
extern std::map<void *, PoolRecord> g_poolRecords;
/* the record of a pool nobody has timed yet: how it was built (looked up by address: the pool may have been built by another thread) */
PoolRecord fresh_pool_record(void *pool, size_t bytes);

void trim_all_caches(); /* every parked stream and every buffer parked in any cache goes back to the runtime */

/* Parked buffers of one kind.  A cache is its allocator and its policy as data:
 *   take   a parked buffer of this thread's device inside [need, need + need / 2 + 1 MiB], the smallest such; for a need of at least
 *          `largeNeed` the window's roof is at least `largeRoof`.  Else a fresh allocation with 1/8 of headroom (exactly `need` from
 *          1 GiB on); after an out-of-memory everything parked anywhere is dropped and exactly `need` asked for once more.
 *   park   keeps at most maxEntries buffers and maxBytes bytes, the oldest go first; see park() for the rules on buffers of a GiB or more. */
class BufCache {
public:
    typedef hipError_t (*AllocFn)(void **out, size_t bytes);
    typedef void (*FreeFn)(void *ptr);
    BufCache(AllocFn alloc, FreeFn free, size_t largeNeed, size_t largeRoof, size_t maxEntries, size_t maxBytes);
    ~BufCache(); /* (leaves trim_all_caches' list; frees nothing: drain() does) */
    BufCache(const BufCache &) = delete;
    BufCache &operator=(const BufCache &) = delete;

    hipError_t take(void **out, size_t need, size_t *actual, bool *fresh = nullptr);
    void park(void *ptr, size_t bytes);
    void drain();

private:
    struct Entry { void *ptr; size_t bytes; int device; };
    const AllocFn alloc_;
    const FreeFn free_;
    const size_t largeNeed_, largeRoof_, maxEntries_, maxBytes_;
    std::mutex mu_;
    std::vector<Entry> parked_; /* oldest first */
    size_t total_ = 0;
    BufCache *next_ = nullptr; /* every cache alive, for trim_all_caches */
    friend void trim_all_caches();
};

/* what a batch allocates: the int16 matrices, the arena of small arrays, the traceback line buffers (device + pinned), upload images */
extern BufCache g_matCache, g_arenaCache, g_tbDevCache, g_tbHostCache, g_stageCache;

/* hipStreamCreate / hipStreamDestroy cost ~2 ms each on this stack: a finished batch parks its (idle) stream */
hipError_t stream_take(hipStream_t *out);
void stream_park(hipStream_t s);

/* One buffer of a cache, owned: taken at first use, parked when the owner goes.  Parking reads t_device, so whoever destroys the owner
 * binds the owner's device first (dpx_batch_destroy does). */
template <class T> class Buf {
public:
    explicit Buf(BufCache &cache) : cache_(&cache) {}
    Buf(Buf &&o) noexcept : cache_(o.cache_), p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    Buf &operator=(Buf &&o) noexcept {
        if (this != &o) { park(); cache_ = o.cache_; p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
        return *this;
    }
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    ~Buf() { park(); }

    T *get() const { return p_; }
    size_t cap() const { return cap_; } /* bytes; may exceed what was asked for (headroom, or a recycled buffer) */
    explicit operator bool() const { return p_ != nullptr; }

    /* taken on first use, else nothing (a failed attempt is simply repeated) */
    hipError_t ensure(size_t need, bool *fresh = nullptr) {
        if (fresh) *fresh = false;
        return p_ ? hipSuccess : take(need, fresh);
    }
    /* absent or too small: the old buffer is parked and a new one taken */
    hipError_t grow(size_t need) {
        if (p_ && cap_ >= need) return hipSuccess;
        park();
        return take(need, nullptr);
    }
    /* the buffer is the caller's now */
    T *release(size_t *cap = nullptr) {
        T *p = p_;
        if (cap) *cap = cap_;
        p_ = nullptr; cap_ = 0;
        return p;
    }
    /* a buffer of this handle's cache that was built aside replaces (and parks) the present one; nullptr: none */
    void adopt(T *p, size_t cap) { park(); p_ = p; cap_ = p ? cap : 0; }
    void park() {
        if (p_) cache_->park(p_, cap_);
        p_ = nullptr; cap_ = 0;
    }

private:
    hipError_t take(size_t need, bool *fresh) {
        void *p = nullptr;
        const hipError_t e = cache_->take(&p, need, &cap_, fresh);
        p_ = e == hipSuccess ? static_cast<T *>(p) : nullptr;
        if (!p_) cap_ = 0;
        return e;
    }
    BufCache *cache_;
    T *p_ = nullptr;
    size_t cap_ = 0;
};

} // namespace dpx_host
#pragma GCC visibility pop
#endif
