/* bufcache_main.cpp -- the buffer caches and the owning handle of csrc/dpx_mem.h on the CPU (tests/test_bufcache_host.py builds and runs
 * this with the address and undefined-behaviour sanitizers).  The caches here stand on a fake allocator that hands out distinct addresses
 * nobody dereferences and keeps the set of live ones, so a case of 16 GiB costs nothing and a double free, or a free of an address it
 * never handed out, ends the program.  What is pinned is what the code does, rule by rule of BufCache::take and BufCache::park. */
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

#include "dpx_mem.h"

using namespace dpx_host;

static int g_checks = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        g_checks++;                                                             \
        if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); exit(1); }     \
    } while (0)

constexpr size_t KiB = (size_t)1 << 10, MiB = (size_t)1 << 20, GiB = (size_t)1 << 30;

/* ---- the fake allocator ---- */
static std::set<void *> g_live;
static std::vector<void *> g_freed;  /* in the order of the calls */
static std::vector<size_t> g_asked;  /* sizes of the calls, failed ones included */
static bool g_failNext = false;
static uintptr_t g_next = (uintptr_t)1 << 44;

static hipError_t fake_alloc(void **out, size_t bytes) {
    g_asked.push_back(bytes);
    if (g_failNext) { g_failNext = false; return hipErrorOutOfMemory; }
    *out = (void *)g_next;
    g_next += 0x10000;
    g_live.insert(*out);
    return hipSuccess;
}
static void fake_free(void *p) {
    if (!g_live.erase(p)) { printf("free of %p: not live (double free, or never allocated)\n", p); exit(1); }
    g_freed.push_back(p);
}
static void *fake_buffer() { void *p = nullptr; (void)fake_alloc(&p, 0); return p; } /* an address to park under any size */
static bool live(void *p) { return g_live.count(p) != 0; }

struct Got { void *p; size_t cap; bool fresh; hipError_t e; };
static Got take(BufCache &c, size_t need) {
    Got g{nullptr, 0, false, hipSuccess};
    g.e = c.take(&g.p, need, &g.cap, &g.fresh);
    return g;
}
/* the three policies of dpx_mem.cpp, on the fake allocator; `entries` / `bytes`: the park limits */
static const size_t kNoLimit = (size_t)1 << 50;
#define PLAIN(name, entries, bytes) BufCache name(fake_alloc, fake_free, 0, 0, entries, bytes)
#define POOL(name, entries, bytes) BufCache name(fake_alloc, fake_free, 64 * MiB, 13 * GiB, entries, bytes)
#define PINNED(name, entries, bytes) BufCache name(fake_alloc, fake_free, 2 * MiB, 32 * MiB, entries, bytes)

static void nothing_parked() {
    PLAIN(c, 64, kNoLimit);
    for (const size_t need : {(size_t)1, (size_t)100000, 64 * KiB, 7 * MiB + 3, GiB - 1}) {
        const Got g = take(c, need);
        CHECK(g.e == hipSuccess && g.fresh && live(g.p));
        CHECK(g.cap == align_up(need + need / 8, 64 * KiB) && g_asked.back() == g.cap);
        fake_free(g.p);
    }
    for (const size_t need : {GiB, GiB + 1, 22 * GiB + 12345}) { /* from 1 GiB on: exactly what was asked for */
        const Got g = take(c, need);
        CHECK(g.e == hipSuccess && g.fresh && g.cap == need && g_asked.back() == need);
        fake_free(g.p);
    }
}

static void best_fit() {
    PLAIN(c, 64, kNoLimit);
    const size_t need = 10 * MiB, roof = need + need / 2 + MiB;
    void *a = fake_buffer(), *b = fake_buffer(), *over = fake_buffer(), *under = fake_buffer();
    c.park(a, 14 * MiB);
    c.park(b, 12 * MiB);
    c.park(over, roof + 1);
    c.park(under, need - 1);
    Got g = take(c, need);
    CHECK(g.p == b && g.cap == 12 * MiB && !g.fresh); /* the smaller of the two inside the window */
    g = take(c, need);
    CHECK(g.p == a && g.cap == 14 * MiB && !g.fresh);
    g = take(c, need);
    CHECK(g.fresh && g.p != over && g.p != under); /* just above the roof, just below the need: not taken */
    fake_free(g.p);
    c.park(a, roof); /* the window's two ends are inside */
    g = take(c, need);
    CHECK(g.p == a && !g.fresh);
    c.park(b, need);
    g = take(c, need);
    CHECK(g.p == b && !g.fresh);
    /* of two equal ones the older */
    c.park(a, 11 * MiB);
    c.park(b, 11 * MiB);
    g = take(c, need);
    CHECK(g.p == a);
    g = take(c, roof + 1); /* (`over` serves a need of its own size) */
    CHECK(g.p == over && !g.fresh);
    fake_free(a); fake_free(over);
    c.drain();
    CHECK(!live(b) && !live(under));
}

static void large_need_roofs() {
    {
        POOL(c, 64, kNoLimit);
        void *p = fake_buffer(), *q = fake_buffer();
        c.park(p, 13 * GiB);
        Got g = take(c, 64 * MiB - 1); /* a small need keeps the window */
        CHECK(g.fresh);
        fake_free(g.p);
        g = take(c, 64 * MiB);
        CHECK(g.p == p && g.cap == 13 * GiB && !g.fresh);
        c.park(q, 13 * GiB + 1);
        g = take(c, 64 * MiB);
        CHECK(g.fresh);
        fake_free(g.p);
        g = take(c, 10 * GiB); /* the window where it is wider than the roof: 10 + 5 GiB + 1 MiB */
        CHECK(g.p == q && !g.fresh);
        c.park(q, 15 * GiB + MiB + 1);
        g = take(c, 10 * GiB);
        CHECK(g.fresh);
        fake_free(g.p); fake_free(p);
        c.drain();
    }
    {
        PINNED(c, 64, kNoLimit);
        void *p = fake_buffer(), *q = fake_buffer();
        c.park(p, 32 * MiB);
        Got g = take(c, 2 * MiB - 1);
        CHECK(g.fresh);
        fake_free(g.p);
        g = take(c, 2 * MiB);
        CHECK(g.p == p && !g.fresh);
        c.park(q, 32 * MiB + 1);
        g = take(c, 2 * MiB);
        CHECK(g.fresh);
        fake_free(g.p);
        g = take(c, 40 * MiB); /* window 61 MiB */
        CHECK(g.fresh);
        fake_free(g.p);
        g = take(c, 30 * MiB); /* window 46 MiB */
        CHECK(g.p == q && !g.fresh);
        fake_free(p); fake_free(q);
    }
    {
        PLAIN(c, 64, kNoLimit);
        void *p = fake_buffer(), *q = fake_buffer();
        c.park(p, 13 * GiB);
        c.park(q, 32 * MiB);
        Got g = take(c, 64 * MiB);
        CHECK(g.fresh);
        fake_free(g.p);
        g = take(c, 2 * MiB);
        CHECK(g.fresh);
        fake_free(g.p);
        c.drain();
        CHECK(!live(p) && !live(q));
    }
}

static void other_device() {
    PLAIN(c, 64, kNoLimit);
    void *p = fake_buffer();
    t_device = 0;
    c.park(p, MiB);
    t_device = 1;
    Got g = take(c, MiB);
    CHECK(g.fresh && g.p != p);
    fake_free(g.p);
    t_device = 0;
    g = take(c, MiB);
    CHECK(g.p == p && !g.fresh);
    fake_free(p);
}

static void park_limits() {
    {
        PLAIN(c, 64, kNoLimit);
        std::vector<void *> v;
        for (int k = 0; k < 65; k++) v.push_back(fake_buffer());
        g_freed.clear();
        for (int k = 0; k < 64; k++) c.park(v[(size_t)k], 4 * KiB);
        CHECK(g_freed.empty());
        c.park(v[64], 4 * KiB); /* the 65th: the oldest goes */
        CHECK(g_freed.size() == 1 && g_freed[0] == v[0]);
        c.drain();
        CHECK(g_freed.size() == 65);
    }
    {
        PLAIN(c, 64, 10 * MiB);
        void *a = fake_buffer(), *b = fake_buffer(), *d = fake_buffer(), *e = fake_buffer(), *f = fake_buffer(), *g = fake_buffer();
        g_freed.clear();
        c.park(a, 4 * MiB);
        c.park(b, 4 * MiB);
        CHECK(g_freed.empty());
        c.park(d, 4 * MiB); /* 12 MiB: the oldest goes */
        CHECK(g_freed.size() == 1 && g_freed[0] == a);
        c.park(e, 9 * MiB); /* ... the two oldest, oldest first */
        CHECK(g_freed.size() == 3 && g_freed[1] == b && g_freed[2] == d);
        c.park(f, 10 * MiB + 1); /* larger than the cache may hold: freed at once, nothing else touched */
        CHECK(g_freed.size() == 4 && g_freed[3] == f && live(e));
        t_device = -1;
        c.park(g, KiB); /* no device bound: freed at once */
        CHECK(g_freed.size() == 5 && g_freed[4] == g);
        t_device = 0;
        c.park(nullptr, KiB); /* nothing */
        const Got got = take(c, 9 * MiB);
        CHECK(got.p == e && !got.fresh);
        fake_free(e);
    }
}

/* buffers of a GiB or more, per device: today's loop in BufCache::park, replayed */
static void gib_rules() {
    { /* an arrival of 16 GiB: every parked buffer of a GiB or more of this device goes, newest first; smaller ones and other devices' stay */
        POOL(c, 64, kNoLimit);
        void *far = fake_buffer(), *a = fake_buffer(), *b = fake_buffer(), *s = fake_buffer(), *h = fake_buffer(), *n = fake_buffer(), *t = fake_buffer();
        t_device = 1;
        c.park(far, 2 * GiB);
        t_device = 0;
        c.park(a, GiB);
        c.park(b, 2 * GiB);
        c.park(s, 512 * MiB);
        g_freed.clear();
        c.park(h, 16 * GiB);
        CHECK(g_freed.size() == 2 && g_freed[0] == b && g_freed[1] == a && live(s) && live(far) && live(h));
        c.park(t, GiB - 1); /* an arrival below a GiB drops nothing */
        CHECK(g_freed.size() == 2);
        c.park(n, GiB); /* an arrival of a GiB: a parked one of 16 GiB goes */
        CHECK(g_freed.size() == 3 && g_freed[2] == h && live(n) && live(s) && live(t));
        c.drain();
        CHECK(g_live.empty());
    }
    { /* the ninth of a GiB or more: the oldest goes, eight stay */
        POOL(c, 64, kNoLimit);
        std::vector<void *> v;
        for (int k = 0; k < 10; k++) v.push_back(fake_buffer());
        g_freed.clear();
        for (int k = 0; k < 8; k++) c.park(v[(size_t)k], GiB + (size_t)k);
        CHECK(g_freed.empty());
        c.park(v[8], GiB);
        CHECK(g_freed.size() == 1 && g_freed[0] == v[0]);
        c.park(v[9], 3 * GiB);
        CHECK(g_freed.size() == 2 && g_freed[1] == v[1]);
        c.drain();
        CHECK(g_live.empty());
    }
    { /* 48 GiB of them, the arrival included: what lies behind the sum's crossing goes */
        POOL(c, 64, kNoLimit);
        std::vector<void *> v;
        for (int k = 0; k < 6; k++) v.push_back(fake_buffer());
        g_freed.clear();
        for (int k = 0; k < 4; k++) c.park(v[(size_t)k], 10 * GiB);
        CHECK(g_freed.empty()); /* 40 GiB */
        c.park(v[4], 10 * GiB); /* 10 + 30 = 40 with the three newest, 50 with the oldest */
        CHECK(g_freed.size() == 1 && g_freed[0] == v[0]);
        c.park(v[5], 8 * GiB + 1); /* 8 + 40 GiB + 1 crosses at the oldest of the four */
        CHECK(g_freed.size() == 2 && g_freed[1] == v[1]);
        c.drain();
        CHECK(g_live.empty());
    }
}

static void out_of_memory() {
    PLAIN(c, 64, kNoLimit);
    PINNED(other, 64, kNoLimit);
    void *a = fake_buffer(), *b = fake_buffer(), *far = fake_buffer();
    c.park(a, KiB);
    other.park(b, MiB);
    t_device = 1;
    c.park(far, MiB);
    t_device = 0;
    const size_t need = 3 * MiB + 17;
    g_asked.clear();
    g_failNext = true;
    const Got g = take(c, need);
    CHECK(g.e == hipSuccess && g.fresh && g.cap == need); /* the retry asks for exactly the need */
    CHECK(g_asked.size() == 2 && g_asked[0] == align_up(need + need / 8, 64 * KiB) && g_asked[1] == need);
    CHECK(!live(a) && !live(b) && !live(far)); /* everything parked in every cache was dropped */
    fake_free(g.p);
    /* a second failure is the caller's */
    g_failNext = true;
    Got g2 = take(c, GiB);
    CHECK(g2.e == hipSuccess && g2.cap == GiB); /* (one failure, one retry) */
    fake_free(g2.p);
    CHECK(g_live.empty());
}

static void drain_frees_once() {
    PLAIN(c, 64, kNoLimit);
    void *a = fake_buffer(), *b = fake_buffer(), *d = fake_buffer();
    c.park(a, KiB); c.park(b, MiB); c.park(d, GiB);
    g_freed.clear();
    c.drain();
    CHECK(g_freed.size() == 3 && !live(a) && !live(b) && !live(d));
    c.drain();
    CHECK(g_freed.size() == 3);
    const Got g = take(c, KiB);
    CHECK(g.fresh);
    fake_free(g.p);
}

static void handle() {
    PLAIN(c, 64, kNoLimit);
    {
        Buf<uint32_t> h(c);
        CHECK(!h && h.get() == nullptr && h.cap() == 0);
        g_asked.clear();
        bool fresh = false;
        CHECK(h.ensure(MiB, &fresh) == hipSuccess && fresh && h && h.cap() == align_up(MiB + MiB / 8, 64 * KiB));
        uint32_t *first = h.get();
        CHECK(h.ensure(MiB, &fresh) == hipSuccess && !fresh && h.get() == first && g_asked.size() == 1); /* ensure twice: one allocation */
        CHECK(h.grow(MiB + 1) == hipSuccess && h.get() == first && g_asked.size() == 1);                  /* large enough: nothing */
        /* grow parks the old buffer BEFORE it takes the new one: an allocation that fails once finds it parked and drops it */
        g_failNext = true;
        CHECK(h.grow(4 * MiB) == hipSuccess && h.get() != first && h.cap() == 4 * MiB && !live(first));
        /* ... and without a failure the old one is in the cache afterwards */
        uint32_t *second = h.get();
        CHECK(h.grow(8 * MiB) == hipSuccess && h.get() != second && live(second));
        Buf<uint32_t> other(c);
        CHECK(other.ensure(4 * MiB) == hipSuccess && other.get() == second && other.cap() == 4 * MiB);
        /* a failed take leaves the handle empty, and the attempt is simply repeated */
        Buf<char> late(c);
        g_failNext = true;
        g_asked.clear();
        hipError_t e = late.ensure(64 * MiB);
        CHECK(e == hipSuccess && g_asked.size() == 2); /* (the cache's own retry) */
        late.park();
        CHECK(!late && late.cap() == 0);
    } /* h, other: parked here */
    {
        const Got g = take(c, 8 * MiB);
        CHECK(!g.fresh);
        c.park(g.p, g.cap);
    }
    c.drain();
    CHECK(g_live.empty());
    { /* release leaves nothing to park: the buffer is the caller's (dpx_batch_output_take -> dpx_text_free) */
        size_t cap = 0;
        char *p = nullptr;
        {
            Buf<char> h(c);
            CHECK(h.ensure(100) == hipSuccess);
            p = h.release(&cap);
            CHECK(p && cap == 64 * KiB && !h && h.cap() == 0);
        }
        c.drain();
        CHECK(live(p));
        c.park(p, cap);
        c.drain();
        CHECK(g_live.empty());
    }
    { /* adopt parks what it replaces */
        Buf<char> h(c), aside(c);
        CHECK(h.ensure(MiB) == hipSuccess && aside.ensure(3 * MiB) == hipSuccess);
        char *old = h.get(), *built = aside.get();
        size_t cap = 0;
        char *p = aside.release(&cap);
        h.adopt(p, cap);
        CHECK(h.get() == built && h.cap() == cap);
        const Got g = take(c, MiB);
        CHECK(g.p == old && !g.fresh);
        c.park(g.p, g.cap);
        h.adopt(nullptr, 123); /* (no mask any more: the handle is empty) */
        CHECK(!h && h.cap() == 0);
    }
    { /* a moved-from handle parks nothing: were it to, drain would free the address twice */
        Buf<char> a(c);
        CHECK(a.ensure(MiB) == hipSuccess);
        char *p = a.get();
        Buf<char> b(std::move(a));
        CHECK(!a && a.cap() == 0 && b.get() == p);
        Buf<char> d(c);
        CHECK(d.ensure(2 * MiB) == hipSuccess);
        char *q = d.get();
        d = std::move(b); /* (parks q, owns p) */
        CHECK(!b && d.get() == p && live(q));
    }
    c.drain();
    CHECK(g_live.empty()); /* every address was parked or freed exactly once */
}

int main() {
    t_device = 0;
    nothing_parked();
    best_fit();
    large_need_roofs();
    other_device();
    park_limits();
    gib_rules();
    out_of_memory();
    drain_frees_once();
    handle();
    CHECK(g_live.empty());
    printf("ok %d checks\n", g_checks);
    return 0;
}
