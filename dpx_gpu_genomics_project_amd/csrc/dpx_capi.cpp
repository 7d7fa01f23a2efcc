/*
 * dpx_capi.cpp -- implementation of include/dpx_align.h on the HIP runtime (host side of libdpxalign.so): device and batch life cycle, fills,
 * results and matrices.  The setters are dpx_settings.cpp's, text / CIGARs / difference strings dpx_output.cpp's; memory is dpx_mem.cpp's.
 *
 * Owns streams and launch geometry; the arithmetic is in the kernel units (dpx_kernels.hip and the other *_kernels.hip).  There is no CPU
 * fallback anywhere in the host units: without a gfx950 device every entry point fails with DPX_ERR_NO_DEVICE.
 */
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "dpx_batch.h"

static std::mutex g_mu;
static int g_device = -1; /* default device: the one dpx_init() bound (dpx_batch_create, dpx_device_info, dpx_prim_eval) */

int dpx_host::bind_device(int device) {
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

/* A z-dropped pair: the fill stopped on anti-diagonal lastDiag of the pair's dpx_extension record, and what the pool holds behind it is
 * whatever was there before.  `out`: the pair's exported plane (int16 scores or direction codes), row-major; the cells behind go to 0. */
template <class T> static hipError_t mask_behind_last_diag(const dpx_batch *b, size_t pair, T *out) {
    dpx_extension rec{};
    const hipError_t e = hipMemcpy(&rec, b->dExt.get() + pair * (sizeof rec / sizeof(int32_t)), sizeof rec, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    const dpx_pair_dev &pd = b->pairs[pair];
    if (rec.lastDiag < pd.m + pd.n)
        for (int i = 0; i <= pd.m; i++)
            for (int j = std::max(rec.lastDiag - i + 1, 0); j <= pd.n; j++) out[(size_t)i * (size_t)(pd.n + 1) + (size_t)j] = 0;
    return hipSuccess;
}

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
    const size_t bytes = b->dMat.cap();
    auto set_pool = [&](void *p) {
        (void)b->dMat.release(); /* (candidates and losers are this function's: nothing parks here) */
        b->dMat.adopt((int16_t *)p, bytes);
        b->args.mat = b->dMat.get(); b->pkArgs.mat = b->dMat.get();
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
    auto range_of = [&](void *pool) { char t[64]; snprintf(t, sizeof t, "%p+%zu", pool, bytes); return std::string(t); };
    void *best = b->dMat.get();
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
    (void)wait_for_fill(b);
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
    delete b; /* (every buffer parks itself: dpx_mem.h's Buf) */
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
        CREATE_TRY(b->arena.ensure(need));
        char *q = b->arena.get();
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
        const size_t front = (size_t)((char *)b->dTbOff - b->arena.get()) + szOff;
        if (!alphabet && front <= ((size_t)256 << 10)) {
            CREATE_TRY(b->hStage.ensure(align_up(front, (size_t)64 << 10)));
            stageBytes = front;
        }
    }
    /* host -> arena: into the image when there is one */
    auto upload = [&](void *dst, const void *src, size_t bytes) -> hipError_t {
        if (!b->hStage) return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
        memcpy(b->hStage.get() + ((char *)dst - b->arena.get()), src, bytes);
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
        CREATE_TRY(hipMemcpyAsync(b->arena.get(), b->hStage.get(), stageBytes, hipMemcpyHostToDevice, b->stream));
        b->uploadPending = true;
    }
    /* (the device, or the image, has the launch lists now; the pair table and the line offsets stay: the output path reads them) */
    b->singles = std::vector<int32_t>(); b->couples = std::vector<int32_t>(); b->waves = std::vector<dpx_wave_desc>();
    /* (a batch whose pairs are all empty has no cells, but k_traceback_wave loads the pool's first 16 bytes in place of every cell without
     * storage and masks them afterwards: such a batch gets a pool of 256 bytes, so that a.mat is an address the device may read) */
    if (b->store && (b->matElems || b->dirScratch || numPairs)) {
        bool fresh = false;
        /* DPX_POOL_GUARD=1 (tests): 4 MiB behind the matrices are filled with a pattern here and checked by dpx_batch_sync() -- a kernel that
         * writes past the end of the batch's matrices fails the test instead of hitting whatever is mapped behind the pool */
        const bool guardOn = kn.poolGuard != 0;
        b->guardBytes = guardOn ? (size_t)4 << 20 : 0;
        const size_t guardAt = b->matElems * sizeof(int16_t) + b->dirScratch;
        CREATE_TRY(b->dMat.ensure(std::max<size_t>(guardAt + b->guardBytes, 256), &fresh));
        void *const pool = b->dMat.get();
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
        if (!known) rec = fresh_pool_record(pool, b->dMat.cap());
        b->tunePool = tune && rec.candidatesMs.empty() && b->dMat.cap() >= ((size_t)1 << 30) && !b->guardBytes; /* (the memset probe would wipe the band) */
        /* (shopping for a pool nobody has shopped for yet: a fresh one, or one that dpx_pool_reserve built ahead of time) */
        b->tuneShop = b->tunePool && (fresh || rec.fillMs.empty()) && probeEnv != 1; /* DPX_POOL_PROBE=1: time only, no shopping */
        if (b->tunePool) rec.candidatesMs.assign(1, time_memset(pool, b->dMat.cap(), b->stream));
        b->poolRec = rec;
        { std::lock_guard<std::mutex> lk(g_poolRecMu); g_poolRecords[pool] = rec; }
    }
    trace.mark("create: H2D pairs+matrix pool");
#undef CREATE_TRY

    /* the plan's launch arguments get their device pointers */
    for (dpx_fill_args *x : {&b->args, &b->pkArgs}) {
        if (x == &b->pkArgs && !b->packed && !b->lanePacked) break; /* (stays zero) */
        x->seq = b->dSeq; x->pairs = b->dPairs; x->mat = b->dMat.get();
        x->score = b->dScore; x->endRow = b->dEndRow; x->endCol = b->dEndCol;
    }
    b->args.order = b->dOrder;
    if (b->packed) b->pkArgs.order = b->dCouples;
    if (b->lanePacked) b->pkArgs.waves = reinterpret_cast<const dpx_wave_desc *>(b->dCouples);
    if (b->dirs) {
        dpx_dir_args &d = b->dirArgs;
        d.seq = b->dSeq; d.pairs = b->dPairs; d.order = b->dOrder;
        d.codes = reinterpret_cast<uint8_t *>(b->dMat.get());
        d.score = b->dScore; d.endRow = b->dEndRow; d.endCol = b->dEndCol;
        d.scratch = b->dirScratch ? reinterpret_cast<unsigned char *>(b->dMat.get()) + b->matElems * sizeof(int16_t) : nullptr;
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
        g_poolRecords[b->dMat.get()] = b->poolRec;
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

static hipError_t launch_main(dpx_batch *b, const dpx_route &r, hipStream_t s) { /* the one-wave-per-pair kernel of the batch's algorithm */
    if (r.main == DPX_MAIN_LB2) { /* (DPX_LOCAL_TWO_PIECE_GAPS: k_lb2_fill with and without a table; the table's LDS as for k_bdlt_fill.  In front of
                                   * the switch: the value is declared behind dpx_main_launch's enumerator list, dpx_plan.h) */
        dpx_lb2_args xa = {b->args, {nullptr, nullptr}, b->gapOpen2, b->gapExtend2};
        if (b->substAlphabet) {
            xa.tab = table_ref(b);
            xa.f.ldsPerWave += DPX_SUBST_IMAGE_BYTES; xa.f.wavesPerBlock = dpx_plan_bdx_waves(*b, true);
        }
        return dpx_launch_lb2_fill(xa, b->R, s);
    }
    if (r.main == DPX_MAIN_BSCORE || r.main == DPX_MAIN_LSCORE) { /* (DPX_LONG_SCORES: k_bscore_fill / k_lscore_fill in every mode; the table's LDS as for
                                                                   * k_bdx_fill / k_bdlt_fill.  In front of the switch for the same reason) */
        dpx_bdx_args xa = {b->args, {nullptr, nullptr}, {r.ext ? b->zdrop : -1, r.ext ? b->endBonus : -1, b->dExt.get()}};
        if (b->substAlphabet) {
            xa.tab = table_ref(b);
            xa.f.ldsPerWave += DPX_SUBST_IMAGE_BYTES; xa.f.wavesPerBlock = dpx_plan_bdx_waves(*b, true);
        }
        return r.main == DPX_MAIN_LSCORE ? dpx_launch_lscore_fill(xa, b->R, b->prm.algo == DPX_ALGO_BASW, s) : dpx_launch_bscore_fill(xa, b->R, r.ext, s);
    }
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
        const dpx_zext_args za = {b->args, {b->zdrop, b->endBonus, b->dExt.get()}};
        return dpx_launch_zext_fill(za, b->R, b->store, b->ldsBytes, s);
    }
    case DPX_MAIN_SUBST: return dpx_launch_subst_fill(subst_args(b), b->R, b->store, r.ext, subst_lds_bytes(b), s);
    case DPX_MAIN_ZSUB: {
        const dpx_zsub_args za = {subst_args(b), {b->zdrop, b->endBonus, b->dExt.get()}};
        return dpx_launch_zsub_fill(za, b->R, b->store, subst_lds_bytes(b), s);
    }
    case DPX_MAIN_BDIR: return dpx_launch_bdir_fill(b->args, b->R, r.ext, s);
    case DPX_MAIN_BDL: return dpx_launch_bdl_fill(b->args, b->R, b->prm.algo == DPX_ALGO_BASW, s);
    case DPX_MAIN_BDLT: { /* (dpx_batch_set_local_direction_table: every wave's LDS slice grows by the image, and the workgroup may shrink to one wave) */
        dpx_subst_args ta = subst_args(b);
        ta.f.wavesPerBlock = dpx_plan_bdx_waves(*b, true);
        return dpx_launch_bdlt_fill(ta, b->R, b->prm.algo == DPX_ALGO_BASW, s);
    }
    case DPX_MAIN_BDX: { /* (dpx_batch_set_direction_scoring: with a table every wave's LDS slice grows by the image, and the workgroup may shrink to one wave) */
        dpx_bdx_args xa = {b->args, {nullptr, nullptr}, {r.ext ? b->zdrop : -1, r.ext ? b->endBonus : -1, b->dExt.get()}};
        if (b->substAlphabet) {
            xa.tab = table_ref(b);
            xa.f.ldsPerWave += DPX_SUBST_IMAGE_BYTES; xa.f.wavesPerBlock = dpx_plan_bdx_waves(*b, true);
        }
        return dpx_launch_bdx_fill(xa, b->R, r.ext, s);
    }
    case DPX_MAIN_BD2: { /* (a two-piece batch: every mode, "nothing on" included, is k_bd2_fill's; the table's LDS as for k_bdx_fill) */
        dpx_bd2_args xa = {b->args, {nullptr, nullptr}, {r.ext ? b->zdrop : -1, r.ext ? b->endBonus : -1, b->dExt.get()}, b->gapOpen2, b->gapExtend2};
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

/* the time between two events of the batch that DPX_TIME_FILLS records; !timed: they were never recorded */
static int last_usec(dpx_batch *b, bool dpx_batch::*timed, hipEvent_t dpx_batch::*e0, hipEvent_t dpx_batch::*e1, double *usec) {
    if (!b || !usec) return DPX_ERR_INVALID;
    if (!(b->*timed)) return DPX_ERR_NOT_FILLED;
    int rc = bind_device(b->device);
    if (rc != DPX_OK) return rc;
    HIP_TRY(hipEventSynchronize(b->*e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, b->*e0, b->*e1));
    *usec = (double)ms * 1000.0;
    return DPX_OK;
}
/* NOT_FILLED: no fill yet, or the batch was created without DPX_TIME_FILLS */
int dpx_batch_last_fill_usec(dpx_batch *b, double *usec) { return last_usec(b, &dpx_batch::fillTimed, &dpx_batch::evT0, &dpx_batch::evT1, usec); }
/* NOT_FILLED: no dpx_batch_output_begin() yet, or the batch was created without DPX_TIME_FILLS */
int dpx_batch_last_output_usec(dpx_batch *b, double *usec) { return last_usec(b, &dpx_batch::outTimed, &dpx_batch::evOut0, &dpx_batch::evOut1, usec); }

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
    HIP_TRY(hipMemcpy(h.data(), (const char *)b->dMat.get() + b->matElems * sizeof(int16_t) + b->dirScratch, b->guardBytes, hipMemcpyDeviceToHost));
    for (size_t k = 0; k < h.size(); k++)
        if (h[k] != 0xA5) { t_err = "DPX_POOL_GUARD: byte " + std::to_string(k) + " behind the matrices was overwritten"; return DPX_ERR_HIP; }
    return DPX_OK;
}

int dpx_batch_sync(dpx_batch *b) {
    if (!b) return DPX_ERR_INVALID;
    int rc = bind_device(b->device);
    if (rc != DPX_OK) return rc;
    HIP_TRY(wait_for_fill(b));
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
    HIP_TRY(wait_for_fill(b));
    HIP_TRY(hipStreamSynchronize(b->stream));
    const size_t bytes = b->numPairs * sizeof(int32_t);
    const size_t stride = (size_t)((const char *)b->dEndRow - (const char *)b->dScore); /* the three arrays follow each other in the arena */
    if (bytes && b->resultsCopied && b->outState != 0 && b->hMeta) { /* dpx_batch_output_begin() brought them along (small batches) */
        const char *tail = b->hMeta.get() + (b->numPairs + 1) * sizeof(uint64_t) + b->numPairs * sizeof(int32_t) + 16;
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
    if ((!b->dirs && !b->bandDirs) || b->bandScores) return DPX_ERR_NO_MATRIX; /* (DPX_LONG_SCORES: a band-direction plan without codes) */
    if (!b->filled) return DPX_ERR_NOT_FILLED;
    int rc = bind_device(b->device);
    if (rc != DPX_OK) return rc;
    const dpx_pair_dev &pd = b->pairs[pair];
    const size_t total = (size_t)(pd.m + 1) * (size_t)(pd.n + 1);
    Buf<uint8_t> dOut(g_tbDevCache); /* row-major scratch */
    HIP_TRY(wait_for_fill(b));
    HIP_TRY(dOut.ensure(std::max<size_t>(total, 16)));
    hipError_t e = (b->twoPiece && b->bandLocal) ? dpx_launch_lb2_export(reinterpret_cast<const uint8_t *>(b->dMat.get()), pd, b->dSeq, b->prm.band, which, dOut.get(), b->stream)
                   : b->twoPiece ? dpx_launch_bd2_export(reinterpret_cast<const uint8_t *>(b->dMat.get()), pd, b->dSeq, b->prm.band, which, dOut.get(), b->stream)
                   : b->bandLocal ? dpx_launch_bdl_export(reinterpret_cast<const uint8_t *>(b->dMat.get()), pd, b->dSeq, b->prm.band, which, dOut.get(), b->stream)
                   : b->bandDirs ? dpx_launch_bdir_export(reinterpret_cast<const uint8_t *>(b->dMat.get()), pd, b->dSeq, b->prm.band, which, dOut.get(), b->stream)
                                 : dpx_launch_export_dir(reinterpret_cast<const uint8_t *>(b->dMat.get()), pd, b->dSeq, b->kernelAlgo, b->R, which, dOut.get(), b->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    if (e == hipSuccess) e = hipMemcpy(out, dOut.get(), total, hipMemcpyDeviceToHost);
    dOut.park();
    if (e == hipSuccess && b->bandDirs && b->extFilled) e = mask_behind_last_diag(b, pair, out); /* (k_bdx_fill / k_bd2_fill with the scan on) */
    if (e != hipSuccess) return hip_fail(e, "dpx_batch_directions");
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
    Buf<int16_t> dOut(g_tbDevCache); /* row-major scratch */
    HIP_TRY(wait_for_fill(b));
    HIP_TRY(dOut.ensure(total * sizeof(int16_t)));
    hipError_t e = hipErrorInvalidValue;
    switch (route_of(b).exportKind) {
    case DPX_EXPORT_PLAIN: e = dpx_launch_export(b->dMat.get(), pd, b->kernelAlgo, b->R, b->planes, which, b->prm.gapOpen, b->prm.gapExtend, b->prm.band, dOut.get(), b->stream); break;
    case DPX_EXPORT_BASW: e = dpx_launch_basw_export(b->dMat.get(), pd, which, b->prm.band, dOut.get(), b->stream); break;
    case DPX_EXPORT_BANW: e = dpx_launch_banw_export(b->dMat.get(), pd, which, b->prm.band, b->prm.gapOpen, b->prm.gapExtend, dOut.get(), b->stream); break;
    }
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    if (e == hipSuccess) e = hipMemcpy(out, dOut.get(), total * sizeof(int16_t), hipMemcpyDeviceToHost);
    dOut.park();
    if (e == hipSuccess && b->extFilled) e = mask_behind_last_diag(b, pair, out); /* (k_zext_fill / k_zsub_fill) */
    if (e != hipSuccess) return hip_fail(e, "dpx_batch_matrix");
    return DPX_OK;
}


int dpx_batch_extensions(dpx_batch *b, dpx_extension *out) {
    if (!b || !out) return DPX_ERR_INVALID;
    if (!b->filled) return DPX_ERR_NOT_FILLED;
    if (!b->extFilled) return DPX_ERR_UNSUPPORTED;
    int rc = bind_device(b->device);
    if (rc != DPX_OK) return rc;
    HIP_TRY(wait_for_fill(b));
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (b->numPairs) HIP_TRY(hipMemcpy(out, b->dExt.get(), b->numPairs * sizeof(dpx_extension), hipMemcpyDeviceToHost));
    return check_guard(b);
}


int dpx_batch_describe(dpx_batch *b, char *buf, size_t cap) {
    if (!b || !buf || !cap) return DPX_ERR_INVALID;
    int len = dpx_plan_describe(*b, knobs().tbWalk, b->zdrop, b->endBonus, b->substAlphabet, buf, cap);
    if (b->revCount && len > 0 && (size_t)len < cap) /* (the two blocks are diagnostics like pool_addr: the tests overwrite them between calls) */
        len += snprintf(buf + len, cap - (size_t)len, " reversed=%zu rev_addr=0x%llx rev_bytes=%zu lines_addr=0x%llx lines_bytes=%zu", b->revCount,
                        (unsigned long long)(uintptr_t)b->dRev.get(), b->dRev.cap(), (unsigned long long)(uintptr_t)b->dTb.get(), b->dTb.cap());
    if (b->dMat && len > 0 && (size_t)len < cap) { /* the matrix pool: how it was built, and the memset time of every candidate that was timed */
        const PoolRecord &r = b->poolRec;
        len += snprintf(buf + len, cap - (size_t)len, " pool=%s pool_bytes=%zu pool_addr=0x%llx pool_chunk_mb=%zu pool_kept=%d pool_memset_ms=", r.mode.c_str(), b->dMat.cap(),
                        (unsigned long long)(uintptr_t)b->dMat.get(), r.chunkBytes >> 20, r.kept);
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
