// capi.hip -- implementation of include/rustybam_amd.h (host side, HIP runtime).
//
// No CPU fallback lives here: every compute entry point needs a gfx950 device and fails with
// RB_E_NO_DEVICE otherwise.  Nothing in this file (or this library) touches oracle/.
#include <hip/hip_runtime.h>
#include <sys/mman.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <numeric>
#include <string>
#include <thread>
#include <vector>
#include <chrono>
#include <map>
#include <mutex>

#include "../../include/rustybam_amd.h"
#include "rb_lift.h" // rb_lift_params (the device helpers in it are unused here)
#include "rb_trim.h" // rb_trim_params
#include "rb_launch.h" // the other kernels' parameter blocks and launchers

#ifndef RB_SCAN_ROWS_MEAN_MAX
#define RB_SCAN_ROWS_MEAN_MAX 1536 // ops per record, batch mean, up to which rb_dev_scan_records takes the row form (k_records.hip)
#endif
#ifndef RB_SHORT_MAX_DEFAULT
#define RB_SHORT_MAX_DEFAULT 2048 // records of up to this many ops go through the tile kernel (profiles/r05_reclen_summary.md)
#endif

#define RB_MAX_ARENA 256

#define RB_TIMING_RING 256
// Filling device memory is done by a kernel of the library (plain 16-byte stores; the runtime's hipMemsetAsync is a kernel too).
// Round 4 wrote it while hunting a fill that "ran" and changed nothing; the cause turned out to be elsewhere -- a virtual range
// given back and taken again, rb_free_vmm -- and the kernel stayed: one code path less that is not the library's own.
__global__ __launch_bounds__(256) void rb_k_fill_bytes(uint8_t *dst, uint32_t v4, size_t n) {
    const uintptr_t a = (uintptr_t)dst;
    const size_t head = n < 16 ? n : (size_t)((16 - (a & 15)) & 15); // bytes in front of the first 16-byte boundary
    const size_t body = (n - head) / 16;                             // whole 16-byte groups
    const size_t tail0 = head + body * 16;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t k = i; k < body; k += stride) *reinterpret_cast<uint4 *>(dst + head + k * 16) = make_uint4(v4, v4, v4, v4);
    if (i < head) dst[i] = (uint8_t)v4;
    if (i < n - tail0) dst[tail0 + i] = (uint8_t)v4;
}
extern "C" hipError_t rb_fill_async(void *dst, int value, size_t bytes, hipStream_t stream) {
    if (!bytes) return hipSuccess;
    const uint32_t b = (uint32_t)value & 255u, v4 = b | (b << 8) | (b << 16) | (b << 24);
    const size_t groups = bytes / 16 + 1;
    const unsigned blocks = (unsigned)std::min<size_t>((groups + 255) / 256, 65536);
    hipLaunchKernelGGL(rb_k_fill_bytes, dim3(blocks ? blocks : 1), dim3(256), 0, stream, (uint8_t *)dst, v4, bytes);
    return hipGetLastError();
}

struct rb_ctx {
    int device = -1;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    // optional HIP-event timing of the dominant (streaming) kernel of each liftover/break call
    bool timing = false;
    std::vector<hipEvent_t> ev_a, ev_b;
    uint64_t timed_calls = 0;
    // liftover: the stream the tile kernel runs on beside the per-record kernel (lift_common), and the two events that tie it to `stream`
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // trim-paf: slabs of device memory for pairs whose overlap region does not fit LDS (allocated at the first rb_dev_overlap_split)
    void *trim_scratch = nullptr;
    uint32_t trim_scratch_blocks = 0;
    void *trim_pend = nullptr; // [count (256 B) | indices of the pairs the first wave kernel declined]
    uint64_t trim_pend_cap = 0;
    void *scan_list = nullptr; // [count (256 B) | indices of the records the row form of the scan left to the wave-per-record kernel]
    uint64_t scan_list_cap = 0;
    uint64_t scan_rows_n = 0; // records of the last rb_dev_scan_records call if it took the row form, 0 if not (rb_ctx_scan_route)
    // pinned staging ring of the host-buffer entry points (rb_dev_upload / rb_dev_download): large transfers go through two
    // page-locked chunks (hipHostMalloc), the copy into / out of a chunk on several host threads while the DMA of the other runs
    void *pin[2] = {nullptr, nullptr};
    hipEvent_t pin_ev[2] = {nullptr, nullptr};
    bool pin_busy[2] = {false, false};
    unsigned pin_next = 0; // the slot the next upload chunk takes
    uint64_t alloc_fallbacks = 0; // rb_dev_alloc requests that wanted the chunked route and got plain hipMalloc
    // buffers given back with rb_dev_release: still mapped (a chunked buffer keeps its physical pages, hence its placement), handed out
    // again by the next rb_dev_alloc / rb_dev_alloc_placed of the same size on this context
    struct cached_buf { void *p; size_t bytes; bool placed; };
    std::vector<cached_buf> cache;
    size_t cache_bytes = 0;
};
#define RB_PIN_CHUNK ((size_t)32 << 20)
#define RB_PIN_MIN ((size_t)8 << 20) // (round 3: smaller transfers took the runtime's own pageable path; round 4: nothing does, rb_dev_upload says why)

struct rb_plan {
    rb_ctx *ctx = nullptr;
    uint64_t n_rec = 0, n_win = 0, n_ops = 0;
    uint32_t n_contig = 0;
    uint32_t depth = 0; // most windows of a sorted per-contig window list that overlap at one point (0: no sorted list)
    // device arrays
    uint32_t *sched = nullptr, *slot_of = nullptr, *canon_pos = nullptr, *w_orig = nullptr, *ident = nullptr;
    uint64_t *w_st = nullptr, *w_en = nullptr, *wo_st = nullptr, *wo_en = nullptr, *cw_off = nullptr;
    uint8_t *cw_mono = nullptr;
    // short records (k_tile.hip): tiles of consecutive records, three words each {first record | passthrough << 31, records, schedule slot of
    // the first record}; the schedule's slots [0, stream_end) hold the records longer than the tiles take, longest first, the others follow in memory order
    uint32_t *tiles = nullptr;
    uint32_t n_tiles = 0, stream_end = 0;
};

static int fail(rb_ctx *ctx, int code, const char *fmt, ...) {
    if (ctx) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        ctx->err = buf;
    }
    return code;
}
#define HIPCHK(ctx, call)                                                                             \
    do {                                                                                              \
        hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess) return fail((ctx), RB_E_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)

extern "C" int rb_abi_version(void) { return RB_ABI_VERSION; }

extern "C" int rb_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int rb_ctx_create(int device, void *hip_stream, rb_ctx **out) {
    if (!out) return RB_E_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return RB_E_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return RB_E_NO_DEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        fprintf(stderr, "rustybam_amd: device %d is %s; this library only carries gfx950 (MI355X) code objects\n", device, prop.gcnArchName);
        return RB_E_NO_DEVICE;
    }
    if (hipSetDevice(device) != hipSuccess) return RB_E_NO_DEVICE;
    rb_ctx *c = new rb_ctx();
    c->device = device;
    if (hip_stream) {
        c->stream = (hipStream_t)hip_stream;
    } else {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
            delete c;
            return RB_E_HIP;
        }
        c->own_stream = true;
    }
    // the side stream at the lowest priority: its waves go where a wave of the main stream's kernel does not fit, and take no place
    // from one (profiles/tile_beside_summary.md has normal priority beside it)
    int prio_least = 0, prio_greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) != hipSuccess ||
        hipStreamCreateWithPriority(&c->side, hipStreamNonBlocking, prio_least) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        rb_ctx_destroy(c);
        return RB_E_HIP;
    }
    *out = c;
    return RB_OK;
}
extern "C" void rb_ctx_destroy(rb_ctx *ctx) {
    if (!ctx) return;
    if (ctx->side) {
        (void)hipStreamSynchronize(ctx->side); // (what it still runs writes the caller's buffers)
        hipStreamDestroy(ctx->side);
    }
    if (ctx->ev_fork) hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) hipEventDestroy(ctx->ev_join);
    for (auto e : ctx->ev_a) hipEventDestroy(e);
    for (auto e : ctx->ev_b) hipEventDestroy(e);
    for (int k = 0; k < 2; k++) {
        if (ctx->pin[k]) hipHostFree(ctx->pin[k]);
        if (ctx->pin_ev[k]) hipEventDestroy(ctx->pin_ev[k]);
    }
    if (ctx->trim_scratch) hipFree(ctx->trim_scratch);
    if (ctx->trim_pend) hipFree(ctx->trim_pend);
    if (ctx->scan_list) hipFree(ctx->scan_list);
    (void)rb_dev_cache_trim(ctx, 0);
    if (ctx->own_stream) hipStreamDestroy(ctx->stream);
    delete ctx;
}
extern "C" const char *rb_ctx_last_error(const rb_ctx *ctx) { return ctx ? ctx->err.c_str() : "no context"; }
extern "C" int rb_ctx_sync(rb_ctx *ctx) {
    if (!ctx) return RB_E_INVALID;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RB_OK;
}
extern "C" void *rb_ctx_stream(rb_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

extern "C" int rb_ctx_set_timing(rb_ctx *ctx, int enabled) {
    if (!ctx) return RB_E_INVALID;
    if (enabled && ctx->ev_a.empty()) {
        ctx->ev_a.resize(RB_TIMING_RING);
        ctx->ev_b.resize(RB_TIMING_RING);
        for (int i = 0; i < RB_TIMING_RING; i++) {
            HIPCHK(ctx, hipEventCreate(&ctx->ev_a[i]));
            HIPCHK(ctx, hipEventCreate(&ctx->ev_b[i]));
        }
    }
    ctx->timing = enabled != 0;
    ctx->timed_calls = 0;
    return RB_OK;
}
extern "C" int rb_ctx_get_timing(rb_ctx *ctx, double *ms_out, int cap, int *n_out) {
    if (!ctx || !ms_out || !n_out) return RB_E_INVALID;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const uint64_t have = ctx->timed_calls < RB_TIMING_RING ? ctx->timed_calls : RB_TIMING_RING;
    int n = 0;
    for (uint64_t k = 0; k < have && n < cap; k++) {
        const uint64_t call = ctx->timed_calls - have + k;
        const size_t slot = (size_t)(call % RB_TIMING_RING);
        float ms = 0;
        HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ev_a[slot], ctx->ev_b[slot]));
        ms_out[n++] = ms;
    }
    *n_out = n;
    return RB_OK;
}

// A large buffer as separately created 2 MB physical chunks (hipMemCreate) mapped into one virtual range, in the order they were
// created or (RB_ALLOC_MODE=scatter) in a pseudo-random one; rb_dev_free unmaps and releases them (rb_dev_alloc says why).
struct rb_vmm_alloc {
    size_t bytes, chunk;
    std::vector<hipMemGenericAllocationHandle_t> handles;
    bool placed = false; // chosen among candidates by measurement (rb_dev_alloc_placed[_by])
};
static std::map<void *, rb_vmm_alloc> g_vmm;
static std::mutex g_vmm_mu;
// Virtual address space: a freed chunked buffer's range is never given back to the driver (rb_free_vmm says why), so every chunked
// allocation that is FREED costs its size in address space for the life of the process.  Counted, and capped: beyond the cap (default
// 32 TB of the 128 TB a process has, RB_ALLOC_VA_CAP_GB) the chunked route is refused and rb_dev_alloc falls back to plain hipMalloc
// (rb_dev_alloc_mode / rb_dev_alloc_stats say so).  A host that recycles its buffers with rb_dev_release instead of rb_dev_free retires
// nothing.
static size_t g_va_live = 0, g_va_retired = 0; // (under g_vmm_mu)
static std::map<void *, size_t> g_asked;        // (under g_vmm_mu) what rb_dev_alloc was asked for, rounded to 256: buffers of 1 MB and more (the ones rb_dev_release keeps)
static size_t rb_va_cap() { // (read per call: tests move it)
    const char *e = getenv("RB_ALLOC_VA_CAP_GB");
    return (size_t)(e ? strtoull(e, nullptr, 10) : 32768ull) << 30;
}
// -> 0: not one of ours; 1: released; -1: a HIP call failed (*err names it; the pieces that could be given back have been)
static int rb_free_vmm(void *p, int device, hipError_t *err) {
    std::lock_guard<std::mutex> lk(g_vmm_mu);
    auto it = g_vmm.find(p);
    if (it == g_vmm.end()) return 0;
    hipError_t first = hipSuccess;
    auto note = [&](hipError_t e) {
        if (e != hipSuccess && first == hipSuccess) first = e;
    };
    note(hipSetDevice(device));       // (the buffer's device, not whatever is current: kernels on it must have drained)
    note(hipDeviceSynchronize());
    // every chunk is a mapping of its own: HIP promises the unmapping of whole mappings, not of a range that spans several
    const size_t chunk = it->second.chunk, n = it->second.handles.size();
    for (size_t k = 0; k < n; k++) note(hipMemUnmap((char *)p + k * chunk, chunk));
    for (auto &h : it->second.handles) note(hipMemRelease(h));
    // The virtual range is NOT given back (hipMemAddressFree): a later reservation would get it again, and a kernel's stores into a
    // buffer mapped at addresses this process had mapped before went to the OLD physical pages -- a fill kernel that "ran" and changed
    // nothing that three different readers could see (tools/alloc_probe2.py: a 300 MB buffer taken right after a 1 GB one was freed;
    // copies, which do not go through the compute units' translation caches, read and wrote the new pages).  Addresses are not
    // scarce (a batch of 75 GB takes 2^-11 of the 47-bit range); memory is what is returned, chunk by chunk, above.
    g_va_live -= it->second.bytes;
    g_va_retired += it->second.bytes;
    g_vmm.erase(it);
    if (first != hipSuccess) (void)hipGetLastError();
    *err = first;
    return first == hipSuccess ? 1 : -1;
}
static void *rb_alloc_vmm(int device, size_t bytes, bool shuffle) {
    hipMemAllocationProp prop;
    memset(&prop, 0, sizeof prop);
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = device;
    size_t gran = 0;
    if (hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityMinimum) != hipSuccess || !gran) return nullptr;
    // (2 MB: chunks of 4 MB measured 2 % slower, and with 8 MB and 32 MB chunks the first kernel on the buffer took a memory access
    //  fault on this ROCm -- not understood, not used)
    size_t chunk = (size_t)2 << 20;
    chunk = (chunk + gran - 1) / gran * gran;
    const size_t n = (bytes + chunk - 1) / chunk;
    {
        std::lock_guard<std::mutex> lk(g_vmm_mu);
        if (g_va_live + g_va_retired + n * chunk > rb_va_cap()) return nullptr; // (address space used up by freed buffers: the caller takes plain hipMalloc)
    }
    void *va = nullptr;
    if (hipMemAddressReserve(&va, n * chunk, 0, nullptr, 0) != hipSuccess || !va) return nullptr;
    std::vector<hipMemGenericAllocationHandle_t> h;
    h.reserve(n);
    size_t mapped = 0;
    bool ok = true;
    for (size_t k = 0; k < n && ok; k++) {
        hipMemGenericAllocationHandle_t hk;
        ok = hipMemCreate(&hk, chunk, &prop, 0) == hipSuccess;
        if (ok) h.push_back(hk);
    }
    std::vector<size_t> order(n);
    for (size_t k = 0; k < n; k++) order[k] = k;
    if (shuffle) {
        uint64_t x = 0x9E3779B97F4A7C15ull;
        for (size_t k = n; k > 1; k--) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            std::swap(order[k - 1], order[(size_t)(x % k)]);
        }
    }
    for (size_t k = 0; k < n && ok; k++) {
        ok = hipMemMap((char *)va + k * chunk, chunk, 0, h[order[k]], 0) == hipSuccess;
        if (ok) mapped = k + 1;
    }
    if (ok) {
        hipMemAccessDesc acc;
        memset(&acc, 0, sizeof acc);
        acc.location = prop.location;
        acc.flags = hipMemAccessFlagsProtReadWrite;
        ok = hipMemSetAccess(va, n * chunk, &acc, 1) == hipSuccess;
    }
    if (!ok) { // give everything back: the caller falls back to hipMalloc
        (void)hipGetLastError();
        for (size_t k = 0; k < mapped; k++) (void)hipMemUnmap((char *)va + k * chunk, chunk);
        for (auto &hk : h) (void)hipMemRelease(hk);
        (void)hipMemAddressFree(va, n * chunk);
        return nullptr;
    }
    {
        std::lock_guard<std::mutex> lk(g_vmm_mu);
        g_vmm[va] = rb_vmm_alloc{n * chunk, chunk, h};
        g_va_live += n * chunk;
    }
    return va;
}
extern "C" int rb_dev_alloc(rb_ctx *ctx, size_t bytes, void **dev_ptr) {
    if (!ctx || !dev_ptr) return RB_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t want = bytes ? ((bytes + 255) & ~(size_t)255) : 256;
    // How a large buffer is pieced together physically decides the streaming kernels' time: the same clip kernel on the same virtual
    // addresses takes 10.2-11.9 ms in plain hipMalloc memory depending on the allocation (tools/layout_probe.py), 18-20 ms in
    // physically contiguous memory (hipDeviceMallocContiguous), and 9.4 ms -- every time -- when the buffer is made of separately
    // created 2 MB physical chunks mapped side by side (hipMemCreate / hipMemMap; tools/contig_probe.py, round 3).  So requests of
    // 1 GB and more -- a resident batch and its outputs -- are built that way (about 14 us per chunk: 1 s for 75 GB, once per batch);
    // smaller ones, and everything under RB_ALLOC_MODE=default, come from hipMalloc.  RB_ALLOC_MODE=chunks / scatter (the chunks in
    // pseudo-random order: no different) / contiguous force a mode for the probe.
    for (size_t k = 0; k < ctx->cache.size(); k++) // a buffer this context released, of this very size: as it is (still mapped, its pages its own)
        if (ctx->cache[k].bytes == want) {
            *dev_ptr = ctx->cache[k].p;
            ctx->cache_bytes -= want;
            ctx->cache.erase(ctx->cache.begin() + (long)k);
            return RB_OK;
        }
    const char *mode = getenv("RB_ALLOC_MODE");
    // (round 4: from 256 MB up, not 1 GB -- the row arena of the headline batch, 1.02e9 bytes, fell just short of the old threshold and sat
    //  in plain hipMalloc memory beside a chunked batch)
    const size_t chunk_min = (size_t)256 << 20;
    const bool chunks = mode ? (!strcmp(mode, "scatter") || !strcmp(mode, "chunks")) : want >= chunk_min;
    if (want >= ((size_t)64 << 20) && chunks) {
        void *q = rb_alloc_vmm(ctx->device, want, mode && !strcmp(mode, "scatter"));
        if (q) {
            *dev_ptr = q;
            std::lock_guard<std::mutex> lk(g_vmm_mu);
            g_asked[q] = want;
            return RB_OK;
        }
        const hipError_t why = hipGetLastError();
        ctx->alloc_fallbacks++; // (rb_dev_alloc_mode tells the caller which route a buffer took: the two differ by 10-20 % in the clip kernel's time)
        if (getenv("RB_ALLOC_LOG")) fprintf(stderr, "[rb_dev_alloc] %zu bytes: the chunked route failed (%s), plain hipMalloc instead\n", want, hipGetErrorString(why));
    }
    auto remember = [&]() {
        if (want >= ((size_t)1 << 20)) {
            std::lock_guard<std::mutex> lk(g_vmm_mu);
            g_asked[*dev_ptr] = want;
        }
    };
    if (want >= ((size_t)64 << 20) && mode && !strcmp(mode, "contiguous")) {
        if (hipExtMallocWithFlags(dev_ptr, want, hipDeviceMallocContiguous) == hipSuccess) {
            remember();
            return RB_OK;
        }
        (void)hipGetLastError();
    }
    hipError_t e = hipMalloc(dev_ptr, want);
    if (e != hipSuccess) {
        (void)hipGetLastError(); // reported through the return code: not left behind for the caller's next HIP call to trip over
        return fail(ctx, RB_E_NOMEM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
    }
    remember();
    return RB_OK;
}
// which route a buffer of rb_dev_alloc took: 1 = separately created 2 MB physical chunks, 0 = anything else (plain hipMalloc: a small
// request, a forced mode, the fallback when the chunked route failed or the address-space cap was reached; or a foreign pointer)
extern "C" int rb_dev_alloc_mode(rb_ctx *ctx, const void *dev_ptr) {
    if (!ctx || !dev_ptr) return RB_E_INVALID;
    std::lock_guard<std::mutex> lk(g_vmm_mu);
    return g_vmm.count(const_cast<void *>(dev_ptr)) ? 1 : 0;
}
static size_t rb_buf_bytes(rb_ctx *, void *p, bool *placed) {
    std::lock_guard<std::mutex> lk(g_vmm_mu);
    auto it = g_asked.find(p);
    if (it == g_asked.end()) return 0;
    auto iv = g_vmm.find(p);
    *placed = iv != g_vmm.end() && iv->second.placed;
    return it->second;
}
extern "C" int rb_dev_free(rb_ctx *ctx, void *dev_ptr) {
    if (!ctx) return RB_E_INVALID;
    if (!dev_ptr) return RB_OK;
    {
        std::lock_guard<std::mutex> lk(g_vmm_mu);
        g_asked.erase(dev_ptr);
    }
    hipError_t e = hipSuccess;
    const int mine = rb_free_vmm(dev_ptr, ctx->device, &e);
    if (mine < 0) return fail(ctx, RB_E_HIP, "rb_dev_free (chunked buffer): %s", hipGetErrorString(e));
    if (mine > 0) return RB_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipFree(dev_ptr));
    return RB_OK;
}
// rb_dev_release: the buffer goes back to the CONTEXT, not to the device -- it stays mapped, a chunked buffer keeps its physical pages
// (and with them what rb_dev_alloc_placed chose them for), and the next rb_dev_alloc / rb_dev_alloc_placed of exactly this size on this
// context returns it.  No address space is retired and nothing is unmapped, so a host that allocates and releases the same shapes batch
// after batch runs in constant address space and pays the 14 us per chunk once.  The cache holds at most RB_ALLOC_CACHE_GB (default
// 96) gigabytes: what does not fit is freed (rb_dev_free).  The caller's work on the buffer must have been enqueued on the context's
// stream (it is synchronised here) or be finished.
static size_t rb_cache_cap() {
    static const size_t v = [] { const char *e = getenv("RB_ALLOC_CACHE_GB"); return (size_t)(e ? strtoull(e, nullptr, 10) : 96ull) << 30; }();
    return v;
}
extern "C" int rb_dev_release(rb_ctx *ctx, void *dev_ptr) {
    if (!ctx) return RB_E_INVALID;
    if (!dev_ptr) return RB_OK;
    bool placed = false;
    const size_t bytes = rb_buf_bytes(ctx, dev_ptr, &placed);
    if (!bytes || bytes > rb_cache_cap()) return rb_dev_free(ctx, dev_ptr);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    while (!ctx->cache.empty() && ctx->cache_bytes + bytes > rb_cache_cap()) { // the oldest go first
        void *q = ctx->cache.front().p;
        ctx->cache_bytes -= ctx->cache.front().bytes;
        ctx->cache.erase(ctx->cache.begin());
        const int rc = rb_dev_free(ctx, q);
        if (rc) return rc;
    }
    ctx->cache.push_back({dev_ptr, bytes, placed});
    ctx->cache_bytes += bytes;
    return RB_OK;
}
// frees cached buffers, oldest first, until at most keep_bytes are held
extern "C" int rb_dev_cache_trim(rb_ctx *ctx, uint64_t keep_bytes) {
    if (!ctx) return RB_E_INVALID;
    while (!ctx->cache.empty() && ctx->cache_bytes > keep_bytes) {
        void *q = ctx->cache.front().p;
        ctx->cache_bytes -= ctx->cache.front().bytes;
        ctx->cache.erase(ctx->cache.begin());
        const int rc = rb_dev_free(ctx, q);
        if (rc) return rc;
    }
    return RB_OK;
}
// out[0] = bytes of live chunked buffers (this process), out[1] = bytes this context holds for reuse (rb_dev_release), out[2] = address
// space retired by freed chunked buffers (this process; never returned: rb_free_vmm), out[3] = the cap on out[0] + out[2],
// out[4] = rb_dev_alloc requests of this context that wanted the chunked route and got plain hipMalloc
extern "C" int rb_dev_alloc_stats(rb_ctx *ctx, uint64_t out[5]) {
    if (!ctx || !out) return RB_E_INVALID;
    std::lock_guard<std::mutex> lk(g_vmm_mu);
    out[0] = g_va_live, out[1] = ctx->cache_bytes, out[2] = g_va_retired, out[3] = rb_va_cap(), out[4] = ctx->alloc_fallbacks;
    return RB_OK;
}
static bool pin_ready(rb_ctx *ctx) {
    if (ctx->pin[0]) return true;
    static const bool off = getenv("RB_NO_PINNED") != nullptr; // diagnostics: the runtime's pageable path for everything
    if (off) return false;
    for (int k = 0; k < 2; k++) {
        if (hipHostMalloc(&ctx->pin[k], RB_PIN_CHUNK, hipHostMallocDefault) != hipSuccess || hipEventCreateWithFlags(&ctx->pin_ev[k], hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            for (int j = 0; j <= k; j++) {
                if (ctx->pin[j]) hipHostFree(ctx->pin[j]);
                if (ctx->pin_ev[j]) hipEventDestroy(ctx->pin_ev[j]);
                ctx->pin[j] = nullptr, ctx->pin_ev[j] = nullptr;
            }
            return false;
        }
    }
    return true;
}
static void par_memcpy(void *dst, const void *src, size_t n) { // a chunk of the staging ring, on a few host threads
    const unsigned T = n >= ((size_t)16 << 20) ? 8u : (n >= ((size_t)4 << 20) ? 4u : 1u); // (a thread copies 6-8 GB/s; the DMA behind it does 50+)
    if (T == 1) {
        memcpy(dst, src, n);
        return;
    }
    std::vector<std::thread> th;
    const size_t part = ((n + T - 1) / T + 63) & ~(size_t)63; // (rounded UP before the alignment: n / T rounded down left the last n % T bytes of a chunk uncopied
                                                              //  whenever n / T was a multiple of 64 -- found by the md5 of a 19 GB output, round 3)
    for (unsigned t = 1; t < T; t++) {
        const size_t lo = std::min(n, t * part), hi = std::min(n, (t + 1) * part);
        if (hi > lo) th.emplace_back([=]() { memcpy((char *)dst + lo, (const char *)src + lo, hi - lo); });
    }
    memcpy(dst, src, std::min(n, part));
    for (auto &x : th) x.join();
}
extern "C" int rb_dev_upload(rb_ctx *ctx, void *dev_dst, const void *host_src, size_t bytes) {
    if (!ctx) return RB_E_INVALID;
    if (!bytes) return RB_OK;
    // Every transfer goes through the context's own page-locked chunks (round 4; small ones used to be handed to the runtime as
    // pageable memory): one path, and the caller's buffer is never pinned behind its back.
    if (!pin_ready(ctx)) { // (no page-locked memory to be had: the runtime's path, synchronously)
        HIPCHK(ctx, hipMemcpy(dev_dst, host_src, bytes, hipMemcpyHostToDevice));
        return RB_OK;
    }
    // host_src is consumed chunk by chunk into page-locked memory; when the call returns the caller may reuse it, the DMAs are
    // queued on the context's stream
    // (the slot cursor runs on ACROSS calls: two small uploads in a row take different slots, so the second does not wait for the DMA --
    //  and whatever kernel was queued in front of it -- of the first)
    for (size_t off = 0; off < bytes; off += RB_PIN_CHUNK) {
        const int slot = (int)(ctx->pin_next++ & 1u);
        const size_t n = std::min(RB_PIN_CHUNK, bytes - off);
        if (ctx->pin_busy[slot]) HIPCHK(ctx, hipEventSynchronize(ctx->pin_ev[slot]));
        par_memcpy(ctx->pin[slot], (const char *)host_src + off, n);
        HIPCHK(ctx, hipMemcpyAsync((char *)dev_dst + off, ctx->pin[slot], n, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipEventRecord(ctx->pin_ev[slot], ctx->stream));
        ctx->pin_busy[slot] = true;
    }
    return RB_OK;
}
extern "C" int rb_dev_download(rb_ctx *ctx, void *host_dst, const void *dev_src, size_t bytes) {
    if (!ctx) return RB_E_INVALID;
    if (!bytes) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        return RB_OK;
    }
    if (!pin_ready(ctx)) { // (see rb_dev_upload)
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        HIPCHK(ctx, hipMemcpy(host_dst, dev_src, bytes, hipMemcpyDeviceToHost));
        return RB_OK;
    }
    // chunk k + 1 is in flight into one page-locked slot while chunk k leaves the other for host_dst
    size_t prev_off = 0, prev_n = 0;
    int prev_slot = -1;
    for (size_t off = 0, k = 0; off < bytes; off += RB_PIN_CHUNK, k++) {
        const int slot = (int)(k & 1);
        const size_t n = std::min(RB_PIN_CHUNK, bytes - off);
        if (ctx->pin_busy[slot]) HIPCHK(ctx, hipEventSynchronize(ctx->pin_ev[slot])); // (an upload that used the slot)
        HIPCHK(ctx, hipMemcpyAsync(ctx->pin[slot], (const char *)dev_src + off, n, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipEventRecord(ctx->pin_ev[slot], ctx->stream));
        ctx->pin_busy[slot] = true;
        if (prev_slot >= 0) {
            HIPCHK(ctx, hipEventSynchronize(ctx->pin_ev[prev_slot]));
            par_memcpy((char *)host_dst + prev_off, ctx->pin[prev_slot], prev_n);
            ctx->pin_busy[prev_slot] = false;
        }
        prev_off = off, prev_n = n, prev_slot = slot;
    }
    if (prev_slot >= 0) {
        HIPCHK(ctx, hipEventSynchronize(ctx->pin_ev[prev_slot]));
        par_memcpy((char *)host_dst + prev_off, ctx->pin[prev_slot], prev_n);
        ctx->pin_busy[prev_slot] = false;
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RB_OK;
}
extern "C" int rb_dev_memset(rb_ctx *ctx, void *dev_dst, int value, size_t bytes) {
    if (!ctx) return RB_E_INVALID;
    if (bytes) HIPCHK(ctx, rb_fill_async(dev_dst, value, bytes, ctx->stream));
    return RB_OK;
}

// ---- K1 ----------------------------------------------------------------------------------------
extern "C" int rb_dev_scan_records(rb_ctx *ctx, const rb_batch_view *b, rb_reduce_row *reduce_rows, rb_norm_row *norm_rows) {
    if (!ctx || !b) return RB_E_INVALID;
    if (((uintptr_t)b->ops & 15u) != 0) return fail(ctx, RB_E_INVALID, "ops must be 16-byte aligned");
    rb_scan_params p;
    p.n_rec = b->n_rec;
    p.ops = b->ops;
    p.op_off = b->op_off;
    p.t_st = b->t_st;
    p.t_en = b->t_en;
    p.q_st = b->q_st;
    p.q_en = b->q_en;
    p.strand = b->strand;
    p.reduce_rows = reduce_rows;
    p.norm_rows = norm_rows;
    p.list = nullptr;
    p.n_list = nullptr;
    ctx->scan_rows_n = 0;
    // a batch of short records (config 4's shape: a few hundred ops each) goes through the row form, four records per wavefront, and
    // only what that lists through the wave-per-record kernel
    if (b->n_rec >= 64 && b->n_ops / b->n_rec <= RB_SCAN_ROWS_MEAN_MAX) {
        if (ctx->scan_list_cap < b->n_rec) { // (grows with the largest batch seen: four bytes per record)
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            if (ctx->scan_list) hipFree(ctx->scan_list);
            ctx->scan_list = nullptr, ctx->scan_list_cap = 0;
            const uint64_t cap = b->n_rec + b->n_rec / 4 + 1024;
            if (hipMalloc(&ctx->scan_list, 256 + cap * 4) == hipSuccess) ctx->scan_list_cap = cap;
            else (void)hipGetLastError();
        }
        if (ctx->scan_list) {
            HIPCHK(ctx, rb_fill_async(ctx->scan_list, 0, 8, ctx->stream));
            HIPCHK(ctx, rb_launch_scan_rows(&p, ctx->scan_list, ctx->stream));
            ctx->scan_rows_n = b->n_rec;
            return RB_OK;
        }
    }
    HIPCHK(ctx, rb_launch_scan_records(&p, ctx->stream));
    return RB_OK;
}

// which kernel scanned what in the last rb_dev_scan_records call of this context: the list's count is still on the device
extern "C" int rb_ctx_scan_route(rb_ctx *ctx, uint64_t out[2]) {
    if (!ctx || !out) return RB_E_INVALID;
    out[0] = out[1] = 0;
    if (!ctx->scan_rows_n) return RB_OK; // the wave-per-record kernel took the whole batch (or nothing was scanned yet)
    unsigned long long n_listed = 0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemcpyAsync(&n_listed, ctx->scan_list, sizeof n_listed, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    out[0] = ctx->scan_rows_n - n_listed;
    out[1] = n_listed;
    return RB_OK;
}

// ---- plan ----------------------------------------------------------------------------------------
template <typename T>
static int upload_vec(rb_ctx *ctx, const std::vector<T> &v, T **dev) {
    int rc = rb_dev_alloc(ctx, v.size() * sizeof(T) + 16, (void **)dev);
    if (rc) return rc;
    if (!v.empty()) { // (through the context's page-locked chunks, like every host transfer of the library: rb_dev_upload says why)
        rc = rb_dev_upload(ctx, *dev, v.data(), v.size() * sizeof(T)); // (the host vector is consumed when this returns; the DMA is queued)
        if (rc) return rc;
    }
    return RB_OK;
}

// Tiles of short records (k_tile.hip): runs of consecutive records of 8 .. short_max ops, at most rb_tile_max_records() of them and
// rb_tile_max_ops() ops together, three words a tile {first record | pass-through << 31, records, schedule slot of the first record}; runs of
// records below 8 ops become pass-through tiles (the per-record kernel takes them: a lane's eight ops would hold three records).  `sched` comes
// in as the longest-first order of all records and leaves as: the records longer than short_max, longest first (*n_long of them: the
// per-record kernel's launch), then the others in MEMORY order -- their slots are never launched as waves of their own, they are where the
// records' jobs lie, so a tile's jobs lie side by side (one coalesced read instead of a gather, and rb_k_make_jobs writes them side by side).
// No tile worth the name (nothing of 8 ops and more below the line): tiles stays empty and sched as it was.
static void rb_cut_tiles(uint64_t n_rec, const uint64_t *op_off, uint64_t short_max, std::vector<uint32_t> &sched, std::vector<uint32_t> &tiles,
                         uint64_t *n_long_out) {
    tiles.clear();
    *n_long_out = 0;
    short_max = std::min<uint64_t>(short_max, rb_tile_max_ops());
    if (short_max < 8 || !n_rec) return;
    const uint64_t max_ops = rb_tile_max_ops(), max_rec = rb_tile_max_records();
    std::vector<uint32_t> t2;
    uint64_t first = 0, cnt = 0, ops = 0, n_long = 0, n_tiled = 0;
    bool tiny = false;
    auto close = [&]() {
        if (cnt) t2.push_back((uint32_t)first | (tiny ? 0x80000000u : 0u)), t2.push_back((uint32_t)cnt), n_tiled += tiny ? 0 : cnt;
        cnt = 0, ops = 0;
    };
    for (uint64_t r = 0; r < n_rec; r++) {
        const uint64_t n = op_off[r + 1] - op_off[r];
        if (n > short_max) {
            close();
            n_long++;
            continue;
        }
        const bool t = n < 8;
        if (cnt && (t != tiny || cnt >= max_rec || (!t && ops + n > max_ops))) close();
        if (!cnt) first = r, tiny = t;
        cnt++, ops += n;
    }
    close();
    if (n_tiled == 0) return;
    std::vector<uint32_t> s2(n_rec);
    uint64_t a = 0, b = n_long;
    for (uint64_t w = 0; w < n_rec; w++)
        if (op_off[(uint64_t)sched[w] + 1] - op_off[sched[w]] > short_max) s2[a++] = sched[w];
    std::vector<uint32_t> slot_short(n_rec, 0);
    for (uint64_t r = 0; r < n_rec; r++)
        if (op_off[r + 1] - op_off[r] <= short_max) slot_short[r] = (uint32_t)b, s2[b++] = (uint32_t)r;
    sched.swap(s2);
    tiles.reserve(t2.size() / 2 * 3);
    for (size_t t = 0; t + 1 < t2.size(); t += 2) tiles.push_back(t2[t]), tiles.push_back(t2[t + 1]), tiles.push_back(slot_short[t2[t] & 0x7FFFFFFFu]);
    *n_long_out = n_long;
}
// the same on plain host arrays, no device needed (tests/test_plan_tiles.py; a host that wants to know how a batch will be cut):
// sched_out [n_rec], tiles_out [3 * tiles_cap]; returns the number of tiles (tiles beyond tiles_cap are counted, not written), -1: bad arguments
extern "C" int64_t rb_plan_tiles_host(uint64_t n_rec, const uint64_t *op_off, uint64_t short_max, uint32_t *sched_out, uint32_t *tiles_out,
                                      uint64_t tiles_cap, uint64_t *n_long_out) {
    if (n_rec && (!op_off || !sched_out)) return -1;
    if (n_rec >= 0xFFFFFFFFull) return -1;
    std::vector<uint32_t> sched(n_rec), tiles;
    std::iota(sched.begin(), sched.end(), 0u);
    std::stable_sort(sched.begin(), sched.end(), [&](uint32_t x, uint32_t y) { return op_off[(uint64_t)x + 1] - op_off[x] > op_off[(uint64_t)y + 1] - op_off[y]; }); // (what rb_plan_create's radix sort gives)
    uint64_t n_long = 0;
    rb_cut_tiles(n_rec, op_off, short_max ? short_max : RB_SHORT_MAX_DEFAULT, sched, tiles, &n_long);
    for (uint64_t i = 0; i < n_rec; i++) sched_out[i] = sched[i];
    const uint64_t nt = tiles.size() / 3;
    for (uint64_t t = 0; t < nt && t < tiles_cap && tiles_out; t++)
        for (int k = 0; k < 3; k++) tiles_out[3 * t + k] = tiles[3 * t + k];
    if (n_long_out) *n_long_out = tiles.empty() ? n_rec : n_long;
    return (int64_t)nt;
}

extern "C" int rb_plan_create(rb_ctx *ctx, uint64_t n_rec, const uint64_t *op_off, const uint32_t *contig, uint64_t n_win,
                              const uint32_t *w_contig, const uint64_t *w_st, const uint64_t *w_en, rb_plan **out) {
    if (!ctx || !out || (n_rec && (!op_off || !contig))) return RB_E_INVALID;
    if (n_rec >= 0xFFFFFFFFull || n_win >= 0xFFFFFFFFull) return fail(ctx, RB_E_INVALID, "too many records/windows for one batch");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    rb_plan *pl = new rb_plan();
    pl->ctx = ctx;
    pl->n_rec = n_rec;
    pl->n_win = n_win;
    uint32_t maxc = 0;
    for (uint64_t i = 0; i < n_rec; i++) maxc = std::max(maxc, contig[i]);
    for (uint64_t i = 0; i < n_win; i++) maxc = std::max(maxc, w_contig[i]);
    const uint32_t n_contig = (n_rec || n_win) ? maxc + 1 : 0;
    pl->n_contig = n_contig;
    // canonical order: contigs by first appearance among the records (liftover.rs:151), then record order
    std::vector<uint32_t> canon_pos(n_rec);
    {
        std::vector<uint64_t> rank(n_contig, UINT64_MAX);
        uint64_t nr = 0;
        for (uint64_t i = 0; i < n_rec; i++)
            if (rank[contig[i]] == UINT64_MAX) rank[contig[i]] = nr++;
        std::vector<uint64_t> start(nr + 1, 0);
        for (uint64_t i = 0; i < n_rec; i++) start[rank[contig[i]] + 1]++;
        for (uint64_t k = 0; k < nr; k++) start[k + 1] += start[k];
        for (uint64_t i = 0; i < n_rec; i++) canon_pos[i] = (uint32_t)start[rank[contig[i]]]++;
    }
    // launch order: longest record first (pure load balancing)
    std::vector<uint32_t> sched(n_rec), ident(n_rec);
    std::iota(ident.begin(), ident.end(), 0u);
    {   // stable, descending by op count: an LSD radix sort on the complemented count, 16 bits a pass (a comparison sort of 1e6
        // records with its random reads of op_off took 90 ms of the host's time per plan; this takes a tenth)
        uint64_t max_len = 0;
        std::vector<uint64_t> key(n_rec);
        for (uint64_t i = 0; i < n_rec; i++) key[i] = op_off[i + 1] - op_off[i], max_len = std::max(max_len, key[i]);
        int passes = 0;
        while (passes < 4 && (max_len >> (16 * passes)) != 0) passes++;
        std::vector<uint32_t> a(ident), b(n_rec);
        std::vector<uint64_t> cnt(65537);
        for (int ps = 0; ps < passes; ps++) {
            std::fill(cnt.begin(), cnt.end(), 0);
            const int sh = 16 * ps;
            for (uint64_t i = 0; i < n_rec; i++) cnt[(0xFFFFu - (uint32_t)((key[i] >> sh) & 0xFFFFu)) + 1]++;
            for (int k = 0; k < 65536; k++) cnt[k + 1] += cnt[k];
            for (uint64_t i = 0; i < n_rec; i++) {
                const uint32_t r = a[i];
                b[cnt[0xFFFFu - (uint32_t)((key[r] >> sh) & 0xFFFFu)]++] = r;
            }
            a.swap(b);
        }
        sched = a;
    }
    // windows grouped by contig, BED order kept inside a contig
    std::vector<uint64_t> cw_off(n_contig + 1, 0), g_st(n_win), g_en(n_win), o_st(n_win), o_en(n_win);
    std::vector<uint32_t> g_orig(n_win);
    std::vector<uint8_t> mono(n_contig ? n_contig : 1, 1);
    for (uint64_t i = 0; i < n_win; i++) cw_off[w_contig[i] + 1]++;
    for (uint32_t c = 0; c < n_contig; c++) cw_off[c + 1] += cw_off[c];
    {
        std::vector<uint64_t> cur(cw_off.begin(), cw_off.end() - (n_contig ? 1 : 0));
        for (uint64_t i = 0; i < n_win; i++) {
            const uint64_t d = cur[w_contig[i]]++;
            g_st[d] = w_st[i];
            g_en[d] = w_en[i];
            g_orig[d] = (uint32_t)i;
            o_st[i] = w_st[i];
            o_en[i] = w_en[i];
        }
    }
    for (uint32_t c = 0; c < n_contig; c++)
        for (uint64_t i = cw_off[c] + 1; i < cw_off[c + 1]; i++)
            if (g_st[i] < g_st[i - 1] || g_en[i] < g_en[i - 1]) mono[c] = 0;
    // how deep the sorted window lists overlap: clip j of a record goes to output slot j mod depth (k_liftover.hip), so that
    // clips sharing a slot follow one another along the record; en == st counts as overlapping (both clips may cut one op)
    pl->n_ops = n_rec ? op_off[n_rec] : 0;
    for (uint32_t c = 0; c < n_contig; c++) {
        if (!mono[c]) continue;
        uint64_t lo = cw_off[c];
        for (uint64_t i = cw_off[c]; i < cw_off[c + 1]; i++) {
            while (lo < i && g_en[lo] < g_st[i]) lo++; // (a window with en < st may not push lo past i)
            pl->depth = std::max<uint32_t>(pl->depth, (uint32_t)std::min<uint64_t>(i - lo + 1, 1u << 20));
        }
    }
    // tiles of short records (k_tile.hip): rb_plan_tiles_host below.  RB_TILE=0 switches the tile kernel off, RB_SHORT_MAX=<ops> moves the
    // line between the two kernels (experiments).
    std::vector<uint32_t> tiles;
    pl->stream_end = (uint32_t)n_rec;
    {
        const char *e = getenv("RB_TILE");
        const bool on = !(e && !strcmp(e, "0"));
        uint64_t short_max = RB_SHORT_MAX_DEFAULT;
        if (const char *m = getenv("RB_SHORT_MAX")) short_max = strtoull(m, nullptr, 10);
        if (on && n_rec) {
            uint64_t n_long = 0;
            rb_cut_tiles(n_rec, op_off, short_max, sched, tiles, &n_long);
            if (!tiles.empty()) pl->stream_end = (uint32_t)n_long;
        }
        pl->n_tiles = (uint32_t)(tiles.size() / 3);
    }
    int rc = RB_OK;
    std::vector<uint32_t> slot_of(n_rec);
    for (uint64_t w = 0; w < n_rec; w++) slot_of[sched[w]] = (uint32_t)w;
    if (!rc) rc = upload_vec(ctx, sched, &pl->sched);
    if (!rc) rc = upload_vec(ctx, slot_of, &pl->slot_of);
    if (!rc) rc = upload_vec(ctx, ident, &pl->ident);
    if (!rc) rc = upload_vec(ctx, canon_pos, &pl->canon_pos);
    if (!rc) rc = upload_vec(ctx, g_st, &pl->w_st);
    if (!rc) rc = upload_vec(ctx, g_en, &pl->w_en);
    if (!rc) rc = upload_vec(ctx, g_orig, &pl->w_orig);
    if (!rc) rc = upload_vec(ctx, o_st, &pl->wo_st);
    if (!rc) rc = upload_vec(ctx, o_en, &pl->wo_en);
    if (!rc) rc = upload_vec(ctx, cw_off, &pl->cw_off);
    if (!rc) rc = upload_vec(ctx, mono, &pl->cw_mono);
    if (!rc && pl->n_tiles) rc = upload_vec(ctx, tiles, &pl->tiles);
    if (!rc && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = fail(ctx, RB_E_HIP, "plan upload: %s", hipGetErrorString(hipGetLastError())); // (once, for all of them)
    if (rc) {
        rb_plan_destroy(pl);
        return rc;
    }
    *out = pl;
    return RB_OK;
}
extern "C" void rb_plan_destroy(rb_plan *pl) {
    if (!pl) return;
    void *ptrs[] = {pl->sched, pl->slot_of, pl->ident, pl->canon_pos, pl->w_st, pl->w_en, pl->w_orig, pl->wo_st, pl->wo_en, pl->cw_off, pl->cw_mono, pl->tiles};
    for (void *q : ptrs)
        if (q) (void)rb_dev_free(pl->ctx, q); // (rb_dev_alloc memory: a large array is a chunked buffer, which hipFree does not know)
    delete pl;
}

// workspace layout: [hit_off (n_rec+1) u64][win_lo][block sums][arena cursors][jobs n_rec x 64 B][gen_list rows_cap u32][x_st rows_cap u64][x_en rows_cap u64]
struct ws_layout {
    size_t hit_off, win_lo, block_sums, arena, pend_count, pend_list, jobs, gen_list, x_st, x_en, bp_tmp, bp_off, bp_cur, brk_rows, copy_count, copy_list, decl_count, decl_list, gen_cp, diag_stamps, fb_count, fb_list, starts_bad, total;
};
// RB_DEBUG_NO_GEN_CP (diagnostics: the generic kernel walks every record from its first op, no room for checkpoints): read ONCE per
// process -- the workspace layout and the kernel parameter must agree on it
static bool rb_no_gen_cp() {
    static const bool v = getenv("RB_DEBUG_NO_GEN_CP") != nullptr;
    return v;
}
static ws_layout ws_of(uint64_t n_rec, uint64_t rows_cap, uint64_t n_ops) {
    ws_layout w;
    size_t o = 0;
    auto take = [&](size_t bytes) {
        size_t at = o;
        o += (bytes + 255) & ~(size_t)255;
        return at;
    };
    w.hit_off = take((n_rec + 2) * 8);
    w.win_lo = take((n_rec + 2) * 4);
    w.block_sums = take(rb_scan_block_sums_count(n_rec) * 8);
    w.arena = take((size_t)RB_MAX_ARENA * RB_ARENA_STRIDE * 8);
    w.pend_count = take(256);
    w.pend_list = take((n_rec + 1) * 4);
    w.jobs = take((n_rec + 1) * sizeof(rb_job));
    w.gen_list = take((rows_cap + 1) * 4);
    w.x_st = take((rows_cap + 1) * 8);
    w.x_en = take((rows_cap + 1) * 8);
    w.bp_tmp = take((rows_cap + 1) * 8); // break-paf: piece windows between the collect pass and their rows
    w.bp_off = take((n_rec + 1) * 8);
    w.bp_cur = take((size_t)RB_MAX_ARENA * 128);
    w.brk_rows = take((rows_cap + 1) * sizeof(rb_hit_row)); // break-paf in one walk: the rows before they are in record order
    w.copy_count = take(256);
    w.copy_list = take((rows_cap + 1) * 16);
    w.decl_count = take(256);
    w.decl_list = take((n_rec + 1) * 4); // break-paf in one walk: the records its clip kernel declined
    w.gen_cp = take(rb_no_gen_cp() ? 256 : (size_t)(n_ops / RB_GCP + n_rec + 2) * sizeof(uint4)); // checkpoints of the records the generic kernel works on
    w.diag_stamps = take((n_rec + 1) * 4); // diagnostics build of the clip kernel: when each record's wave was done
    w.fb_count = take(256);
    w.fb_list = take((n_rec + 1) * 4); // the records of the tiles the tile kernel handed to the per-record kernel
    w.starts_bad = take(256);          // RB_LIFT_OP_STARTS: the first record outside the batch
    w.total = o;
    return w;
}
extern "C" size_t rb_plan_workspace_bytes(const rb_plan *plan, uint64_t rows_cap) {
    if (!plan) return 0;
    return ws_of(plan->n_rec, rows_cap, plan->n_ops).total;
}
extern "C" size_t rb_plan_diag_stamps_offset(const rb_plan *plan, uint64_t rows_cap) {
    if (!plan) return 0;
    return ws_of(plan->n_rec, rows_cap, plan->n_ops).diag_stamps;
}

// ops per output slot: the batch's op index space, 32 ops (one 128-byte line) of room per record (records that share a line in the
// input must not share one in the output), a multiple of 32
static uint64_t slot_stride_of(uint64_t n_ops, uint64_t n_rec) { return ((n_ops + 31) & ~(uint64_t)31) + 32 * n_rec + 64; }
extern "C" uint64_t rb_plan_out_capacity(const rb_plan *plan, int for_break) {
    if (!plan) return 0;
    const uint64_t slots = for_break ? std::min<uint32_t>(2u, RB_MS) : std::min<uint32_t>(plan->depth, RB_MS);
    return slots * slot_stride_of(plan->n_ops, plan->n_rec) + plan->n_ops / 16 + 32 * plan->n_rec + (1u << 20);
}

static uint32_t pick_arenas(uint64_t n_rec) {
    uint64_t a = n_rec / 256;
    if (a < 1) a = 1;
    if (a > RB_MAX_ARENA) a = RB_MAX_ARENA;
    return (uint32_t)a;
}

static int lift_common(rb_ctx *ctx, const rb_plan *plan, const rb_batch_view *b, const rb_norm_row *norm, int policy,
                       void *workspace, rb_hit_row *rows, uint64_t rows_cap, uint32_t *out_ops, uint64_t out_cap,
                       rb_counters *counters, bool is_break, uint32_t max_size) {
    if (!ctx || !plan || !b || !norm || !workspace || !counters) return RB_E_INVALID;
    if (b->n_rec != plan->n_rec) return fail(ctx, RB_E_INVALID, "plan was built for %llu records, batch has %llu", (unsigned long long)plan->n_rec, (unsigned long long)b->n_rec);
    if (((uintptr_t)b->ops & 15u) || ((uintptr_t)out_ops & 15u)) return fail(ctx, RB_E_INVALID, "ops/out_ops must be 16-byte aligned");
    if (rows_cap >= 0xFFFFFFFFull) return fail(ctx, RB_E_INVALID, "rows_cap too large");
    if ((uintptr_t)workspace & 255u) return fail(ctx, RB_E_INVALID, "workspace must be 256-byte aligned");
    const ws_layout w = ws_of(plan->n_rec, rows_cap, plan->n_ops);
    char *ws = (char *)workspace;
    rb_lift_params p;
    memset(&p, 0, sizeof p);
    p.n_rec = b->n_rec;
    p.ops = b->ops;
    p.op_off = b->op_off;
    p.contig = b->contig;
    p.strand = b->strand;
    p.norm = norm;
    p.sched = plan->sched;
    p.slot_of = plan->slot_of;
    p.canon_pos = is_break ? plan->ident : plan->canon_pos;
    p.w_st = plan->w_st;
    p.w_en = plan->w_en;
    p.w_orig = plan->w_orig;
    p.wo_st = plan->wo_st;
    p.wo_en = plan->wo_en;
    p.cw_off = plan->cw_off;
    p.cw_mono = plan->cw_mono;
    p.n_contig = plan->n_contig;
    p.hit_off = (uint64_t *)(ws + w.hit_off);
    p.win_lo = (uint32_t *)(ws + w.win_lo);
    p.rows = rows;
    p.rows_cap = rows_cap;
    p.out_ops = out_ops;
    p.out_cap = out_cap;
    p.arena_cur = (unsigned long long *)(ws + w.arena);
    p.n_arena = pick_arenas(b->n_rec);
    p.desc_mode = (policy & RB_LIFT_DESCRIPTORS) ? 1 : 0;
    // out_ops = [slots the streaming kernel emits into | arenas of the generic and the copy kernel] (descriptor mode: [descriptors | arenas]).
    // As many slots as the window lists overlap deep (break-paf: two -- its pieces do not overlap, but neighbours end and begin in
    // the same 128-byte line, and a slot wants its clips four lines apart), as far as out_cap allows; with fewer,
    // or none, the clips that lose their place are copied into the arenas instead: slower, same rows.
    p.slot_stride = slot_stride_of(b->n_ops, b->n_rec);
    const uint32_t want = p.desc_mode ? 0u : std::min<uint32_t>(is_break ? 2u : plan->depth, RB_MS);
    const uint64_t min_arena = 1024ull * p.n_arena;
    uint32_t n_slots = want;
    while (n_slots && (uint64_t)n_slots * p.slot_stride + min_arena > out_cap) n_slots--;
    if (getenv("RB_DEBUG_SLOTS")) n_slots = std::min<uint32_t>(n_slots, (uint32_t)atoi(getenv("RB_DEBUG_SLOTS"))); // tests: force the copy path
    p.n_slots = n_slots;
    p.needed_base = p.desc_mode ? 4 * rows_cap : (uint64_t)want * p.slot_stride;
    p.arena_origin = p.desc_mode ? 4 * rows_cap : (uint64_t)n_slots * p.slot_stride;
    if (p.desc_mode && out_cap < p.arena_origin + 1024) return fail(ctx, RB_E_CAPACITY, "descriptor mode needs out_cap >= 4 * rows_cap + 1024");
    p.arena_size = out_cap > p.arena_origin ? ((out_cap - p.arena_origin) / p.n_arena) & ~(uint64_t)3 : 0;
    p.copy_list = (uint4 *)(ws + w.copy_list);
    // the generic kernel's per-hit descriptors take three arrays that are done with by the time it runs (rb_lift.h)
    p.gj_a = (rb_gja *)(ws + w.brk_rows), p.gj_b = (uint4 *)(ws + w.copy_list), p.gj_c = (uint2 *)(ws + w.bp_tmp);
    p.copy_count = (unsigned long long *)(ws + w.copy_count);
    p.gen_list = (uint32_t *)(ws + w.gen_list);
    p.gen_cp = rb_no_gen_cp() ? nullptr : (uint4 *)(ws + w.gen_cp);
    p.diag_stamps = (uint32_t *)(ws + w.diag_stamps); // (diagnostics: every generic walk from the record's first op, as before round 3)
    p.jobs = (rb_job *)(ws + w.jobs);
    p.fused = (policy & RB_LIFT_FUSED_SCAN) ? 1 : 0;
    p.op_starts = (policy & RB_LIFT_OP_STARTS) ? 1 : 0;
    if (p.op_starts && p.fused) return fail(ctx, RB_E_INVALID, "RB_LIFT_OP_STARTS takes finished norm_rows: not together with RB_LIFT_FUSED_SCAN");
    if (p.op_starts && (policy & RB_LIFT_DESCRIPTORS)) return fail(ctx, RB_E_INVALID, "RB_LIFT_OP_STARTS with RB_LIFT_DESCRIPTORS: a descriptor indexes the record's ORIGINAL cigar, which a batch cut in place no longer is");
    if (p.op_starts && b->n_ops > plan->n_ops) return fail(ctx, RB_E_INVALID, "RB_LIFT_OP_STARTS: batch->n_ops exceeds the plan's op count (gather the batch first)");
    if (p.op_starts && b->n_rec) {
        // the contract, enforced before any clip kernel runs: a record a pass has moved lies at or behind batch->n_ops, where the
        // per-record state sized by the plan's op count (the generic kernel's checkpoints, gen_cp) and the tiles do not reach.  One
        // check over the starts and the norm rows, and one wait for it
        unsigned long long *bad = (unsigned long long *)(ws + w.starts_bad), first_bad = 0;
        HIPCHK(ctx, rb_fill_async(bad, 0xFF, 8, ctx->stream));
        HIPCHK(ctx, rb_launch_starts_check(b->op_off, norm, b->n_rec, b->n_ops, bad, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(&first_bad, bad, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if (first_bad != ~0ull)
            return fail(ctx, RB_E_INVALID, "RB_LIFT_OP_STARTS: record %llu lies outside the batch's %llu ops (a pass moved it: gather the batch first)",
                        first_bad, (unsigned long long)b->n_ops);
    }
    p.norm_w = const_cast<rb_norm_row *>(norm);
    p.pend_list = (uint32_t *)(ws + w.pend_list);
    p.pend_count = (unsigned long long *)(ws + w.pend_count);
    // short records go through the tile kernel (k_tile.hip); the diagnostics builds keep every record on the per-record kernel
    const bool use_tiles = plan->n_tiles != 0 && ((policy >> 8) & 0xFFF) == 0;
    p.tile_first = use_tiles ? plan->tiles : nullptr;
    p.n_tiles = use_tiles ? plan->n_tiles : 0;
    p.fb_list = (uint32_t *)(ws + w.fb_list);
    p.fb_count = (unsigned long long *)(ws + w.fb_count);
    const uint32_t stream_end = use_tiles ? plan->stream_end : (uint32_t)b->n_rec;
    rb_scan_params sp;
    memset(&sp, 0, sizeof sp);
    if (p.fused) {
        sp.n_rec = b->n_rec;
        sp.ops = b->ops;
        sp.op_off = b->op_off;
        sp.t_st = b->t_st, sp.t_en = b->t_en, sp.q_st = b->q_st, sp.q_en = b->q_en;
        sp.strand = b->strand;
        sp.norm_rows = p.norm_w;
        HIPCHK(ctx, rb_fill_async(p.pend_count, 0, 8, ctx->stream));
        HIPCHK(ctx, rb_launch_peek_norm(&sp, ctx->stream)); // provisional rows from the records' ends
    }
    p.counters = counters;
    p.policy = policy & 1;
    p.early_exit = (policy & RB_LIFT_EARLY_EXIT) ? 1 : 0;
    p.debug_skip = (policy >> 8) & 0xFFF; // diagnostics only, undocumented on purpose
    uint64_t *block_sums = (uint64_t *)(ws + w.block_sums);
    HIPCHK(ctx, rb_fill_async(counters, 0, sizeof(rb_counters), ctx->stream));
    HIPCHK(ctx, rb_fill_async(p.copy_count, 0, 8, ctx->stream));
    HIPCHK(ctx, rb_fill_async(p.arena_cur, 0, (size_t)RB_MAX_ARENA * RB_ARENA_STRIDE * 8, ctx->stream));
    if (b->n_rec == 0) return RB_OK;
    const bool one_walk = is_break && (policy & RB_BREAK_ONE_WALK) && !p.desc_mode;
    if (one_walk) {
        // the clip kernel finds the long indels while it streams (k_liftover.hip, BRK): no pass over the ops before it.  Rows land
        // in scratch (one bump cursor of 256 per record), the piece counts are scanned, rb_k_break_gather orders the rows
        p.brk_mode = 1, p.brk_max = max_size;
        p.rows_final = rows;
        p.rows = (rb_hit_row *)(ws + w.brk_rows);
        p.brk_off = (uint64_t *)(ws + w.bp_off);
        p.brk_cursor = (unsigned long long *)(ws + w.bp_cur);
        p.brk_n_arena = pick_arenas(b->n_rec);
        p.brk_arena_cap = rows_cap / p.brk_n_arena;
        p.brk_decl_list = (uint32_t *)(ws + w.decl_list);
        p.brk_decl_count = (unsigned long long *)(ws + w.decl_count);
        HIPCHK(ctx, rb_fill_async(p.brk_decl_count, 0, 8, ctx->stream));
        HIPCHK(ctx, rb_fill_async(p.brk_cursor, 0, (size_t)RB_MAX_ARENA * 128, ctx->stream));
        HIPCHK(ctx, rb_fill_async(p.hit_off, 0, (size_t)(b->n_rec + 2) * 8, ctx->stream));
        HIPCHK(ctx, rb_fill_async(p.brk_off, 0xFF, (size_t)(b->n_rec + 1) * 8, ctx->stream));
        HIPCHK(ctx, rb_launch_make_jobs(&p, ctx->stream));
        const size_t slot1 = (size_t)(ctx->timed_calls % RB_TIMING_RING);
        if (ctx->timing) HIPCHK(ctx, hipEventRecord(ctx->ev_a[slot1], ctx->stream));
        p.wave0 = 0;
        p.wave_end = stream_end;
        HIPCHK(ctx, rb_launch_liftover_stream(&p, ctx->stream));
        if (use_tiles) {
            HIPCHK(ctx, rb_fill_async(p.fb_count, 0, 8, ctx->stream));
            HIPCHK(ctx, rb_launch_liftover_tiles(&p, ctx->stream));
            HIPCHK(ctx, rb_launch_liftover_stream_list(&p, ctx->stream));
        }
        if (p.fused) {
            sp.list = p.pend_list;
            sp.n_list = (const uint64_t *)p.pend_count;
            HIPCHK(ctx, rb_launch_scan_records(&sp, ctx->stream));
        }
        if (ctx->timing) {
            HIPCHK(ctx, hipEventRecord(ctx->ev_b[slot1], ctx->stream));
            ctx->timed_calls++;
        }
        // the records the clip kernel declined, one by one: their pieces counted (list mode) before the scan of the counts, their
        // windows written to their rows' places after it, rows + generic-list entries made, and the generic kernel clips them
        rb_break_params bp;
        memset(&bp, 0, sizeof bp);
        bp.n_rec = b->n_rec, bp.ops = b->ops, bp.op_off = b->op_off, bp.norm = norm, bp.sched = plan->sched, bp.hit_off = p.hit_off;
        bp.x_st = (uint64_t *)(ws + w.x_st), bp.x_en = (uint64_t *)(ws + w.x_en);
        bp.rows_cap = rows_cap, bp.max_size = max_size;
        bp.list = p.brk_decl_list, bp.n_list = p.brk_decl_count;
        bp.fill = 0;
        HIPCHK(ctx, rb_launch_break_list_declined(&p, ctx->stream));
        HIPCHK(ctx, rb_launch_break_pieces(&bp, ctx->stream));
        HIPCHK(ctx, rb_launch_count_and_scan(&p, block_sums, false, ctx->stream));
        bp.fill = 1;
        HIPCHK(ctx, rb_launch_break_pieces(&bp, ctx->stream));
        HIPCHK(ctx, rb_launch_break_gather(&p, ctx->stream)); // (copies the clips without a slot, moves the rows into record order)
        rb_lift_params pg = p; // the generic kernel works on the final rows, with the declined records' windows as explicit windows
        pg.rows = rows, pg.x_st = bp.x_st, pg.x_en = bp.x_en;
        HIPCHK(ctx, rb_launch_break_declined(&pg, ctx->stream));
        return RB_OK;
    }
    if (is_break) {
        rb_break_params bp;
        memset(&bp, 0, sizeof bp);
        bp.n_rec = b->n_rec;
        bp.ops = b->ops;
        bp.op_off = b->op_off;
        bp.norm = norm;
        bp.sched = plan->sched;
        bp.hit_off = p.hit_off;
        bp.x_st = (uint64_t *)(ws + w.x_st);
        bp.x_en = (uint64_t *)(ws + w.x_en);
        bp.rows_cap = rows_cap;
        bp.max_size = max_size;
        // one walk of the ops: count the pieces of every record and keep their windows (tmp[]), scan the counts, move the
        // windows to their rows; a second walk only for records with more pieces than the collect pass keeps
        bp.tmp = (uint2 *)(ws + w.bp_tmp);
        bp.tmp_off = (uint64_t *)(ws + w.bp_off);
        bp.tmp_cursor = (unsigned long long *)(ws + w.bp_cur);
        bp.n_arena = pick_arenas(b->n_rec);
        bp.arena_cap = rows_cap / bp.n_arena;
        HIPCHK(ctx, rb_fill_async(bp.tmp_cursor, 0, (size_t)RB_MAX_ARENA * 128, ctx->stream));
        bp.fill = 2, bp.redo_only = 0;
        HIPCHK(ctx, rb_launch_break_pieces(&bp, ctx->stream));
        HIPCHK(ctx, rb_launch_count_and_scan(&p, block_sums, false, ctx->stream));
        HIPCHK(ctx, rb_launch_break_place(&bp, ctx->stream));
        bp.fill = 1, bp.redo_only = 1;
        HIPCHK(ctx, rb_launch_break_pieces(&bp, ctx->stream));
        p.x_st = bp.x_st;
        p.x_en = bp.x_en;
    } else {
        HIPCHK(ctx, rb_launch_count_and_scan(&p, block_sums, true, ctx->stream));
    }
    // The clip kernels.  Liftover with long AND short records runs the tile kernel BESIDE the per-record kernel, on the context's side
    // stream: four waves of rb_k_liftover_stream per SIMD take 416 of the 512 vector registers and four of its workgroups 116,800 of a
    // CU's 163,840 bytes of LDS, which leaves room for exactly one workgroup of rb_k_liftover_tile (96 registers, 29,696 bytes) that
    // the per-record kernel cannot use.  Order: fork event | side stream: wait, tiles, list kernel over what the
    // tiles hand back, join event | main stream: per-record kernel, wait for the join, the rest.  The side stream's launches are
    // issued first, so that both queues hold work when the large grid arrives.  The two kernels share no output line (a tile's clips
    // lie in the slot lines of its own records, slot_stride_of) and append to the lists and arena cursors with atomics only, so rows
    // and clip contents are the single-stream call's; the order of list entries, hence out_off of arena clips, may differ.  The
    // timing bracket covers max(per-record kernel, tiles + list).  Everything else (no tiles, no long records, break-paf -- its
    // per-record build runs five waves of 96 registers per SIMD and leaves no room --, diagnostics builds, RB_TILE=0, and
    // RB_TILE_BESIDE=0 in the environment, read per call: tests, A/B runs, callers who capture the call in a graph and want no
    // branch in it) is one stream, launch for launch as before.
    const char *tb = getenv("RB_TILE_BESIDE");
    const bool beside = use_tiles && !is_break && stream_end != 0 && !(tb && atoi(tb) == 0);
    if (use_tiles && !is_break) HIPCHK(ctx, rb_fill_async(p.fb_count, 0, 8, ctx->stream)); // (the last call's list kernel is done: that call joined)
    HIPCHK(ctx, rb_launch_make_jobs(&p, ctx->stream));
    const size_t slot = (size_t)(ctx->timed_calls % RB_TIMING_RING);
    if (beside) HIPCHK(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));
    if (ctx->timing) HIPCHK(ctx, hipEventRecord(ctx->ev_a[slot], ctx->stream));
    p.wave0 = 0;
    p.wave_end = stream_end;
    if (beside) {
        // from here to the join the side stream may write the caller's buffers: no return before it is idle or the main stream waits for it
        hipError_t e = hipStreamWaitEvent(ctx->side, ctx->ev_fork, 0);
        const char *what = "hipStreamWaitEvent(fork)";
        if (e == hipSuccess) e = rb_launch_liftover_tiles(&p, ctx->side), what = "rb_launch_liftover_tiles";
        if (e == hipSuccess) e = rb_launch_liftover_stream_list(&p, ctx->side), what = "rb_launch_liftover_stream_list";
        if (e == hipSuccess) e = hipEventRecord(ctx->ev_join, ctx->side), what = "hipEventRecord(join)";
        if (e == hipSuccess) e = rb_launch_liftover_stream(&p, ctx->stream), what = "rb_launch_liftover_stream";
        if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0), what = "hipStreamWaitEvent(join)";
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(ctx->side);
            return fail(ctx, RB_E_HIP, "%s: %s", what, hipGetErrorString(e));
        }
    } else {
        HIPCHK(ctx, rb_launch_liftover_stream(&p, ctx->stream));
        if (use_tiles) {
            if (is_break) HIPCHK(ctx, rb_fill_async(p.fb_count, 0, 8, ctx->stream));
            HIPCHK(ctx, rb_launch_liftover_tiles(&p, ctx->stream));
            HIPCHK(ctx, rb_launch_liftover_stream_list(&p, ctx->stream));
        }
    }
    if (p.fused) { // the full record scan for the records the clip kernel handed back (usually none)
        sp.list = p.pend_list;
        sp.n_list = (const uint64_t *)p.pend_count;
        HIPCHK(ctx, rb_launch_scan_records(&sp, ctx->stream));
    }
    if (ctx->timing) {
        HIPCHK(ctx, hipEventRecord(ctx->ev_b[slot], ctx->stream));
        ctx->timed_calls++;
    }
    HIPCHK(ctx, rb_launch_liftover_tail(&p, ctx->stream));
    return RB_OK;
}

extern "C" int rb_dev_liftover(rb_ctx *ctx, const rb_plan *plan, const rb_batch_view *batch, const rb_norm_row *norm_rows,
                               int bsearch_policy, void *workspace, rb_hit_row *rows, uint64_t rows_cap, uint32_t *out_ops,
                               uint64_t out_cap, rb_counters *counters) {
    return lift_common(ctx, plan, batch, norm_rows, bsearch_policy, workspace, rows, rows_cap, out_ops, out_cap, counters, false, 0);
}
extern "C" int rb_dev_break(rb_ctx *ctx, const rb_plan *plan, const rb_batch_view *batch, const rb_norm_row *norm_rows,
                            uint32_t max_size, int bsearch_policy, void *workspace, rb_hit_row *rows, uint64_t rows_cap,
                            uint32_t *out_ops, uint64_t out_cap, rb_counters *counters) {
    return lift_common(ctx, plan, batch, norm_rows, bsearch_policy, workspace, rows, rows_cap, out_ops, out_cap, counters, true, max_size);
}

extern "C" int rb_dev_swap(rb_ctx *ctx, const rb_batch_view *b, uint32_t *out_ops) {
    if (!ctx || !b || !out_ops) return RB_E_INVALID;
    rb_swap_params p;
    p.n_rec = b->n_rec;
    p.ops = b->ops;
    p.op_off = b->op_off;
    p.strand = b->strand;
    p.out_ops = out_ops;
    if (out_ops == b->ops) { // in place
        HIPCHK(ctx, rb_launch_swap_inplace(&p, ctx->stream));
        return RB_OK;
    }
    // (rb_k_swap reads a record's words while other lanes write them: an output that shares words with the input is only right when it IS the input)
    if (out_ops < b->ops + b->n_ops && b->ops < out_ops + b->n_ops)
        return fail(ctx, RB_E_INVALID, "rb_dev_swap: out_ops overlaps the batch's ops without being equal to them (in place: out_ops == batch->ops)");
    HIPCHK(ctx, rb_launch_swap(&p, ctx->stream));
    return RB_OK;
}

static int trim_pend_reserve(rb_ctx *ctx, uint64_t n_pairs) {
    if (ctx->trim_pend && ctx->trim_pend_cap >= n_pairs) return RB_OK;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->trim_pend) hipFree(ctx->trim_pend);
    ctx->trim_pend = nullptr, ctx->trim_pend_cap = 0;
    const uint64_t cap = n_pairs + n_pairs / 4 + 1024;
    const hipError_t e = hipMalloc(&ctx->trim_pend, 256 + cap * 4); // (4 bytes per pair, beside rows of 128 the caller has allocated)
    if (e != hipSuccess) {
        ctx->trim_pend = nullptr, (void)hipGetLastError();
        return fail(ctx, RB_E_NOMEM, "hipMalloc(list of %llu pending pairs): %s", (unsigned long long)cap, hipGetErrorString(e));
    }
    ctx->trim_pend_cap = cap;
    return RB_OK;
}
extern "C" int rb_dev_trim_reserve(rb_ctx *ctx, uint64_t n_pairs) {
    if (!ctx) return RB_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return trim_pend_reserve(ctx, n_pairs);
}

extern "C" int rb_dev_overlap_split(rb_ctx *ctx, const rb_batch_view *b, const rb_norm_row *norm, uint64_t n_pairs, const uint32_t *left,
                                    const uint32_t *right, const uint64_t *pair_out_off, int match_score, int diff_score,
                                    int indel_score, int policy, rb_pair_row *rows, uint32_t *out_ops) {
    if (!ctx || !b || !norm || (n_pairs && (!left || !right || !pair_out_off || !rows || !out_ops))) return RB_E_INVALID;
    rb_trim_params p;
    p.n_pairs = n_pairs;
    p.ops = b->ops;
    p.op_off = b->op_off;
    p.strand = b->strand;
    p.norm = norm;
    p.left = left;
    p.right = right;
    p.pair_out_off = pair_out_off;
    p.match_score = match_score;
    p.diff_score = diff_score;
    p.indel_score = indel_score;
    p.policy = policy & 1;
    p.rows = rows;
    p.out_ops = out_ops;
    p.list_declined = 0; // (rb_launch_overlap_split sets it for its first attempt)
    p.in_place = (policy & RB_TRIM_IN_PLACE) ? 1 : 0;
    if (p.in_place && out_ops != b->ops) return fail(ctx, RB_E_INVALID, "RB_TRIM_IN_PLACE: out_ops must be the batch's own ops array");
    if (!ctx->trim_scratch) { // (40 MB, once per context; without it those pairs simply stay with the serial kernel)
        const uint32_t blocks = 48;
        if (hipMalloc(&ctx->trim_scratch, rb_trim_scratch_bytes(blocks)) == hipSuccess) ctx->trim_scratch_blocks = blocks;
        else ctx->trim_scratch = nullptr, (void)hipGetLastError();
    }
    p.scratch = (uint32_t *)ctx->trim_scratch;
    p.scratch_blocks = ctx->trim_scratch_blocks;
    { // (the list grows with the largest pass seen; a few bytes per pair.  rb_dev_trim_reserve takes the growth out of the first pass)
        const int rc = trim_pend_reserve(ctx, n_pairs);
        if (rc) return rc;
    }
    p.pend = (unsigned long long *)ctx->trim_pend;
    p.pend_list = (uint32_t *)((char *)ctx->trim_pend + 256);
    HIPCHK(ctx, rb_fill_async(p.pend, 0, 8, ctx->stream));
    HIPCHK(ctx, rb_launch_overlap_split(&p, ctx->stream));
    return RB_OK;
}

// scratch of rb_dev_trim_select: [slot (n_groups + 2) u64][has (n_groups + 2) u64][cand 2 n_groups u32][block sums of the scans]
extern "C" size_t rb_trim_select_scratch_bytes(uint64_t n_groups) {
    return 2 * (((n_groups + 2) * 8 + 255) & ~(size_t)255) + ((2 * n_groups * 4 + 255) & ~(size_t)255) + (rb_scan_block_sums_count(n_groups) + 4) * 8 + 256;
}
extern "C" int rb_dev_trim_select(rb_ctx *ctx, uint64_t n_rec, uint64_t n_groups, const uint32_t *order, const uint64_t *grp_off,
                                  const rb_norm_row *norm_rows, uint64_t out_base, uint8_t *contained, uint32_t *left, uint32_t *right,
                                  uint64_t *pair_out_off, rb_trim_pass *pass, void *scratch) {
    if (!ctx || !pass || (n_groups && (!order || !grp_off || !norm_rows || !contained || !left || !right || !pair_out_off || !scratch))) return RB_E_INVALID;
    (void)n_rec;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    rb_tsel_params p;
    memset(&p, 0, sizeof p);
    char *sc = (char *)scratch;
    p.n_groups = n_groups, p.order = order, p.grp_off = grp_off, p.norm = norm_rows, p.contained = contained;
    p.slot = (uint64_t *)sc;
    sc += ((n_groups + 2) * 8 + 255) & ~(size_t)255;
    p.has = (uint64_t *)sc;
    sc += ((n_groups + 2) * 8 + 255) & ~(size_t)255;
    p.cand = (uint32_t *)sc;
    sc += (2 * n_groups * 4 + 255) & ~(size_t)255;
    p.out_base = out_base, p.left = left, p.right = right, p.pair_out_off = pair_out_off, p.pass = pass;
    HIPCHK(ctx, rb_launch_trim_select(&p, (uint64_t *)sc, ctx->stream));
    return RB_OK;
}
extern "C" int rb_dev_trim_check(rb_ctx *ctx, uint64_t n_pairs, const rb_pair_row *rows, rb_trim_pass *pass) {
    if (!ctx || !pass || (n_pairs && !rows)) return RB_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, rb_launch_trim_check(rows, n_pairs, pass, ctx->stream));
    return RB_OK;
}
extern "C" int rb_dev_apply_pairs(rb_ctx *ctx, uint64_t n_pairs, const uint32_t *left, const uint32_t *right, const rb_pair_row *rows,
                                  uint64_t *op_off, rb_norm_row *norm_rows) {
    if (!ctx || (n_pairs && (!left || !right || !rows || !op_off || !norm_rows))) return RB_E_INVALID;
    rb_apply_params p{n_pairs, left, right, rows, op_off, norm_rows};
    HIPCHK(ctx, rb_launch_apply_pairs(&p, ctx->stream));
    return RB_OK;
}
extern "C" int rb_dev_gather_records(rb_ctx *ctx, uint64_t n_rec, const uint32_t *ops, const uint64_t *op_off, const rb_norm_row *norm_rows,
                                     uint64_t *new_op_off, uint32_t *new_ops, void *scratch) {
    if (!ctx || !new_op_off || !scratch || (n_rec && (!ops || !op_off || !norm_rows))) return RB_E_INVALID;
    rb_gather_params p{n_rec, ops, op_off, norm_rows, new_op_off, new_ops, 0};
    HIPCHK(ctx, rb_fill_async(new_op_off + n_rec, 0, 8, ctx->stream));
    if (n_rec == 0) return RB_OK;
    HIPCHK(ctx, rb_launch_gather_records(&p, ctx->stream));
    HIPCHK(ctx, rb_launch_exclusive_scan(new_op_off, n_rec, (uint64_t *)scratch, nullptr, ctx->stream));
    if (new_ops) { // (NULL: sizes only -- new_op_off[n_rec] says how many ops the dense batch holds)
        p.fill = 1;
        HIPCHK(ctx, rb_launch_gather_records(&p, ctx->stream));
    }
    return RB_OK;
}

// ---- liftover --largest ---------------------------------------------------------------------------
// scratch of rb_dev_largest: [best_span (n_keys + 1) u64][best_row n_keys u64][block sums of the scan]
static size_t largest_span_bytes(uint64_t n_keys) { return ((size_t)(n_keys + 1) * 8 + 255) & ~(size_t)255; }
static size_t largest_row_bytes(uint64_t n_keys) { return ((size_t)n_keys * 8 + 255) & ~(size_t)255; }
extern "C" size_t rb_largest_scratch_bytes(uint64_t n_keys) {
    return largest_span_bytes(n_keys) + largest_row_bytes(n_keys) + (rb_scan_block_sums_count(n_keys) + 4) * 8;
}
// worst_status: NULL, or 4 bytes of device memory for the largest panic status among all rows (rb_launch.h)
static int largest_impl(rb_ctx *ctx, const rb_hit_row *rows, uint64_t n_rows, const uint32_t *win_key, const uint32_t *rec_key, uint64_t n_keys,
                        uint64_t *sel, uint64_t *out, void *scratch, uint32_t *worst_status) {
    if (!ctx || !out || (n_rows && (!rows || !win_key)) || (n_keys && (!sel || !scratch))) return RB_E_INVALID;
    if (((uintptr_t)rows & 15u) != 0) return fail(ctx, RB_E_INVALID, "rows must be 16-byte aligned");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    rb_largest_params p;
    memset(&p, 0, sizeof p);
    char *sc = (char *)scratch;
    p.rows = rows, p.n_rows = n_rows, p.win_key = win_key, p.rec_key = rec_key, p.n_keys = n_keys;
    p.best_span = (unsigned long long *)sc;
    p.best_row = (unsigned long long *)(sc + largest_span_bytes(n_keys));
    p.sel = sel, p.out = (unsigned long long *)out, p.worst_status = worst_status;
    HIPCHK(ctx, rb_fill_async(out, 0, 16, ctx->stream));
    if (worst_status) HIPCHK(ctx, rb_fill_async(worst_status, 0, 4, ctx->stream));
    if (n_keys) HIPCHK(ctx, rb_fill_async(sc, 0, largest_span_bytes(n_keys) + largest_row_bytes(n_keys), ctx->stream)); // (every call: nothing of the last one counts)
    HIPCHK(ctx, rb_launch_largest(&p, (uint64_t *)(sc + largest_span_bytes(n_keys) + largest_row_bytes(n_keys)), ctx->stream));
    return RB_OK;
}
extern "C" int rb_dev_largest(rb_ctx *ctx, const rb_hit_row *rows, uint64_t n_rows, const uint32_t *win_key, const uint32_t *rec_key,
                              uint64_t n_keys, uint64_t *sel, uint64_t *out, void *scratch) {
    return largest_impl(ctx, rows, n_rows, win_key, rec_key, n_keys, sel, out, scratch, nullptr);
}

// ---- CIGAR text ----------------------------------------------------------------------------------
extern "C" size_t rb_text_scratch_bytes(uint64_t n) { return (rb_scan_block_sums_count(n) + 4) * 8; }
extern "C" int rb_dev_parse_cigars(rb_ctx *ctx, const uint8_t *text, const uint64_t *text_off, const uint64_t *text_end, uint64_t n_rec,
                                   uint64_t *op_off, uint32_t *ops, uint64_t ops_cap, uint8_t *status, void *scratch) {
    if (!ctx || !text_off || !op_off || !status || !scratch || (n_rec && !text)) return RB_E_INVALID;
    if (((uintptr_t)text & 15u) != 0) return fail(ctx, RB_E_INVALID, "text must be 16-byte aligned");
    rb_parse_params p;
    p.n_rec = n_rec;
    p.text = text;
    p.text_off = text_off;
    p.text_end = text_end;
    p.op_off = op_off;
    p.ops = ops;
    p.ops_cap = ops_cap;
    p.status = status;
    HIPCHK(ctx, rb_fill_async(op_off + n_rec, 0, 8, ctx->stream));
    if (n_rec == 0) return RB_OK;
    HIPCHK(ctx, rb_launch_parse_cigars(&p, false, ctx->stream));
    HIPCHK(ctx, rb_launch_exclusive_scan(op_off, n_rec, (uint64_t *)scratch, nullptr, ctx->stream));
    HIPCHK(ctx, rb_launch_parse_cigars(&p, true, ctx->stream));
    return RB_OK;
}
// offsets_ready: text_off already holds the prefix of a sizes-only call on the same items (the host wrappers size, allocate, fill)
static int format_cigars_impl(rb_ctx *ctx, const uint32_t *ops, const uint32_t *ops_alt, uint64_t n_items, const uint64_t *first,
                              const uint32_t *count, const uint32_t *first_len, const uint32_t *last_len, uint64_t *text_off,
                              uint8_t *text, uint64_t text_cap, void *scratch, bool offsets_ready, bool plain_ops = false) {
    if (!ctx || !text_off || !scratch || (n_items && (!ops || !first || !count))) return RB_E_INVALID;
    rb_format_params p;
    p.plain_ops = plain_ops ? 1 : 0; // (the caller knows that ops[] came out of rb_k_parse_cigars: no continuation words to look for)
    p.n_items = n_items;
    p.ops = ops;
    p.ops_alt = ops_alt;
    p.first = first;
    p.count = count;
    p.first_len = first_len;
    p.last_len = last_len;
    p.text_off = text_off;
    p.text = text;
    p.text_cap = text_cap;
    if (!offsets_ready) HIPCHK(ctx, rb_fill_async(text_off + n_items, 0, 8, ctx->stream));
    if (n_items == 0) return RB_OK;
    if (!offsets_ready) {
        HIPCHK(ctx, rb_launch_format_cigars(&p, false, ctx->stream));
        HIPCHK(ctx, rb_launch_exclusive_scan(text_off, n_items, (uint64_t *)scratch, nullptr, ctx->stream));
    }
    if (text) HIPCHK(ctx, rb_launch_format_cigars(&p, true, ctx->stream));
    return RB_OK;
}
extern "C" int rb_dev_format_cigars(rb_ctx *ctx, const uint32_t *ops, const uint32_t *ops_alt, uint64_t n_items, const uint64_t *first,
                                    const uint32_t *count, const uint32_t *first_len, const uint32_t *last_len, uint64_t *text_off,
                                    uint8_t *text, uint64_t text_cap, void *scratch) {
    return format_cigars_impl(ctx, ops, ops_alt, n_items, first, count, first_len, last_len, text_off, text, text_cap, scratch, false);
}

// gigabyte-sized host buffers: ask for huge pages where the system lets a process opt in (transparent_hugepage = madvise): a
// 2 GB buffer is then a thousand faults and a thousand pages to free instead of half a million of each
static void rb_advise_huge(void *p, size_t bytes) {
    if (!p || bytes < ((size_t)8 << 20)) return;
    const uintptr_t a = ((uintptr_t)p + ((size_t)2 << 20) - 1) & ~(uintptr_t)(((size_t)2 << 20) - 1), e = ((uintptr_t)p + bytes) & ~(uintptr_t)(((size_t)2 << 20) - 1);
    if (e > a) (void)madvise((void *)a, (size_t)(e - a), MADV_HUGEPAGE);
}
// ---- host-buffer wrappers ----------------------------------------------------------------------
namespace {
struct DevBatch {
    rb_ctx *ctx;
    rb_batch_view v{};
    std::vector<void *> owned;
    explicit DevBatch(rb_ctx *c) : ctx(c) {}
    ~DevBatch() {
        for (void *q : owned) (void)rb_dev_free(ctx, q);
    }
    template <typename T>
    int up(const T *host, size_t n, const T **dev) {
        void *d = nullptr;
        int rc = rb_dev_alloc(ctx, n * sizeof(T) + 256, &d); // (the kernels read whole 128-byte lines of the ops)
        if (rc) return rc;
        owned.push_back(d);
        if (host && n) rc = rb_dev_upload(ctx, d, host, n * sizeof(T));
        *dev = (const T *)d;
        return rc;
    }
    template <typename T>
    int alloc(size_t n, T **dev) {
        void *d = nullptr;
        int rc = rb_dev_alloc(ctx, n * sizeof(T) + 64, &d);
        if (rc) return rc;
        owned.push_back(d);
        *dev = (T *)d;
        return RB_OK;
    }
    int load(uint64_t n_rec, const uint32_t *ops, const uint64_t *op_off, const uint64_t *t_st, const uint64_t *t_en,
             const uint64_t *q_st, const uint64_t *q_en, const uint8_t *strand, const uint32_t *contig) {
        v.n_rec = n_rec;
        v.n_ops = n_rec ? op_off[n_rec] : 0;
        int rc = RB_OK;
        std::vector<uint32_t> zc;
        std::vector<uint8_t> zs;
        if (!contig) {
            zc.assign(n_rec, 0);
            contig = zc.data();
        }
        if (!strand) {
            zs.assign(n_rec, (uint8_t)'+');
            strand = zs.data();
        }
        if (!rc) rc = up(ops, (size_t)v.n_ops + 4, &v.ops);
        if (!rc) rc = up(op_off, (size_t)n_rec + 1, &v.op_off);
        if (!rc) rc = up(t_st, (size_t)n_rec, &v.t_st);
        if (!rc) rc = up(t_en, (size_t)n_rec, &v.t_en);
        if (!rc) rc = up(q_st, (size_t)n_rec, &v.q_st);
        if (!rc) rc = up(q_en, (size_t)n_rec, &v.q_en);
        if (!rc) rc = up(strand, (size_t)n_rec, &v.strand);
        if (!rc) rc = up(contig, (size_t)n_rec, &v.contig);
        if (!rc) rc = rb_ctx_sync(ctx); // the temporaries above must outlive the copies
        return rc;
    }
};
// ---- the arguments of the text entry points (rb_host_*_text), stated once.  An extern wrapper fills the packs by brace-initialisation in
// the order of its own parameter list; the internal functions take them by reference.
struct text_cols { // the input columns
    uint64_t n_rec;
    const uint8_t *text;
    uint64_t text_bytes;
    const uint64_t *cig_off, *cig_end, *t_st, *t_en, *q_st, *q_en;
    const uint8_t *strand;
    const uint32_t *contig;
};
struct text_wins { // the windows (value-initialised: a break route has none)
    uint64_t n_win;
    const uint32_t *w_contig;
    const uint64_t *w_st, *w_en;
};
struct text_outs { // the outputs; a stats form passes stats and no row_text_off / row_text, rb_host_scan_text passes the first three alone
    uint8_t *cig_status;
    rb_reduce_row *reduce_out;
    rb_norm_row *norm_out;
    rb_hit_row **rows;
    uint64_t *n_rows, **row_text_off;
    uint8_t **row_text;
    rb_reduce_row **stats;
    rb_counters *counters;
    // storage of the pack's own for what such a caller does not pass (text_front_of points there; nothing is ever allocated into it)
    rb_hit_row *own_rows = nullptr;
    uint64_t own_n = 0, *own_off = nullptr;
    uint8_t *own_text = nullptr;
    void drop() { // an error behind the point where the results were allocated: the caller gets none of them
        free(*rows), free(*row_text_off), free(*row_text);
        *rows = nullptr, *row_text_off = nullptr, *row_text = nullptr, *n_rows = 0;
        if (stats) free(*stats), *stats = nullptr;
    }
    int finish(int rc, uint64_t n, const rb_counters &hc) { // the end of a route: the counts with the results, or no results
        if (rc) drop();
        else *n_rows = n;
        if (!rc && counters) *counters = hc;
        return rc;
    }
};
} // namespace

extern "C" void rb_host_free(void *p) { free(p); }

extern "C" int rb_host_scan_records(rb_ctx *ctx, uint64_t n_rec, const uint32_t *ops, const uint64_t *op_off, const uint64_t *t_st,
                                    const uint64_t *t_en, const uint64_t *q_st, const uint64_t *q_en, const uint8_t *strand,
                                    rb_reduce_row *reduce_rows, rb_norm_row *norm_rows) {
    if (!ctx) return RB_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevBatch b(ctx);
    int rc = b.load(n_rec, ops, op_off, t_st, t_en, q_st, q_en, strand, nullptr);
    if (rc) return rc;
    rb_reduce_row *d_red = nullptr;
    rb_norm_row *d_norm = nullptr;
    if (reduce_rows && (rc = b.alloc(n_rec, &d_red))) return rc;
    if (norm_rows && (rc = b.alloc(n_rec, &d_norm))) return rc;
    if ((rc = rb_dev_scan_records(ctx, &b.v, d_red, d_norm))) return rc;
    if (reduce_rows && (rc = rb_dev_download(ctx, reduce_rows, d_red, n_rec * sizeof(rb_reduce_row)))) return rc;
    if (norm_rows && (rc = rb_dev_download(ctx, norm_rows, d_norm, n_rec * sizeof(rb_norm_row)))) return rc;
    return rb_ctx_sync(ctx);
}

static double rb_now_s() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + 1e-9 * ts.tv_nsec;
}
static void rb_lap(const char *what, double &t) {
    static const bool on = getenv("RB_TIMING") != nullptr;
    const double n = rb_now_s();
    if (on) fprintf(stderr, "[rb timing]     %-24s %.3f s\n", what, n - t);
    t = n;
}
// Plan, workspace, rows and clips for one liftover / break-paf call on a device-resident batch: the clip kernels are run again with
// larger outputs while the counters say they overflowed (at most 6 attempts).  The rows and clips of the last attempt go with the batch
// (*d_rows, *d_out); the plan and the workspace are freed here.
static int lift_sized(rb_ctx *ctx, DevBatch &b, const uint64_t *op_off, const uint32_t *contig, uint64_t n_win, const uint32_t *w_contig,
                      const uint64_t *w_st, const uint64_t *w_en, const rb_norm_row *d_norm, bool is_break, uint32_t max_size, int policy,
                      rb_hit_row **d_rows, uint32_t **d_out, rb_counters *hc, double &tl) {
    memset(hc, 0, sizeof *hc);
    rb_plan *plan = nullptr;
    int rc = rb_plan_create(ctx, b.v.n_rec, op_off, contig, n_win, w_contig, w_st, w_en, &plan);
    if (rc) return rc;
    rb_lap("plan", tl);
    rb_counters *d_cnt = nullptr;
    rc = b.alloc(1, &d_cnt);
    const bool desc = (policy & RB_LIFT_DESCRIPTORS) != 0;
    uint64_t rows_cap = 16 * b.v.n_rec + n_win + 1024; // a first guess; the counters say what is needed if it is short
    uint64_t out_cap = (desc ? b.v.n_ops / 4 : rb_plan_out_capacity(plan, is_break ? 1 : 0)) + 16 * rows_cap + 4096;
    void *ws = nullptr;
    rb_hit_row *rows = nullptr;
    uint32_t *out = nullptr;
    for (int attempt = 0; !rc && attempt < 6; attempt++) {
        for (void *q : {ws, (void *)rows, (void *)out})
            if (q) (void)rb_dev_free(ctx, q);
        ws = nullptr, rows = nullptr, out = nullptr;
        rc = rb_dev_alloc(ctx, rb_plan_workspace_bytes(plan, rows_cap), &ws);
        if (!rc) rc = rb_dev_alloc(ctx, (rows_cap + 1) * sizeof(rb_hit_row), (void **)&rows);
        if (!rc) rc = rb_dev_alloc(ctx, (out_cap + 4) * 4, (void **)&out);
        if (!rc)
            rc = is_break ? rb_dev_break(ctx, plan, &b.v, d_norm, max_size, policy | (desc ? 0 : RB_BREAK_ONE_WALK), ws, rows, rows_cap, out, out_cap, d_cnt)
                          : rb_dev_liftover(ctx, plan, &b.v, d_norm, policy, ws, rows, rows_cap, out, out_cap, d_cnt);
        if (!rc) rc = rb_dev_download(ctx, hc, d_cnt, sizeof *hc);
        if (rc || !hc->overflow) break;
        rows_cap = std::max<uint64_t>(rows_cap, hc->n_hits + 16);
        out_cap = std::max<uint64_t>(out_cap * 2, hc->out_ops_needed + hc->out_ops_needed / 4 + 4096 + 4 * rows_cap);
    }
    if (!rc && hc->overflow) rc = RB_E_CAPACITY;
    if (ws) (void)rb_dev_free(ctx, ws);
    rb_plan_destroy(plan);
    for (void *q : {(void *)rows, (void *)out})
        if (q) b.owned.push_back(q);
    *d_rows = rows, *d_out = out;
    rb_lap("alloc + kernels", tl);
    return rc;
}
static int host_lift(rb_ctx *ctx, bool is_break, uint32_t max_size, uint64_t n_rec, const uint32_t *ops, const uint64_t *op_off,
                     const uint64_t *t_st, const uint64_t *t_en, const uint64_t *q_st, const uint64_t *q_en, const uint8_t *strand,
                     const uint32_t *contig, uint64_t n_win, const uint32_t *w_contig, const uint64_t *w_st, const uint64_t *w_en,
                     int policy, rb_norm_row *norm_out, rb_hit_row **rows, uint64_t *n_rows, uint32_t **out_ops, uint64_t *n_out,
                     rb_counters *counters) {
    if (!ctx || !rows || !n_rows || !out_ops || !n_out) return RB_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    *rows = nullptr;
    *out_ops = nullptr;
    *n_rows = *n_out = 0;
    DevBatch b(ctx);
    std::vector<uint32_t> zc;
    if (!contig) {
        zc.assign(n_rec, 0);
        contig = zc.data();
    }
    double tl = rb_now_s();
    int rc = b.load(n_rec, ops, op_off, t_st, t_en, q_st, q_en, strand, contig);
    if (rc) return rc;
    rb_lap("H2D batch", tl);
    rb_norm_row *d_norm = nullptr;
    if ((rc = b.alloc(n_rec, &d_norm))) return rc;
    const bool fused = (policy & RB_LIFT_FUSED_SCAN) != 0; // the clip kernel verifies the records itself
    if (!fused) {
        if ((rc = rb_dev_scan_records(ctx, &b.v, nullptr, d_norm))) return rc;
        if (norm_out && (rc = rb_dev_download(ctx, norm_out, d_norm, n_rec * sizeof(rb_norm_row)))) return rc;
        rb_lap("scan_records + norm D2H", tl);
    }
    rb_counters hc;
    rb_hit_row *d_rows = nullptr;
    uint32_t *d_out = nullptr;
    rc = lift_sized(ctx, b, op_off, contig, n_win, w_contig, w_st, w_en, d_norm, is_break, max_size, policy, &d_rows, &d_out, &hc, tl);
    if (!rc && fused && norm_out) rc = rb_dev_download(ctx, norm_out, d_norm, n_rec * sizeof(rb_norm_row));
    if (!rc) {
        // the clips packed side by side in row order ON THE DEVICE (the slots of out_ops are as large as the batch: only the clips
        // themselves cross PCIe), rows' out_off rebased onto the dense array
        *n_rows = hc.n_hits;
        *rows = (rb_hit_row *)malloc((size_t)(hc.n_hits + 1) * sizeof(rb_hit_row));
        uint64_t o = 0;
        if (hc.n_hits) {
            uint64_t *d_off = nullptr, *d_blk = nullptr;
            uint32_t *d_dense = nullptr;
            rc = rb_dev_alloc(ctx, (hc.n_hits + 2) * 8, (void **)&d_off);
            if (!rc) rc = rb_dev_alloc(ctx, (rb_scan_block_sums_count(hc.n_hits) + 2) * 8, (void **)&d_blk);
            rb_compact_params cp{hc.n_hits, d_rows, d_out, d_off, nullptr, 0};
            if (!rc && rb_launch_compact_clips(&cp, ctx->stream) != hipSuccess) rc = RB_E_HIP;
            if (!rc && rb_launch_exclusive_scan(d_off, hc.n_hits, d_blk, d_off + hc.n_hits, ctx->stream) != hipSuccess) rc = RB_E_HIP;
            if (!rc) rc = rb_dev_download(ctx, &o, d_off + hc.n_hits, 8);
            if (!rc) rc = rb_dev_alloc(ctx, (o + 4) * 4, (void **)&d_dense);
            cp.dst = d_dense, cp.fill = 1;
            if (!rc && rb_launch_compact_clips(&cp, ctx->stream) != hipSuccess) rc = RB_E_HIP;
            if (!rc) rc = rb_dev_download(ctx, *rows, d_rows, (size_t)hc.n_hits * sizeof(rb_hit_row));
            *out_ops = (uint32_t *)malloc((size_t)(o + 1) * 4);
            if (!rc && o) rc = rb_dev_download(ctx, *out_ops, d_dense, (size_t)o * 4);
            if (d_off) (void)rb_dev_free(ctx, d_off);
            if (d_blk) (void)rb_dev_free(ctx, d_blk);
            if (d_dense) (void)rb_dev_free(ctx, d_dense);
            for (uint64_t i = 0; i < hc.n_hits && !rc; i++) // (rows that carry no clip: the fields the reference has no value for)
                if ((*rows)[i].status != RB_ST_OK) (*rows)[i].out_off = 0, (*rows)[i].out_n = 0;
        } else {
            *out_ops = (uint32_t *)malloc(4);
        }
        *n_out = o;
        if (counters) *counters = hc;
        rb_lap("D2H + compact", tl);
    }
    if (rc) {
        free(*rows);
        free(*out_ops);
        *rows = nullptr;
        *out_ops = nullptr;
        *n_rows = *n_out = 0;
    }
    return rc;
}

extern "C" int rb_host_liftover(rb_ctx *ctx, uint64_t n_rec, const uint32_t *ops, const uint64_t *op_off, const uint64_t *t_st,
                                const uint64_t *t_en, const uint64_t *q_st, const uint64_t *q_en, const uint8_t *strand,
                                const uint32_t *contig, uint64_t n_win, const uint32_t *w_contig, const uint64_t *w_st,
                                const uint64_t *w_en, int policy, rb_norm_row *norm_out, rb_hit_row **rows, uint64_t *n_rows,
                                uint32_t **out_ops, uint64_t *n_out, rb_counters *counters) {
    return host_lift(ctx, false, 0, n_rec, ops, op_off, t_st, t_en, q_st, q_en, strand, contig, n_win, w_contig, w_st, w_en, policy,
                     norm_out, rows, n_rows, out_ops, n_out, counters);
}
extern "C" int rb_host_break(rb_ctx *ctx, uint64_t n_rec, const uint32_t *ops, const uint64_t *op_off, const uint64_t *t_st,
                             const uint64_t *t_en, const uint64_t *q_st, const uint64_t *q_en, const uint8_t *strand, uint32_t max_size,
                             int policy, rb_norm_row *norm_out, rb_hit_row **rows, uint64_t *n_rows, uint32_t **out_ops,
                             uint64_t *n_out, rb_counters *counters) {
    return host_lift(ctx, true, max_size, n_rec, ops, op_off, t_st, t_en, q_st, q_en, strand, nullptr, 0, nullptr, nullptr, nullptr,
                     policy, norm_out, rows, n_rows, out_ops, n_out, counters);
}

extern "C" int rb_host_parse_cigars(rb_ctx *ctx, const uint8_t *text, const uint64_t *text_off, const uint64_t *text_end, uint64_t n_rec,
                                    uint64_t *op_off, uint32_t **ops, uint8_t *status) {
    if (!ctx || !text_off || !op_off || !ops || !status) return RB_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    *ops = nullptr;
    uint64_t text_bytes = 0;
    for (uint64_t r = 0; r < n_rec; r++) text_bytes = std::max(text_bytes, text_end ? text_end[r] : text_off[r + 1]);
    DevBatch b(ctx);
    const uint8_t *d_text = nullptr;
    const uint64_t *d_off = nullptr, *d_end = nullptr;
    uint64_t *d_opoff = nullptr;
    uint32_t *d_ops = nullptr;
    uint8_t *d_status = nullptr;
    void *d_scr = nullptr;
    int rc;
    {
        uint8_t *t = nullptr;
        if ((rc = b.alloc((size_t)text_bytes + 32, &t))) return rc;
        if (text_bytes && (rc = rb_dev_upload(ctx, t, text, (size_t)text_bytes))) return rc;
        d_text = t;
    }
    if ((rc = b.up(text_off, (size_t)n_rec + 1, &d_off))) return rc;
    if (text_end && (rc = b.up(text_end, (size_t)n_rec, &d_end))) return rc;
    const uint64_t ops_cap = text_bytes / 2 + 4;
    if ((rc = b.alloc((size_t)n_rec + 2, &d_opoff))) return rc;
    if ((rc = b.alloc((size_t)ops_cap, &d_ops))) return rc;
    if ((rc = b.alloc((size_t)n_rec + 1, &d_status))) return rc;
    if ((rc = b.alloc(rb_text_scratch_bytes(n_rec), (uint8_t **)&d_scr))) return rc;
    if ((rc = rb_dev_parse_cigars(ctx, d_text, d_off, d_end, n_rec, d_opoff, d_ops, ops_cap, d_status, d_scr))) return rc;
    if ((rc = rb_dev_download(ctx, op_off, d_opoff, ((size_t)n_rec + 1) * 8))) return rc;
    if (n_rec && (rc = rb_dev_download(ctx, status, d_status, (size_t)n_rec))) return rc;
    const uint64_t n_ops = op_off[n_rec];
    *ops = (uint32_t *)malloc(((size_t)n_ops + 4) * 4);
    if (!*ops) return fail(ctx, RB_E_NOMEM, "malloc(%llu ops)", (unsigned long long)n_ops);
    if (n_ops) return rb_dev_download(ctx, *ops, d_ops, (size_t)n_ops * 4);
    return RB_OK;
}
extern "C" int rb_host_format_cigars(rb_ctx *ctx, const uint32_t *ops, uint64_t n_ops, uint64_t n_items, const uint64_t *first,
                                     const uint32_t *count, const uint32_t *first_len, const uint32_t *last_len, uint64_t *text_off,
                                     uint8_t **text) {
    if (!ctx || !text_off || !text || (n_items && (!first || !count))) return RB_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    *text = nullptr;
    for (uint64_t i = 0; i < n_items; i++)
        if (first[i] + count[i] > n_ops) return fail(ctx, RB_E_INVALID, "item %llu reaches past the ops", (unsigned long long)i);
    DevBatch b(ctx);
    const uint32_t *d_ops = nullptr, *d_count = nullptr, *d_fl = nullptr, *d_ll = nullptr;
    const uint64_t *d_first = nullptr;
    uint64_t *d_toff = nullptr;
    uint8_t *d_text = nullptr;
    void *d_scr = nullptr;
    int rc;
    if ((rc = b.up(ops, (size_t)n_ops, &d_ops))) return rc;
    if ((rc = b.up(first, (size_t)n_items, &d_first))) return rc;
    if ((rc = b.up(count, (size_t)n_items, &d_count))) return rc;
    if (first_len && (rc = b.up(first_len, (size_t)n_items, &d_fl))) return rc;
    if (last_len && (rc = b.up(last_len, (size_t)n_items, &d_ll))) return rc;
    if ((rc = b.alloc((size_t)n_items + 2, &d_toff))) return rc;
    if ((rc = b.alloc(rb_text_scratch_bytes(n_items), (uint8_t **)&d_scr))) return rc;
    if ((rc = rb_dev_format_cigars(ctx, d_ops, nullptr, n_items, d_first, d_count, d_fl, d_ll, d_toff, nullptr, 0, d_scr))) return rc; // sizes
    if ((rc = rb_dev_download(ctx, text_off, d_toff, ((size_t)n_items + 1) * 8))) return rc;
    const uint64_t bytes = text_off[n_items];
    if ((rc = b.alloc((size_t)bytes + 16, &d_text))) return rc;
    if ((rc = format_cigars_impl(ctx, d_ops, nullptr, n_items, d_first, d_count, d_fl, d_ll, d_toff, d_text, bytes, d_scr, true))) return rc;
    *text = (uint8_t *)malloc((size_t)bytes + 16);
    if (!*text) return fail(ctx, RB_E_NOMEM, "malloc(%llu text bytes)", (unsigned long long)bytes);
    rb_advise_huge(*text, (size_t)bytes);
    if (bytes) return rb_dev_download(ctx, *text, d_text, (size_t)bytes);
    return RB_OK;
}

// What the front of a text route leaves for the rest of it: the batch's op offsets on the host, the contig ids its plan is made with (the
// caller's, or zc: every record on contig 0), the record scan's buffers (they go with the batch), the lap clock.  done: the call is over.
struct text_front {
    std::vector<uint64_t> op_off;
    std::vector<uint32_t> zc;
    const uint32_t *contig = nullptr, *d_contig = nullptr;
    rb_norm_row *d_norm = nullptr;
    rb_reduce_row *d_red = nullptr;
    double tl = 0;
    bool done = true;
};
// The records' `cg:Z:` values parsed on the device, and the batch b.v made of them and of the uploaded columns (f.op_off: its offsets on
// the host; f.contig NULL: every record on contig 0, f.zc then holds the ids).  *parsed = false: a CIGAR did not parse (cig_status says
// which), nothing else was done.
static int text_to_batch(rb_ctx *ctx, DevBatch &b, const text_cols &c, uint8_t *cig_status, text_front &f, bool *parsed) {
    const uint64_t n_rec = c.n_rec, text_bytes = c.text_bytes, *cig_off = c.cig_off, *cig_end = c.cig_end;
    int rc;
    *parsed = false;
    // ---- text -> ops on the device ----
    uint8_t *d_text = nullptr, *d_status = nullptr;
    const uint64_t *d_coff = nullptr, *d_cend = nullptr;
    uint64_t *d_opoff = nullptr;
    uint32_t *d_ops = nullptr;
    void *d_scr = nullptr;
    if ((rc = b.alloc((size_t)text_bytes + 32, &d_text))) return rc;
    if (text_bytes && (rc = rb_dev_upload(ctx, d_text, c.text, (size_t)text_bytes))) return rc;
    if ((rc = b.up(cig_off, (size_t)n_rec, &d_coff))) return rc;
    if ((rc = b.up(cig_end, (size_t)n_rec, &d_cend))) return rc;
    uint64_t cig_bytes = 0;
    for (uint64_t r = 0; r < n_rec; r++) {
        if (cig_end[r] < cig_off[r] || cig_end[r] > text_bytes) return fail(ctx, RB_E_INVALID, "record %llu: CIGAR range outside the text", (unsigned long long)r);
        cig_bytes += cig_end[r] - cig_off[r];
    }
    const uint64_t ops_cap = cig_bytes / 2 + 8;
    if ((rc = b.alloc((size_t)n_rec + 2, &d_opoff))) return rc;
    if ((rc = b.alloc((size_t)ops_cap + 4, &d_ops))) return rc;
    if ((rc = b.alloc((size_t)n_rec + 1, &d_status))) return rc;
    if ((rc = b.alloc(rb_text_scratch_bytes(n_rec), (uint8_t **)&d_scr))) return rc;
    rb_lap("H2D text", f.tl);
    if ((rc = rb_dev_parse_cigars(ctx, d_text, d_coff, d_cend, n_rec, d_opoff, d_ops, ops_cap, d_status, d_scr))) return rc;
    if (n_rec && (rc = rb_dev_download(ctx, cig_status, d_status, (size_t)n_rec))) return rc;
    for (uint64_t r = 0; r < n_rec; r++)
        if (cig_status[r] != RB_TEXT_OK) return RB_OK; // (*parsed stays false) the caller reports it (the reference panics at paf.rs:399)
    f.op_off.assign((size_t)n_rec + 1, 0);
    if ((rc = rb_dev_download(ctx, f.op_off.data(), d_opoff, ((size_t)n_rec + 1) * 8))) return rc;
    rb_lap("parse cigars + op_off D2H", f.tl);
    // ---- the batch, device-resident ----
    if (!f.contig) {
        f.zc.assign(n_rec, 0);
        f.contig = f.zc.data();
    }
    b.v.n_rec = n_rec;
    b.v.n_ops = f.op_off[n_rec];
    b.v.ops = d_ops;
    b.v.op_off = d_opoff;
    if ((rc = b.up(c.t_st, (size_t)n_rec, &b.v.t_st))) return rc;
    if ((rc = b.up(c.t_en, (size_t)n_rec, &b.v.t_en))) return rc;
    if ((rc = b.up(c.q_st, (size_t)n_rec, &b.v.q_st))) return rc;
    if ((rc = b.up(c.q_en, (size_t)n_rec, &b.v.q_en))) return rc;
    if ((rc = b.up(c.strand, (size_t)n_rec, &b.v.strand))) return rc;
    if ((rc = b.up(f.contig, (size_t)n_rec, &b.v.contig))) return rc;
    *parsed = true;
    return RB_OK;
}

// The front of host_lift_text and host_break_lift_text, up to and including the record scan's buffers.  text_args_ok: the null checks on
// the packs, which both make before they refuse anything else or write anything.  text_front_of: the outputs cleared, the result of an empty
// file, hipSetDevice (the one of the call), text_to_batch, d_norm / d_red.  f.done: the call is over with what is returned -- an empty
// file, or a CIGAR that did not parse (o.cig_status says which).  pipeline: the break -> liftover routes, whose plan sees every record
// on contig 0 and which always want the reduce rows.
static bool text_args_ok(const rb_ctx *ctx, const text_cols &c, const text_outs &o) {
    return ctx && (!c.n_rec || (c.cig_off && c.cig_end && o.cig_status));
}
static int text_front_of(rb_ctx *ctx, const text_cols &c, text_outs &o, bool scan_only, bool pipeline, DevBatch &b, text_front &f) {
    if (o.stats) *o.stats = nullptr;
    // (deliberate ABI behaviour: the pipeline's pair clears *counters before it parses, the others only with the empty file's result below)
    if (pipeline && o.counters) memset(o.counters, 0, sizeof *o.counters);
    if (c.n_rec == 0) { // an empty file: no rows, no text
        if (o.rows) *o.rows = nullptr;
        if (o.n_rows) *o.n_rows = 0;
        if (o.row_text) *o.row_text = nullptr;
        if (o.row_text_off) {
            *o.row_text_off = (uint64_t *)calloc(2, 8);
            if (!*o.row_text_off) return fail(ctx, RB_E_NOMEM, "malloc");
        }
        if (o.counters) memset(o.counters, 0, sizeof *o.counters);
        return RB_OK;
    }
    if (scan_only) o.rows = &o.own_rows, o.n_rows = &o.own_n;
    if (scan_only || o.stats) o.row_text_off = &o.own_off, o.row_text = &o.own_text;
    if (!o.rows || !o.n_rows || !o.row_text_off || !o.row_text) return RB_E_INVALID;
    // (deliberate ABI behaviour: *row_text_off stays NULL when a CIGAR does not parse, unlike the empty file's two zero words)
    *o.rows = nullptr, *o.row_text_off = nullptr, *o.row_text = nullptr, *o.n_rows = 0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc;
    bool parsed = false;
    f.tl = rb_now_s();
    f.contig = pipeline ? nullptr : c.contig;
    if ((rc = text_to_batch(ctx, b, c, o.cig_status, f, &parsed)) || !parsed) return rc;
    if (pipeline && c.contig && (rc = b.up(c.contig, (size_t)c.n_rec, &f.d_contig))) return rc; // (the records' own, for the pieces to inherit)
    if ((rc = b.alloc(c.n_rec, &f.d_norm))) return rc;
    if ((pipeline || o.reduce_out) && (rc = b.alloc(c.n_rec, &f.d_red))) return rc;
    f.done = false;
    return RB_OK;
}

// the rows a clip call left on the device: all of them and the call's out_ops; the rows that are printed and the descriptor of row k of
// them at take_desc[4k] (the same two unless --largest or the pairs pass selected); how many go to the host
struct tail_rows {
    const rb_hit_row *rows;
    const uint32_t *out;
    const rb_hit_row *take;
    const uint32_t *take_desc;
    uint64_t n;
};
// The tail of the text wrappers: the hit rows of a clip call in descriptor mode on the device-resident batch b.v (op_off: its offsets on the
// host) go to the host -- with the stats of every row's clip where it lies (o.stats != NULL: rb_dev_stats_rows, no text), or with the clipped
// CIGAR of every row printed on the device (rb_dev_format_cigars).  plain_ops: b.v.ops hold no continuation words.  rc: what the calls in
// front returned (nothing is done if it is not RB_OK).
static int lift_text_tail(rb_ctx *ctx, DevBatch &b, const uint64_t *op_off, int rc, const tail_rows &t, const rb_counters &hc, bool plain_ops, text_outs &o,
                          double &tl) {
    const uint64_t nr = t.n;
    if (o.stats) { // ---- the stats of every row's clip where it lies; rows and stats to the host, no text ----
        rb_reduce_row *d_stats = nullptr;
        if (!rc) rc = b.alloc((size_t)nr + 1, &d_stats);
        if (!rc) rc = rb_dev_stats_rows(ctx, &b.v, t.rows, nr, t.out, d_stats);
        if (!rc) {
            *o.rows = (rb_hit_row *)malloc((size_t)(nr + 1) * sizeof(rb_hit_row));
            *o.stats = (rb_reduce_row *)malloc((size_t)(nr + 1) * sizeof(rb_reduce_row));
            if (!*o.rows || !*o.stats) rc = fail(ctx, RB_E_NOMEM, "malloc(rows)");
        }
        if (!rc && nr) rc = rb_dev_download(ctx, *o.rows, t.rows, (size_t)nr * sizeof(rb_hit_row));
        if (!rc && nr) rc = rb_dev_download(ctx, *o.stats, d_stats, (size_t)nr * sizeof(rb_reduce_row));
        rb_lap("stats rows + rows D2H", tl);
        return o.finish(rc, nr, hc);
    }
    // ---- rows to the host, clip items back to the device, text out ----
    std::vector<uint32_t> desc;
    uint64_t *d_first = nullptr, *d_toff = nullptr;
    uint32_t *d_cnt3 = nullptr; // count | first_len | last_len, three arrays of nr
    uint8_t *d_rtext = nullptr;
    if (!rc) {
        *o.rows = (rb_hit_row *)malloc((size_t)(nr + 1) * sizeof(rb_hit_row));
        *o.row_text_off = (uint64_t *)malloc((size_t)(nr + 2) * 8);
        if (!*o.rows || !*o.row_text_off) rc = fail(ctx, RB_E_NOMEM, "malloc(rows)");
    }
    if (!rc && nr) rc = rb_dev_download(ctx, *o.rows, t.take, (size_t)nr * sizeof(rb_hit_row));
    if (!rc && nr) {
        desc.resize((size_t)nr * 4);
        rc = rb_dev_download(ctx, desc.data(), t.take_desc, (size_t)nr * 16); // descriptor of row k at out_ops[4k]
    }
    rb_lap("rows D2H", tl);
    if (!rc) {
        std::vector<uint64_t> first((size_t)nr + 1, 0);
        std::vector<uint32_t> c3((size_t)nr * 3 + 1, 0);
        for (uint64_t k = 0; k < nr; k++) {
            const rb_hit_row &h = (*o.rows)[k];
            if (h.status != RB_ST_OK) continue;
            if (h.flags & RB_HIT_DESCRIPTOR) {
                const uint32_t *d = &desc[(size_t)k * 4];
                first[k] = op_off[h.rec] + d[0];
                c3[k] = d[1];
                c3[nr + k] = d[2];
                c3[2 * nr + k] = d[3];
            } else { // copied by the generic kernel
                first[k] = h.out_off | (1ull << 63);
                c3[k] = h.out_n;
            }
        }
        rc = b.alloc((size_t)nr + 1, &d_first);
        if (!rc) rc = b.alloc((size_t)nr * 3 + 1, &d_cnt3);
        if (!rc) rc = b.alloc((size_t)nr + 2, &d_toff);
        void *d_scr2 = nullptr;
        if (!rc) rc = b.alloc(rb_text_scratch_bytes(nr), (uint8_t **)&d_scr2);
        if (!rc && nr) rc = rb_dev_upload(ctx, d_first, first.data(), (size_t)nr * 8);
        if (!rc && nr) rc = rb_dev_upload(ctx, d_cnt3, c3.data(), (size_t)nr * 12);
        if (!rc) rc = rb_ctx_sync(ctx);
        if (!rc) rc = format_cigars_impl(ctx, b.v.ops, t.out, nr, d_first, d_cnt3, d_cnt3 + nr, d_cnt3 + 2 * nr, d_toff, nullptr, 0, d_scr2, false, plain_ops);
        if (!rc) rc = rb_dev_download(ctx, *o.row_text_off, d_toff, ((size_t)nr + 1) * 8);
        const uint64_t bytes = rc ? 0 : (*o.row_text_off)[nr];
        if (!rc) rc = b.alloc((size_t)bytes + 16, &d_rtext);
        if (!rc) rc = format_cigars_impl(ctx, b.v.ops, t.out, nr, d_first, d_cnt3, d_cnt3 + nr, d_cnt3 + 2 * nr, d_toff, d_rtext, bytes, d_scr2, true, plain_ops);
        if (!rc) {
            *o.row_text = (uint8_t *)malloc((size_t)bytes + 16);
            if (!*o.row_text) rc = fail(ctx, RB_E_NOMEM, "malloc(%llu text bytes)", (unsigned long long)bytes);
            else rb_advise_huge(*o.row_text, (size_t)bytes);
        }
        if (!rc && bytes) rc = rb_dev_download(ctx, *o.row_text, d_rtext, (size_t)bytes);
        rb_lap("format cigars + text D2H", tl);
    }
    return o.finish(rc, nr, hc);
}

// what rb_host_liftover_largest_text adds to rb_host_liftover_text
struct largest_text {
    const uint32_t *win_key;
    uint64_t n_keys;
    uint32_t inside_key;
    int *declined;
};
// what rb_host_break_pairs_text adds to rb_host_break_text: orient / filter over the pieces' rows before they are printed or counted
struct pairs_text {
    const uint32_t *rec_key;
    const uint64_t *rec_q_len;
    uint64_t n_keys;
    uint32_t mode;
    uint64_t paired_len, min_aln, min_query;
    uint8_t *key_flip; // [n_keys] OUT (host)
    int *declined;
};
// what selects the route of host_lift_text: liftover over the windows (lg: --largest), break-paf at max_size (pr: --orient / --paired-len),
// or the record scan alone (rb_host_scan_text)
struct text_route {
    bool is_break, scan_only;
    uint32_t max_size;
    int policy;
    const largest_text *lg;
    const pairs_text *pr;
    static text_route liftover(int policy, const largest_text *lg) { return {false, false, 0, policy, lg, nullptr}; }
    static text_route brk(uint32_t max_size, int policy, const pairs_text *pr) { return {true, false, max_size, policy, nullptr, pr}; }
    static text_route scan() { return {false, true, 0, 0, nullptr, nullptr}; }
};
// text in -> text out around the clip kernels; scan_only stops after the record scan.  lg: the hit rows stay on the device, rb_dev_largest
// picks one per key, and only those rows come back, get format items and are printed.  o.stats (the *_stats_text forms; not with lg): no
// text out -- rb_dev_stats_rows runs on the rows and clips where the clip kernels left them, and the rows come back with one reduce row each
static int host_lift_text(rb_ctx *ctx, const text_route &rt, const text_cols &c, const text_wins &w, text_outs &o) {
    if (!text_args_ok(ctx, c, o) || (o.stats && (rt.lg || rt.scan_only))) return RB_E_INVALID;
    // liftover --qbed: the wrappers' own bit, taken out before anything reaches rb_dev_liftover
    const bool qbed = (rt.policy & RB_LIFT_QBED) != 0;
    const int policy = rt.policy & ~RB_LIFT_QBED;
    if (qbed && (rt.is_break || rt.scan_only)) return fail(ctx, RB_E_INVALID, "RB_LIFT_QBED: only rb_host_liftover_text and rb_host_liftover_largest_text take it");
    const largest_text *lg = rt.lg;
    const pairs_text *pr = rt.pr;
    if (lg) *lg->declined = 0;
    if (pr) *pr->declined = 0;
    DevBatch b(ctx);
    text_front f;
    int rc = text_front_of(ctx, c, o, rt.scan_only, false, b, f);
    if (rc || f.done) return rc;
    const uint64_t n_rec = c.n_rec, n_win = w.n_win;
    double &tl = f.tl;
    uint32_t *d_ops = (uint32_t *)b.v.ops;
    rb_norm_row *d_norm = f.d_norm;
    rb_reduce_row *d_red = f.d_red;
    if (qbed) {
        // Paf::from_file's check_integrity (paf.rs:70) is the record's as read: reduce rows first, from the unswapped batch.  Then the ops
        // are swapped where they lie (the descriptors of the clip index this array), the t and q columns change places, and the scan for
        // the norm rows -- aligned_pairs' remove_trailing_indels -- sees the swapped record.
        if (o.reduce_out && (rc = rb_dev_scan_records(ctx, &b.v, d_red, nullptr))) return rc;
        if ((rc = rb_dev_swap(ctx, &b.v, d_ops))) return rc;
        std::swap(b.v.t_st, b.v.q_st), std::swap(b.v.t_en, b.v.q_en);
        if ((rc = rb_dev_scan_records(ctx, &b.v, nullptr, d_norm))) return rc;
    } else if ((rc = rb_dev_scan_records(ctx, &b.v, d_red, d_norm))) {
        return rc;
    }
    if (o.norm_out && (rc = rb_dev_download(ctx, o.norm_out, d_norm, n_rec * sizeof(rb_norm_row)))) return rc;
    if (o.reduce_out && (rc = rb_dev_download(ctx, o.reduce_out, d_red, n_rec * sizeof(rb_reduce_row)))) return rc;
    rb_lap("scan_records + rows D2H", tl);
    if (rt.scan_only) return RB_OK;
    rb_counters hc;
    rb_hit_row *d_rows = nullptr;
    uint32_t *d_out = nullptr;
    rc = lift_sized(ctx, b, f.op_off.data(), f.contig, n_win, w.w_contig, w.w_st, w.w_en, d_norm, rt.is_break, rt.max_size, policy | RB_LIFT_DESCRIPTORS,
                    &d_rows, &d_out, &hc, tl);
    uint64_t nr = hc.n_hits;
    const rb_hit_row *d_take = d_rows; // the rows that go to the host, and the descriptor of row k of them at d_take_desc[4k]
    const uint32_t *d_take_desc = d_out;
    if (!rc && lg) { // ---- one row per key ----
        const uint32_t *d_wkey = nullptr;
        uint32_t *d_rkey = nullptr, *d_sdesc = nullptr;
        uint64_t *d_sel = nullptr, *d_lout = nullptr; // d_lout: out[0], out[1] of rb_dev_largest, then the worst panic status of all rows
        rb_hit_row *d_srows = nullptr;
        void *d_lscr = nullptr;
        uint64_t lout[3] = {0, 0, 0};
        rc = b.up(lg->win_key, (size_t)n_win, &d_wkey);
        if (!rc) rc = b.alloc((size_t)n_rec, &d_rkey);
        if (!rc) rc = b.alloc((size_t)lg->n_keys + 1, &d_sel);
        if (!rc) rc = b.alloc(3, &d_lout);
        if (!rc) rc = b.alloc(rb_largest_scratch_bytes(lg->n_keys), (uint8_t **)&d_lscr);
        if (!rc && rb_launch_largest_rec_keys(d_norm, n_rec, lg->inside_key, d_rkey, ctx->stream) != hipSuccess) rc = fail(ctx, RB_E_HIP, "rb_launch_largest_rec_keys");
        if (!rc) rc = largest_impl(ctx, d_rows, nr, d_wkey, d_rkey, lg->n_keys, d_sel, d_lout, d_lscr, (uint32_t *)(d_lout + 2));
        if (!rc) rc = rb_dev_download(ctx, lout, d_lout, sizeof lout);
        if (rc) return rc;
        // every window key is inside the key space (checked by the caller of this function), so a row left out is an INSIDE row of a
        // stripped record; a panic status anywhere is the reference's panic inside trim_paf_by_rgns, before it selects anything
        if ((uint32_t)lout[2] != 0 || lout[1] != 0) {
            *lg->declined = (uint32_t)lout[2] != 0 ? 2 : 1;
            return RB_OK;
        }
        nr = lout[0];
        rc = b.alloc((size_t)nr + 1, &d_srows);
        if (!rc) rc = b.alloc((size_t)nr * 4 + 4, &d_sdesc);
        if (!rc && rb_launch_largest_gather(d_rows, d_out, d_sel, nr, d_srows, d_sdesc, ctx->stream) != hipSuccess) rc = fail(ctx, RB_E_HIP, "rb_launch_largest_gather");
        d_take = d_srows, d_take_desc = d_sdesc;
        rb_lap("largest + gather", tl);
    }
    if (!rc && pr) { // ---- orient / filter: the kept rows, dense, flipped where their pair is; the tail works on those ----
        const uint32_t *d_key = nullptr;
        const uint64_t *d_qlen = nullptr;
        rb_hit_row *d_prows = nullptr;
        uint32_t *d_pdesc = nullptr;
        uint8_t *d_flip = nullptr, *d_pscr = nullptr;
        rb_pairs_info *d_info = nullptr, info;
        rc = b.up(pr->rec_key, (size_t)n_rec, &d_key);
        if (!rc) rc = b.up(pr->rec_q_len, (size_t)n_rec, &d_qlen);
        if (!rc) rc = b.alloc((size_t)nr + 1, &d_prows);
        if (!rc) rc = b.alloc((size_t)pr->n_keys + 1, &d_flip);
        if (!rc) rc = b.alloc(1, &d_info);
        if (!rc) rc = b.alloc(rb_pairs_scratch_bytes(pr->n_keys, nr), &d_pscr);
        if (!rc) rc = rb_dev_pairs_rows(ctx, d_rows, nr, d_key, d_qlen, b.v.strand, n_rec, pr->n_keys, pr->mode, pr->paired_len, pr->min_aln, pr->min_query,
                                        d_prows, nr, d_flip, d_info, d_pscr);
        if (!rc) rc = rb_dev_download(ctx, &info, d_info, sizeof info);
        if (!rc && pr->n_keys) rc = rb_dev_download(ctx, pr->key_flip, d_flip, (size_t)pr->n_keys);
        if (rc) return rc;
        if (info.declined || info.overflow) { // (rows_cap = every row: no overflow) the record route replays the file
            *pr->declined = info.declined ? (int)info.declined : -1;
            return RB_OK;
        }
        nr = info.n_kept;
        if (!o.stats) { // (the text tail wants row k's descriptor at [4k])
            rc = b.alloc((size_t)nr * 4 + 4, &d_pdesc);
            if (!rc && rb_launch_pairs_desc(d_prows, nr, d_out, d_pdesc, ctx->stream) != hipSuccess) rc = fail(ctx, RB_E_HIP, "rb_launch_pairs_desc");
        }
        d_rows = d_prows, d_take = d_prows, d_take_desc = d_pdesc;
        rb_lap("pairs rows", tl);
    }
    return lift_text_tail(ctx, b, f.op_off.data(), rc, {d_rows, d_out, d_take, d_take_desc, nr}, hc, true, o, tl);
}

extern "C" int rb_host_liftover_text(rb_ctx *ctx, uint64_t n_rec, const uint8_t *text, uint64_t text_bytes, const uint64_t *cig_off,
                                     const uint64_t *cig_end, const uint64_t *t_st, const uint64_t *t_en, const uint64_t *q_st,
                                     const uint64_t *q_en, const uint8_t *strand, const uint32_t *contig, uint64_t n_win,
                                     const uint32_t *w_contig, const uint64_t *w_st, const uint64_t *w_en, int policy, uint8_t *cig_status,
                                     rb_reduce_row *reduce_out, rb_norm_row *norm_out, rb_hit_row **rows, uint64_t *n_rows,
                                     uint64_t **row_text_off, uint8_t **row_text, rb_counters *counters) {
    const text_cols c{n_rec, text, text_bytes, cig_off, cig_end, t_st, t_en, q_st, q_en, strand, contig};
    text_outs o{cig_status, reduce_out, norm_out, rows, n_rows, row_text_off, row_text, nullptr, counters};
    return host_lift_text(ctx, text_route::liftover(policy, nullptr), c, {n_win, w_contig, w_st, w_en}, o);
}
extern "C" int rb_host_liftover_largest_text(rb_ctx *ctx, uint64_t n_rec, const uint8_t *text, uint64_t text_bytes, const uint64_t *cig_off,
                                             const uint64_t *cig_end, const uint64_t *t_st, const uint64_t *t_en, const uint64_t *q_st,
                                             const uint64_t *q_en, const uint8_t *strand, const uint32_t *contig, uint64_t n_win,
                                             const uint32_t *w_contig, const uint64_t *w_st, const uint64_t *w_en, int policy, uint8_t *cig_status,
                                             rb_reduce_row *reduce_out, rb_norm_row *norm_out, rb_hit_row **rows, uint64_t *n_rows,
                                             uint64_t **row_text_off, uint8_t **row_text, rb_counters *counters, const uint32_t *win_key,
                                             uint64_t n_keys, uint32_t inside_key, int *declined) {
    if (!ctx || !declined || (n_win && !win_key)) return RB_E_INVALID;
    // (0xFFFFFFFF is the key the wrapper gives a stripped record: it must lie outside the key space)
    if (n_keys >= 0xFFFFFFFFull || inside_key >= n_keys) return fail(ctx, RB_E_INVALID, "inside_key %u outside the %llu keys", inside_key, (unsigned long long)n_keys);
    for (uint64_t i = 0; i < n_win; i++)
        if (win_key[i] >= n_keys) return fail(ctx, RB_E_INVALID, "window %llu: key %u outside the %llu keys", (unsigned long long)i, win_key[i], (unsigned long long)n_keys);
    const largest_text lg{win_key, n_keys, inside_key, declined};
    const text_cols c{n_rec, text, text_bytes, cig_off, cig_end, t_st, t_en, q_st, q_en, strand, contig};
    text_outs o{cig_status, reduce_out, norm_out, rows, n_rows, row_text_off, row_text, nullptr, counters};
    return host_lift_text(ctx, text_route::liftover(policy, &lg), c, {n_win, w_contig, w_st, w_en}, o);
}
extern "C" int rb_host_break_text(rb_ctx *ctx, uint64_t n_rec, const uint8_t *text, uint64_t text_bytes, const uint64_t *cig_off,
                                  const uint64_t *cig_end, const uint64_t *t_st, const uint64_t *t_en, const uint64_t *q_st,
                                  const uint64_t *q_en, const uint8_t *strand, uint32_t max_size, int policy, uint8_t *cig_status,
                                  rb_reduce_row *reduce_out, rb_norm_row *norm_out, rb_hit_row **rows, uint64_t *n_rows,
                                  uint64_t **row_text_off, uint8_t **row_text, rb_counters *counters) {
    const text_cols c{n_rec, text, text_bytes, cig_off, cig_end, t_st, t_en, q_st, q_en, strand}; // (no contig: every record on contig 0)
    text_outs o{cig_status, reduce_out, norm_out, rows, n_rows, row_text_off, row_text, nullptr, counters};
    return host_lift_text(ctx, text_route::brk(max_size, policy, nullptr), c, {}, o);
}
extern "C" int rb_host_liftover_stats_text(rb_ctx *ctx, uint64_t n_rec, const uint8_t *text, uint64_t text_bytes, const uint64_t *cig_off,
                                           const uint64_t *cig_end, const uint64_t *t_st, const uint64_t *t_en, const uint64_t *q_st,
                                           const uint64_t *q_en, const uint8_t *strand, const uint32_t *contig, uint64_t n_win,
                                           const uint32_t *w_contig, const uint64_t *w_st, const uint64_t *w_en, int policy, uint8_t *cig_status,
                                           rb_reduce_row *reduce_out, rb_norm_row *norm_out, rb_hit_row **rows, uint64_t *n_rows,
                                           rb_reduce_row **stats, rb_counters *counters) {
    if (!stats) return RB_E_INVALID;
    const text_cols c{n_rec, text, text_bytes, cig_off, cig_end, t_st, t_en, q_st, q_en, strand, contig};
    text_outs o{cig_status, reduce_out, norm_out, rows, n_rows, nullptr, nullptr, stats, counters};
    return host_lift_text(ctx, text_route::liftover(policy, nullptr), c, {n_win, w_contig, w_st, w_en}, o);
}
extern "C" int rb_host_break_stats_text(rb_ctx *ctx, uint64_t n_rec, const uint8_t *text, uint64_t text_bytes, const uint64_t *cig_off,
                                        const uint64_t *cig_end, const uint64_t *t_st, const uint64_t *t_en, const uint64_t *q_st,
                                        const uint64_t *q_en, const uint8_t *strand, uint32_t max_size, int policy, uint8_t *cig_status,
                                        rb_reduce_row *reduce_out, rb_norm_row *norm_out, rb_hit_row **rows, uint64_t *n_rows,
                                        rb_reduce_row **stats, rb_counters *counters) {
    if (!stats) return RB_E_INVALID;
    const text_cols c{n_rec, text, text_bytes, cig_off, cig_end, t_st, t_en, q_st, q_en, strand}; // (no contig: every record on contig 0)
    text_outs o{cig_status, reduce_out, norm_out, rows, n_rows, nullptr, nullptr, stats, counters};
    return host_lift_text(ctx, text_route::brk(max_size, policy, nullptr), c, {}, o);
}
static int break_pairs_text(rb_ctx *ctx, const text_cols &c, uint32_t max_size, int policy, text_outs &o, const pairs_text &pr) {
    if (!ctx || !pr.declined || (c.n_rec && (!pr.rec_key || !pr.rec_q_len || !c.strand)) || (pr.n_keys && !pr.key_flip)) return RB_E_INVALID;
    if (pr.mode & ~(uint32_t)(RB_PAIRS_ORIENT | RB_PAIRS_FILTER)) return fail(ctx, RB_E_INVALID, "mode %u: RB_PAIRS_ORIENT | RB_PAIRS_FILTER", pr.mode);
    if (pr.n_keys) memset(pr.key_flip, 0, (size_t)pr.n_keys);
    return host_lift_text(ctx, text_route::brk(max_size, policy, &pr), c, {}, o);
}
extern "C" int rb_host_break_pairs_text(rb_ctx *ctx, uint64_t n_rec, const uint8_t *text, uint64_t text_bytes, const uint64_t *cig_off,
                                        const uint64_t *cig_end, const uint64_t *t_st, const uint64_t *t_en, const uint64_t *q_st, const uint64_t *q_en,
                                        const uint8_t *strand, uint32_t max_size, int policy, uint8_t *cig_status, rb_reduce_row *reduce_out,
                                        rb_norm_row *norm_out, rb_hit_row **rows, uint64_t *n_rows, uint64_t **row_text_off, uint8_t **row_text,
                                        rb_counters *counters, const uint32_t *rec_key, const uint64_t *rec_q_len, uint64_t n_keys, uint32_t mode,
                                        uint64_t paired_len, uint64_t min_aln, uint64_t min_query, uint8_t *key_flip, int *declined) {
    const text_cols c{n_rec, text, text_bytes, cig_off, cig_end, t_st, t_en, q_st, q_en, strand}; // (no contig: every record on contig 0)
    text_outs o{cig_status, reduce_out, norm_out, rows, n_rows, row_text_off, row_text, nullptr, counters};
    const pairs_text pr{rec_key, rec_q_len, n_keys, mode, paired_len, min_aln, min_query, key_flip, declined};
    return break_pairs_text(ctx, c, max_size, policy, o, pr);
}
extern "C" int rb_host_break_pairs_stats_text(rb_ctx *ctx, uint64_t n_rec, const uint8_t *text, uint64_t text_bytes, const uint64_t *cig_off,
                                              const uint64_t *cig_end, const uint64_t *t_st, const uint64_t *t_en, const uint64_t *q_st,
                                              const uint64_t *q_en, const uint8_t *strand, uint32_t max_size, int policy, uint8_t *cig_status,
                                              rb_reduce_row *reduce_out, rb_norm_row *norm_out, rb_hit_row **rows, uint64_t *n_rows, rb_reduce_row **stats,
                                              rb_counters *counters, const uint32_t *rec_key, const uint64_t *rec_q_len, uint64_t n_keys, uint32_t mode,
                                              uint64_t paired_len, uint64_t min_aln, uint64_t min_query, uint8_t *key_flip, int *declined) {
    if (!stats) return RB_E_INVALID;
    const text_cols c{n_rec, text, text_bytes, cig_off, cig_end, t_st, t_en, q_st, q_en, strand}; // (no contig: every record on contig 0)
    text_outs o{cig_status, reduce_out, norm_out, rows, n_rows, nullptr, nullptr, stats, counters};
    const pairs_text pr{rec_key, rec_q_len, n_keys, mode, paired_len, min_aln, min_query, key_flip, declined};
    return break_pairs_text(ctx, c, max_size, policy, o, pr);
}
extern "C" int rb_host_scan_text(rb_ctx *ctx, uint64_t n_rec, const uint8_t *text, uint64_t text_bytes, const uint64_t *cig_off,
                                 const uint64_t *cig_end, const uint64_t *t_st, const uint64_t *t_en, const uint64_t *q_st,
                                 const uint64_t *q_en, const uint8_t *strand, uint8_t *cig_status, rb_reduce_row *reduce_out,
                                 rb_norm_row *norm_out) {
    const text_cols c{n_rec, text, text_bytes, cig_off, cig_end, t_st, t_en, q_st, q_en, strand};
    text_outs o{cig_status, reduce_out, norm_out}; // (no rows, no text, no counters: the pack's own storage stands in)
    return host_lift_text(ctx, text_route::scan(), c, {}, o);
}

// ---- `rb orient [--scaffold]` / `rb filter` on the records of a file (rb_host_pairs_text) -----------------------------------------------
// text_front_of (parse, the batch), rb_dev_scan_records for Paf::from_file's check_integrity and nmatch / aln_len, rb_dev_pairs_records with
// room for every record, then rb_dev_format_cigars over the kept records only -- an item per kept record: its whole CIGAR, as parsed.  There
// are no hit rows, no norm rows, no policy and no counters here, so the pack's row outputs point at its own storage.
extern "C" int rb_host_pairs_text(rb_ctx *ctx, uint64_t n_rec, const uint8_t *text, uint64_t text_bytes, const uint64_t *cig_off, const uint64_t *cig_end,
                                  const uint64_t *t_st, const uint64_t *t_en, const uint64_t *q_st, const uint64_t *q_en, const uint8_t *strand,
                                  const uint32_t *rec_key, const uint64_t *rec_q_len, uint64_t n_keys, uint32_t mode, uint64_t paired_len, uint64_t min_aln,
                                  uint64_t min_query, uint8_t *cig_status, rb_reduce_row *reduce_out, uint32_t **kept, uint64_t *n_kept, uint64_t *q_st_out,
                                  uint64_t *q_en_out, uint8_t *key_flip, uint64_t *key_order, uint64_t **row_text_off, uint8_t **row_text, int *declined) {
    const text_cols c{n_rec, text, text_bytes, cig_off, cig_end, t_st, t_en, q_st, q_en, strand}; // (no contig: every record on contig 0)
    text_outs o{cig_status, reduce_out, nullptr, nullptr, nullptr, row_text_off, row_text, nullptr, nullptr};
    o.rows = &o.own_rows, o.n_rows = &o.own_n;
    if (!text_args_ok(ctx, c, o) || !kept || !n_kept || !row_text_off || !row_text || !declined ||
        (n_rec && (!rec_key || !rec_q_len || !strand || !t_st || !t_en || !q_st || !q_en || !reduce_out || !q_st_out || !q_en_out)) ||
        (n_keys && (!key_flip || !key_order)))
        return RB_E_INVALID;
    if (mode & ~(uint32_t)(RB_PAIRS_ORIENT | RB_PAIRS_FILTER)) return fail(ctx, RB_E_INVALID, "mode %u: RB_PAIRS_ORIENT | RB_PAIRS_FILTER", mode);
    *kept = nullptr, *n_kept = 0, *declined = 0;
    if (n_keys) memset(key_flip, 0, (size_t)n_keys), memset(key_order, 0, (size_t)n_keys * 8);
    DevBatch b(ctx);
    text_front f;
    int rc = text_front_of(ctx, c, o, false, false, b, f);
    if (rc || f.done) return rc;
    double &tl = f.tl;
    if ((rc = rb_dev_scan_records(ctx, &b.v, f.d_red, nullptr))) return rc;
    if ((rc = rb_dev_download(ctx, reduce_out, f.d_red, n_rec * sizeof(rb_reduce_row)))) return rc;
    rb_lap("scan_records + rows D2H", tl);
    const uint32_t *d_key = nullptr;
    const uint64_t *d_qlen = nullptr;
    uint32_t *d_kept = nullptr;
    uint64_t *d_qs = nullptr, *d_qe = nullptr, *d_order = nullptr;
    uint8_t *d_flip = nullptr, *d_pscr = nullptr;
    rb_pairs_info *d_info = nullptr, info;
    rc = b.up(rec_key, (size_t)n_rec, &d_key);
    if (!rc) rc = b.up(rec_q_len, (size_t)n_rec, &d_qlen);
    if (!rc) rc = b.alloc((size_t)n_rec + 1, &d_kept);
    if (!rc) rc = b.alloc((size_t)n_rec + 1, &d_qs);
    if (!rc) rc = b.alloc((size_t)n_rec + 1, &d_qe);
    if (!rc) rc = b.alloc((size_t)n_keys + 1, &d_flip);
    if (!rc) rc = b.alloc((size_t)n_keys + 1, &d_order);
    if (!rc) rc = b.alloc(1, &d_info);
    if (!rc) rc = b.alloc(rb_pairs_records_scratch_bytes(n_keys, n_rec), &d_pscr);
    if (!rc) rc = rb_dev_pairs_records(ctx, b.v.t_st, b.v.t_en, b.v.q_st, b.v.q_en, b.v.strand, d_key, d_qlen, n_rec, n_keys, mode, paired_len, min_aln, min_query,
                                       d_kept, n_rec, d_qs, d_qe, d_flip, d_order, d_info, d_pscr);
    if (!rc) rc = rb_dev_download(ctx, &info, d_info, sizeof info);
    if (!rc && n_keys) rc = rb_dev_download(ctx, key_flip, d_flip, (size_t)n_keys);
    if (!rc && n_keys) rc = rb_dev_download(ctx, key_order, d_order, (size_t)n_keys * 8);
    if (!rc) rc = rb_dev_download(ctx, q_st_out, d_qs, (size_t)n_rec * 8);
    if (!rc) rc = rb_dev_download(ctx, q_en_out, d_qe, (size_t)n_rec * 8);
    if (rc) return rc;
    if (info.declined || info.overflow) { // (kept_cap = every record: no overflow) the record route replays the file
        *declined = info.declined ? (int)info.declined : -1;
        return RB_OK;
    }
    const uint64_t nk = info.n_kept;
    *kept = (uint32_t *)malloc((size_t)(nk + 1) * 4);
    *row_text_off = (uint64_t *)malloc((size_t)(nk + 2) * 8);
    if (!*kept || !*row_text_off) rc = fail(ctx, RB_E_NOMEM, "malloc(kept)");
    if (!rc && nk) rc = rb_dev_download(ctx, *kept, d_kept, (size_t)nk * 4);
    rb_lap("pairs records + columns D2H", tl);
    // ---- the kept records' CIGARs as format items, text out ----
    uint64_t *d_first = nullptr, *d_toff = nullptr;
    uint32_t *d_cnt = nullptr;
    uint8_t *d_rtext = nullptr;
    void *d_scr2 = nullptr;
    if (!rc) {
        std::vector<uint64_t> first((size_t)nk + 1, 0);
        std::vector<uint32_t> count((size_t)nk + 1, 0);
        for (uint64_t k = 0; k < nk; k++) {
            const uint32_t r = (*kept)[k];
            first[k] = f.op_off[r], count[k] = (uint32_t)(f.op_off[r + 1] - f.op_off[r]);
        }
        rc = b.alloc((size_t)nk + 1, &d_first);
        if (!rc) rc = b.alloc((size_t)nk + 1, &d_cnt);
        if (!rc) rc = b.alloc((size_t)nk + 2, &d_toff);
        if (!rc) rc = b.alloc(rb_text_scratch_bytes(nk), (uint8_t **)&d_scr2);
        if (!rc && nk) rc = rb_dev_upload(ctx, d_first, first.data(), (size_t)nk * 8);
        if (!rc && nk) rc = rb_dev_upload(ctx, d_cnt, count.data(), (size_t)nk * 4);
        if (!rc) rc = rb_ctx_sync(ctx);
    }
    if (!rc) rc = format_cigars_impl(ctx, b.v.ops, nullptr, nk, d_first, d_cnt, nullptr, nullptr, d_toff, nullptr, 0, d_scr2, false, true);
    if (!rc) rc = rb_dev_download(ctx, *row_text_off, d_toff, ((size_t)nk + 1) * 8);
    const uint64_t bytes = rc ? 0 : (*row_text_off)[nk];
    if (!rc) rc = b.alloc((size_t)bytes + 16, &d_rtext);
    if (!rc) rc = format_cigars_impl(ctx, b.v.ops, nullptr, nk, d_first, d_cnt, nullptr, nullptr, d_toff, d_rtext, bytes, d_scr2, true, true);
    if (!rc) {
        *row_text = (uint8_t *)malloc((size_t)bytes + 16);
        if (!*row_text) rc = fail(ctx, RB_E_NOMEM, "malloc(%llu text bytes)", (unsigned long long)bytes);
        else rb_advise_huge(*row_text, (size_t)bytes);
    }
    if (!rc && bytes) rc = rb_dev_download(ctx, *row_text, d_rtext, (size_t)bytes);
    rb_lap("format cigars + text D2H", tl);
    if (rc) {
        free(*kept), free(*row_text_off), free(*row_text);
        *kept = nullptr, *row_text_off = nullptr, *row_text = nullptr;
    } else {
        *n_kept = nk;
    }
    return rc;
}

// ---- `rb break-paf --max-size N in.paf | rb liftover --bed W -` as one device pipeline (rb_host_break_liftover_text / _stats_text) ------
// parse, scan, break in descriptor mode, rb_dev_rows_to_batch (the pieces as a batch: the second command's Paf::from_file), scan of the
// pieces (its check_integrity and aligned_pairs' remove_trailing_indels), a plan over the pieces, liftover in descriptor mode on the piece
// batch, and the tail of host_lift_text.  The first clip call's rows, descriptors and workspace are freed before the second call sizes its
// own.  Whatever only the record route prints right -- a panic in either stage, a piece whose own id would be _TO.<..> -- sets *declined.
static int host_break_lift_text(rb_ctx *ctx, uint32_t max_size, int policy, const text_cols &c, const text_wins &w, text_outs &o, uint32_t **row_piece,
                                int *declined) {
    if (!text_args_ok(ctx, c, o) || !o.rows || !o.n_rows || !row_piece || !declined) return RB_E_INVALID;
    if (!o.stats && (!o.row_text_off || !o.row_text)) return RB_E_INVALID;
    if (policy & RB_LIFT_QBED) return fail(ctx, RB_E_INVALID, "RB_LIFT_QBED: the break-paf | liftover pipeline lifts over target windows only");
    *row_piece = nullptr, *declined = 0;
    DevBatch b(ctx), pb(ctx); // the input batch; the piece batch
    // (break-paf's rows come in record order: its plan sees every record on contig 0, as rb_host_break_text's does; the records' own contigs
    //  go to the device beside the batch, for the pieces to inherit)
    text_front f;
    int rc = text_front_of(ctx, c, o, false, true, b, f);
    if (rc || f.done) return rc;
    const uint64_t n_rec = c.n_rec;
    double &tl = f.tl;
    rb_batch_view sv = b.v; // what rb_dev_rows_to_batch reads strand and contig from
    if (f.d_contig) sv.contig = f.d_contig;
    // ---- the first command: Paf::from_file's check_integrity, aligned_pairs, break_paf_on_indels ----
    rb_norm_row *d_norm = f.d_norm;
    std::vector<rb_norm_row> norm((size_t)n_rec);
    std::vector<rb_reduce_row> red((size_t)n_rec);
    if ((rc = rb_dev_scan_records(ctx, &b.v, f.d_red, d_norm))) return rc;
    if ((rc = rb_dev_download(ctx, norm.data(), d_norm, n_rec * sizeof(rb_norm_row)))) return rc;
    if ((rc = rb_dev_download(ctx, red.data(), f.d_red, n_rec * sizeof(rb_reduce_row)))) return rc;
    if (o.norm_out) memcpy(o.norm_out, norm.data(), n_rec * sizeof(rb_norm_row));
    if (o.reduce_out) memcpy(o.reduce_out, red.data(), n_rec * sizeof(rb_reduce_row));
    rb_lap("scan_records + rows D2H", tl);
    for (uint64_t r = 0; r < n_rec; r++)
        if (red[r].status != RB_ST_OK || norm[r].status != RB_ST_OK) { // the first command panics: before it prints (from_file), or part-way
            *declined = 1;
            return RB_OK;
        }
    auto drop = [&](DevBatch &o, void *q) { // a buffer the batch owns, given back now
        auto it = std::find(o.owned.begin(), o.owned.end(), q);
        if (it != o.owned.end()) o.owned.erase(it);
        if (q) (void)rb_dev_free(ctx, q);
    };
    rb_counters hc;
    rb_hit_row *d_rows = nullptr;
    uint32_t *d_out = nullptr;
    if ((rc = lift_sized(ctx, b, f.op_off.data(), f.contig, 0, nullptr, nullptr, nullptr, d_norm, true, max_size, policy | RB_LIFT_DESCRIPTORS, &d_rows, &d_out, &hc, tl)))
        return rc;
    // ---- the pieces as a batch ----
    rb_pieces_info info, *d_info = nullptr;
    void *d_scr = nullptr;
    if ((rc = b.alloc(1, &d_info))) return rc;
    if ((rc = b.alloc(rb_rows_to_batch_scratch_bytes(hc.n_hits), (uint8_t **)&d_scr))) return rc;
    if ((rc = rb_dev_rows_to_batch(ctx, &sv, d_rows, hc.n_hits, d_out, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, d_info, d_scr)))
        return rc;
    if ((rc = rb_dev_download(ctx, &info, d_info, sizeof info))) return rc;
    if (info.declined) {
        *declined = 1;
        return RB_OK;
    }
    const uint64_t n_p = info.n_pieces;
    if (n_p == 0) { // no record reaches the second command: no rows, no text, as for an empty file
        if (!o.stats && !(*o.row_text_off = (uint64_t *)calloc(2, 8))) return fail(ctx, RB_E_NOMEM, "malloc");
        return RB_OK;
    }
    uint32_t *p_ops = nullptr, *p_contig = nullptr, *p_parent = nullptr;
    uint64_t *p_off = nullptr, *p_c[4] = {nullptr, nullptr, nullptr, nullptr};
    uint8_t *p_strand = nullptr;
    rc = pb.alloc((size_t)info.n_ops + 64, &p_ops); // (the clip kernels read whole 128-byte lines of the ops)
    if (!rc) rc = pb.alloc((size_t)n_p + 2, &p_off);
    for (int i = 0; i < 4 && !rc; i++) rc = pb.alloc((size_t)n_p, &p_c[i]);
    if (!rc) rc = pb.alloc((size_t)n_p, &p_strand);
    if (!rc) rc = pb.alloc((size_t)n_p, &p_contig);
    if (!rc) rc = pb.alloc((size_t)n_p, &p_parent);
    if (!rc)
        rc = rb_dev_rows_to_batch(ctx, &sv, d_rows, hc.n_hits, d_out, n_p, info.n_ops, p_ops, p_off, p_c[0], p_c[1], p_c[2], p_c[3], p_strand, p_contig, p_parent,
                                  d_info, d_scr);
    std::vector<uint64_t> pop_off((size_t)n_p + 1);
    std::vector<uint32_t> pcontig((size_t)n_p), parent((size_t)n_p);
    if (!rc) rc = rb_dev_download(ctx, &info, d_info, sizeof info);
    if (!rc && (info.overflow || info.n_pieces != n_p)) rc = fail(ctx, RB_E_CAPACITY, "rb_dev_rows_to_batch: the sized call did not fit");
    if (!rc) rc = rb_dev_download(ctx, pop_off.data(), p_off, ((size_t)n_p + 1) * 8);
    if (!rc) rc = rb_dev_download(ctx, pcontig.data(), p_contig, (size_t)n_p * 4);
    if (!rc) rc = rb_dev_download(ctx, parent.data(), p_parent, (size_t)n_p * 4);
    if (rc) return rc;
    drop(b, d_rows), drop(b, d_out), drop(b, d_scr); // the first clip call's arena goes before the second one sizes its own
    rb_lap("rows -> piece batch", tl);
    pb.v.n_rec = n_p, pb.v.n_ops = info.n_ops, pb.v.ops = p_ops, pb.v.op_off = p_off;
    pb.v.t_st = p_c[0], pb.v.t_en = p_c[1], pb.v.q_st = p_c[2], pb.v.q_en = p_c[3], pb.v.strand = p_strand, pb.v.contig = p_contig;
    // ---- the second command: aligned_pairs of every piece (liftover.rs:119-121), trim_paf_by_rgns ----
    rb_norm_row *d_pnorm = nullptr;
    std::vector<rb_norm_row> pnorm((size_t)n_p);
    if ((rc = pb.alloc(n_p, &d_pnorm))) return rc;
    if ((rc = rb_dev_scan_records(ctx, &pb.v, nullptr, d_pnorm))) return rc;
    if ((rc = rb_dev_download(ctx, pnorm.data(), d_pnorm, n_p * sizeof(rb_norm_row)))) return rc;
    for (uint64_t p = 0; p < n_p; p++)
        if (pnorm[p].status != RB_ST_OK || (pnorm[p].flags & RB_F_STRIPPED)) { // a panic, or an id of the piece's own (_TO.<..>) that no row carries
            *declined = 1;
            return RB_OK;
        }
    rb_hit_row *d_rows2 = nullptr;
    uint32_t *d_out2 = nullptr;
    rc = lift_sized(ctx, pb, pop_off.data(), pcontig.data(), w.n_win, w.w_contig, w.w_st, w.w_en, d_pnorm, false, 0, policy | RB_LIFT_DESCRIPTORS, &d_rows2, &d_out2, &hc, tl);
    rc = lift_text_tail(ctx, pb, pop_off.data(), rc, {d_rows2, d_out2, d_rows2, d_out2, hc.n_hits}, hc, false, o, tl);
    if (rc) return rc;
    // ---- rows back in the input's terms: rec = the parent record, row_piece = the piece ----
    *row_piece = (uint32_t *)malloc(((size_t)*o.n_rows + 1) * 4);
    if (!*row_piece) {
        o.drop();
        return fail(ctx, RB_E_NOMEM, "malloc(row_piece)");
    }
    for (uint64_t k = 0; k < *o.n_rows; k++) {
        rb_hit_row &h = (*o.rows)[k];
        if (h.status >= RB_ST_PANIC_NOTFOUND) *declined = 1; // the second command panics inside trim_paf_by_rgns
        (*row_piece)[k] = h.rec;
        h.rec = parent[h.rec];
    }
    return RB_OK;
}
extern "C" int rb_host_break_liftover_text(rb_ctx *ctx, uint64_t n_rec, const uint8_t *text, uint64_t text_bytes, const uint64_t *cig_off,
                                           const uint64_t *cig_end, const uint64_t *t_st, const uint64_t *t_en, const uint64_t *q_st,
                                           const uint64_t *q_en, const uint8_t *strand, const uint32_t *contig, uint64_t n_win,
                                           const uint32_t *w_contig, const uint64_t *w_st, const uint64_t *w_en, uint32_t max_size, int policy,
                                           uint8_t *cig_status, rb_reduce_row *reduce_out, rb_norm_row *norm_out, rb_hit_row **rows, uint64_t *n_rows,
                                           uint64_t **row_text_off, uint8_t **row_text, rb_counters *counters, uint32_t **row_piece, int *declined) {
    const text_cols c{n_rec, text, text_bytes, cig_off, cig_end, t_st, t_en, q_st, q_en, strand, contig};
    text_outs o{cig_status, reduce_out, norm_out, rows, n_rows, row_text_off, row_text, nullptr, counters};
    return host_break_lift_text(ctx, max_size, policy, c, {n_win, w_contig, w_st, w_en}, o, row_piece, declined);
}
extern "C" int rb_host_break_liftover_stats_text(rb_ctx *ctx, uint64_t n_rec, const uint8_t *text, uint64_t text_bytes, const uint64_t *cig_off,
                                                 const uint64_t *cig_end, const uint64_t *t_st, const uint64_t *t_en, const uint64_t *q_st,
                                                 const uint64_t *q_en, const uint8_t *strand, const uint32_t *contig, uint64_t n_win,
                                                 const uint32_t *w_contig, const uint64_t *w_st, const uint64_t *w_en, uint32_t max_size, int policy,
                                                 uint8_t *cig_status, rb_reduce_row *reduce_out, rb_norm_row *norm_out, rb_hit_row **rows,
                                                 uint64_t *n_rows, rb_reduce_row **stats, rb_counters *counters, uint32_t **row_piece, int *declined) {
    if (!stats) return RB_E_INVALID;
    const text_cols c{n_rec, text, text_bytes, cig_off, cig_end, t_st, t_en, q_st, q_en, strand, contig};
    text_outs o{cig_status, reduce_out, norm_out, rows, n_rows, nullptr, nullptr, stats, counters};
    return host_break_lift_text(ctx, max_size, policy, c, {n_win, w_contig, w_st, w_en}, o, row_piece, declined);
}

extern "C" int rb_host_swap(rb_ctx *ctx, uint64_t n_rec, const uint32_t *ops, const uint64_t *op_off, const uint8_t *strand,
                            uint32_t *out_ops) {
    if (!ctx) return RB_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevBatch b(ctx);
    std::vector<uint64_t> z(n_rec, 0);
    int rc = b.load(n_rec, ops, op_off, z.data(), z.data(), z.data(), z.data(), strand, nullptr);
    if (rc) return rc;
    uint32_t *d_out = nullptr;
    const uint64_t n_ops = n_rec ? op_off[n_rec] : 0;
    if ((rc = b.alloc((size_t)n_ops + 4, &d_out))) return rc;
    if ((rc = rb_dev_swap(ctx, &b.v, d_out))) return rc;
    return rb_dev_download(ctx, out_ops, d_out, (size_t)n_ops * 4);
}

extern "C" int rb_host_overlap_split(rb_ctx *ctx, uint64_t n_rec, const uint32_t *ops, const uint64_t *op_off, const uint64_t *t_st,
                                     const uint64_t *t_en, const uint64_t *q_st, const uint64_t *q_en, const uint8_t *strand,
                                     uint64_t n_pairs, const uint32_t *left, const uint32_t *right, int match_score, int diff_score,
                                     int indel_score, int policy, rb_pair_row *rows, uint32_t **out_ops, uint64_t *n_out) {
    if (!ctx || !out_ops || !n_out || (n_pairs && !rows)) return RB_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    *out_ops = nullptr;
    *n_out = 0;
    DevBatch b(ctx);
    int rc = b.load(n_rec, ops, op_off, t_st, t_en, q_st, q_en, strand, nullptr);
    if (rc) return rc;
    rb_norm_row *d_norm = nullptr;
    if ((rc = b.alloc(n_rec, &d_norm))) return rc;
    if ((rc = rb_dev_scan_records(ctx, &b.v, nullptr, d_norm))) return rc;
    std::vector<uint64_t> poff(n_pairs + 1, 0);
    for (uint64_t i = 0; i < n_pairs; i++) {
        if (left[i] >= n_rec || right[i] >= n_rec) return fail(ctx, RB_E_INVALID, "pair %llu references a record outside the batch", (unsigned long long)i);
        poff[i + 1] = poff[i] + (op_off[left[i] + 1] - op_off[left[i]]) + (op_off[right[i] + 1] - op_off[right[i]]);
    }
    const uint32_t *d_left = nullptr, *d_right = nullptr;
    const uint64_t *d_poff = nullptr;
    rb_pair_row *d_rows = nullptr;
    uint32_t *d_out = nullptr;
    if ((rc = b.up(left, (size_t)n_pairs, &d_left))) return rc;
    if ((rc = b.up(right, (size_t)n_pairs, &d_right))) return rc;
    if ((rc = b.up(poff.data(), (size_t)n_pairs + 1, &d_poff))) return rc;
    if ((rc = b.alloc((size_t)n_pairs + 1, &d_rows))) return rc;
    if ((rc = b.alloc((size_t)poff[n_pairs] + 4, &d_out))) return rc;
    if ((rc = rb_dev_overlap_split(ctx, &b.v, d_norm, n_pairs, d_left, d_right, d_poff, match_score, diff_score, indel_score, policy,
                                   d_rows, d_out)))
        return rc;
    if (n_pairs && (rc = rb_dev_download(ctx, rows, d_rows, (size_t)n_pairs * sizeof(rb_pair_row)))) return rc;
    std::vector<uint32_t> raw((size_t)poff[n_pairs] + 4);
    if (poff[n_pairs] && (rc = rb_dev_download(ctx, raw.data(), d_out, (size_t)poff[n_pairs] * 4))) return rc;
    uint64_t total = 0;
    for (uint64_t i = 0; i < n_pairs; i++)
        if (rows[i].status == RB_ST_OK) total += rows[i].out_n[0] + rows[i].out_n[1];
    *out_ops = (uint32_t *)malloc((size_t)(total + 1) * 4);
    if (!*out_ops) return fail(ctx, RB_E_NOMEM, "malloc(%llu ops)", (unsigned long long)total);
    // dense offsets first, then the copies on all host threads
    std::vector<uint64_t> src(2 * (size_t)n_pairs);
    uint64_t o = 0;
    for (uint64_t i = 0; i < n_pairs; i++) {
        for (int s = 0; s < 2; s++) {
            src[2 * i + s] = rows[i].out_off[s];
            if (rows[i].status == RB_ST_OK) {
                rows[i].out_off[s] = o;
                o += rows[i].out_n[s];
            } else {
                rows[i].out_off[s] = 0;
                rows[i].out_n[s] = 0;
            }
        }
    }
    {
        const unsigned T = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(std::thread::hardware_concurrency(), n_pairs / 1024));
        std::vector<std::thread> th;
        for (unsigned t = 0; t < T; t++)
            th.emplace_back([&, t] {
                for (uint64_t i = n_pairs * t / T; i < n_pairs * (t + 1) / T; i++)
                    for (int s = 0; s < 2; s++)
                        if (rows[i].out_n[s]) memcpy(*out_ops + rows[i].out_off[s], raw.data() + src[2 * i + s], (size_t)rows[i].out_n[s] * 4);
            });
        for (auto &x : th) x.join();
    }
    *n_out = o;
    return rb_ctx_sync(ctx);
}

// ---- synthetic workload --------------------------------------------------------------------------
#include "synth.h"
extern "C" uint32_t rb_synth_n_ops(uint64_t seed, uint64_t record, uint32_t lo, uint32_t hi) { return rb_synth_n_ops_impl(seed, record, lo, hi); }
extern "C" uint32_t rb_synth_n_ops_lognormal(uint64_t seed, uint64_t record) { return rb_synth_n_ops_lognormal_impl(seed, record); }
extern "C" void rb_synth_fill_ops_host(uint64_t seed, uint64_t first_record, uint64_t n_rec, const uint64_t *op_off, uint32_t *ops) {
    for (uint64_t r = 0; r < n_rec; r++) {
        const uint64_t n = op_off[r + 1] - op_off[r];
        for (uint64_t j = 0; j < n; j++) ops[op_off[r] + j] = rb_synth_op(seed, first_record + r, j);
    }
}
extern "C" int rb_dev_synth_fill_ops(rb_ctx *ctx, uint64_t seed, uint64_t first_record, uint64_t n_rec, const uint64_t *op_off_dev,
                                     uint32_t *ops_dev) {
    if (!ctx) return RB_E_INVALID;
    HIPCHK(ctx, rb_launch_synth(seed, first_record, n_rec, op_off_dev, ops_dev, ctx->stream));
    return RB_OK;
}

// ---- verification aid: digest of rows + clipped cigars ----------------------------------------------
extern "C" int rb_dev_digest_rows(rb_ctx *ctx, const rb_batch_view *batch, const rb_hit_row *rows, uint64_t n_rows, const uint32_t *out_ops,
                                  uint64_t row_base, uint64_t rec_base, uint64_t *digest) {
    if (!ctx || !batch || !digest || (n_rows && (!rows || !out_ops))) return RB_E_INVALID;
    rb_digest_params p;
    p.ops = batch->ops;
    p.op_off = batch->op_off;
    p.rows = rows;
    p.n_rows = n_rows;
    p.out_ops = out_ops;
    p.row_base = row_base;
    p.rec_base = rec_base;
    p.digest = (unsigned long long *)digest;
    HIPCHK(ctx, rb_launch_digest_rows(&p, ctx->stream));
    return RB_OK;
}

// ---- stats of every hit row's clip where it lies (k_hitstats.hip) ------------------------------------
extern "C" int rb_dev_stats_rows(rb_ctx *ctx, const rb_batch_view *batch, const rb_hit_row *rows, uint64_t n_rows, const uint32_t *out_ops,
                                 rb_reduce_row *stats) {
    if (!ctx || !batch || (n_rows && (!rows || !out_ops || !stats))) return RB_E_INVALID;
    rb_hitstats_params p;
    p.ops = batch->ops;
    p.op_off = batch->op_off;
    p.rows = rows;
    p.n_rows = n_rows;
    p.out_ops = out_ops;
    p.stats = stats;
    HIPCHK(ctx, rb_launch_hitstats(&p, ctx->stream));
    return RB_OK;
}

extern "C" int rb_host_stats_rows(rb_ctx *ctx, uint64_t n_rec, const uint32_t *ops, const uint64_t *op_off, const rb_hit_row *rows, uint64_t n_rows,
                                  const uint32_t *out_ops, uint64_t n_out, rb_reduce_row *stats) {
    if (!ctx || (n_rows && (!rows || !stats)) || (n_rec && (!ops || !op_off)) || (n_out && !out_ops)) return RB_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevBatch b(ctx);
    b.v.n_rec = n_rec;
    b.v.n_ops = n_rec ? op_off[n_rec] : 0;
    const rb_hit_row *d_rows = nullptr;
    const uint32_t *d_out = nullptr;
    rb_reduce_row *d_stats = nullptr;
    int rc = b.up(ops, (size_t)b.v.n_ops, &b.v.ops); // (up() leaves 256 readable bytes behind every array)
    if (!rc) rc = b.up(op_off, (size_t)n_rec + 1, &b.v.op_off);
    if (!rc) rc = b.up(rows, (size_t)n_rows, &d_rows);
    if (!rc) rc = b.up(out_ops, (size_t)n_out, &d_out);
    if (!rc) rc = b.alloc((size_t)n_rows + 1, &d_stats);
    if (!rc) rc = rb_dev_stats_rows(ctx, &b.v, d_rows, n_rows, d_out, d_stats);
    if (!rc && n_rows) rc = rb_dev_download(ctx, stats, d_stats, (size_t)n_rows * sizeof(rb_reduce_row));
    return rc ? rc : rb_ctx_sync(ctx);
}

// ---- MD strings and query spans of alignment records (k_alnstats.hip) ----------------------------------
extern "C" void rb_md_shape(uint32_t out[3]) { out[0] = rb_md_row_step(), out[1] = rb_md_row_max(), out[2] = rb_md_wave_step(); }
extern "C" int rb_dev_parse_md(rb_ctx *ctx, const uint8_t *text, const uint64_t *md_off, const uint64_t *md_end, uint64_t n, uint32_t *out,
                               uint8_t *status) {
    if (!ctx || (n && (!text || !md_off || !md_end || !out || !status))) return RB_E_INVALID;
    if ((((uintptr_t)text | (uintptr_t)out) & 15u) != 0) return fail(ctx, RB_E_INVALID, "text and out must be 16-byte aligned");
    rb_md_params p;
    p.n = n;
    p.text = text;
    p.md_off = md_off;
    p.md_end = md_end;
    p.out = out;
    p.status = status;
    HIPCHK(ctx, rb_launch_parse_md(&p, ctx->stream));
    return RB_OK;
}
extern "C" int rb_dev_aln_stats(rb_ctx *ctx, const rb_batch_view *batch, const rb_reduce_row *reduce_rows, const int64_t *pos,
                                const uint32_t *flag, const uint32_t *l_seq, const uint32_t *md, const uint8_t *md_status, const uint8_t *has_md,
                                rb_aln_row *rows) {
    if (!ctx || !batch) return RB_E_INVALID;
    const uint64_t n = batch->n_rec;
    if (n && (!batch->op_off || !reduce_rows || !pos || !flag || !l_seq || !rows || (has_md && !md))) return RB_E_INVALID;
    if (n && batch->n_ops && !batch->ops) return RB_E_INVALID;
    rb_alnstats_params p;
    p.n = n;
    p.ops = batch->ops;
    p.op_off = batch->op_off;
    p.reduce_rows = reduce_rows;
    p.pos = pos;
    p.flag = flag;
    p.l_seq = l_seq;
    p.md = md;
    p.md_status = md_status;
    p.has_md = has_md;
    p.rows = rows;
    HIPCHK(ctx, rb_launch_aln_stats(&p, ctx->stream));
    return RB_OK;
}
extern "C" int rb_host_parse_md(rb_ctx *ctx, const uint8_t *text, uint64_t text_bytes, const uint64_t *md_off, const uint64_t *md_end, uint64_t n,
                                uint32_t *out, uint8_t *status) {
    if (!ctx || (n && (!md_off || !md_end || !out || !status)) || (text_bytes && !text)) return RB_E_INVALID;
    for (uint64_t r = 0; r < n; r++)
        if (md_end[r] > md_off[r] && md_end[r] > text_bytes) return fail(ctx, RB_E_INVALID, "string %llu: MD range outside the text", (unsigned long long)r);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevBatch b(ctx);
    uint8_t *d_text = nullptr, *d_status = nullptr;
    const uint64_t *d_off = nullptr, *d_end = nullptr;
    uint32_t *d_out = nullptr;
    int rc = b.alloc((size_t)text_bytes + 32, &d_text); // (the slack the device call asks for)
    if (!rc && text_bytes) rc = rb_dev_upload(ctx, d_text, text, (size_t)text_bytes);
    if (!rc) rc = b.up(md_off, (size_t)n, &d_off);
    if (!rc) rc = b.up(md_end, (size_t)n, &d_end);
    if (!rc) rc = b.alloc(4 * (size_t)n + 4, &d_out);
    if (!rc) rc = b.alloc((size_t)n + 1, &d_status);
    if (!rc) rc = rb_dev_parse_md(ctx, d_text, d_off, d_end, n, d_out, d_status);
    if (!rc && n) rc = rb_dev_download(ctx, out, d_out, 16 * (size_t)n);
    if (!rc && n) rc = rb_dev_download(ctx, status, d_status, (size_t)n);
    return rc ? rc : rb_ctx_sync(ctx);
}
extern "C" int rb_host_aln_stats(rb_ctx *ctx, uint64_t n, const uint32_t *ops, const uint64_t *op_off, const rb_reduce_row *reduce_rows,
                                 const int64_t *pos, const uint32_t *flag, const uint32_t *l_seq, const uint32_t *md, const uint8_t *md_status,
                                 const uint8_t *has_md, rb_aln_row *rows) {
    if (!ctx || (n && (!op_off || !reduce_rows || !pos || !flag || !l_seq || !rows || (has_md && !md)))) return RB_E_INVALID;
    if (n && op_off[n] && !ops) return RB_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevBatch b(ctx);
    b.v.n_rec = n;
    b.v.n_ops = n ? op_off[n] : 0;
    const rb_reduce_row *d_red = nullptr;
    const int64_t *d_pos = nullptr;
    const uint32_t *d_flag = nullptr, *d_lseq = nullptr, *d_md = nullptr;
    const uint8_t *d_mst = nullptr, *d_has = nullptr;
    rb_aln_row *d_rows = nullptr;
    int rc = b.up(ops, (size_t)b.v.n_ops, &b.v.ops);
    if (!rc) rc = b.up(op_off, (size_t)n + 1, &b.v.op_off);
    if (!rc) rc = b.up(reduce_rows, (size_t)n, &d_red);
    if (!rc) rc = b.up(pos, (size_t)n, &d_pos);
    if (!rc) rc = b.up(flag, (size_t)n, &d_flag);
    if (!rc) rc = b.up(l_seq, (size_t)n, &d_lseq);
    if (!rc && has_md) rc = b.up(md, 4 * (size_t)n, &d_md);
    if (!rc && has_md && md_status) rc = b.up(md_status, (size_t)n, &d_mst);
    if (!rc && has_md) rc = b.up(has_md, (size_t)n, &d_has);
    if (!rc) rc = b.alloc((size_t)n + 1, &d_rows);
    if (!rc) rc = rb_dev_aln_stats(ctx, &b.v, d_red, d_pos, d_flag, d_lseq, d_md, d_mst, d_has, d_rows);
    if (!rc && n) rc = rb_dev_download(ctx, rows, d_rows, (size_t)n * sizeof(rb_aln_row));
    return rc ? rc : rb_ctx_sync(ctx);
}

// ---- the records of an inflated BAM stream (k_bam.hip) -------------------------------------------------
// scratch of rb_dev_bam_records: [where each record's words lie (n) u64][block sums of the scan]
static size_t bam_src_bytes(uint64_t n) { return ((size_t)(n + 1) * 8 + 255) & ~(size_t)255; }
extern "C" size_t rb_bam_scratch_bytes(uint64_t n) { return bam_src_bytes(n) + (rb_scan_block_sums_count(n) + 4) * 8; }
extern "C" void rb_bam_shape(uint32_t out[6]) {
    out[0] = rb_bam_aux_row_step(), out[1] = rb_bam_aux_row_max(), out[2] = rb_bam_aux_wave_step();
    out[3] = rb_bam_copy_row_step(), out[4] = rb_bam_copy_row_max(), out[5] = rb_bam_copy_wave_step();
}
extern "C" int rb_dev_bam_records(rb_ctx *ctx, const uint8_t *data, const uint64_t *rec_off, const uint32_t *rec_len, uint64_t n, int32_t *tid,
                                  int64_t *pos, uint32_t *flag, uint32_t *l_seq, uint8_t *has_md, uint64_t *md_off, uint64_t *md_end, uint64_t *op_off,
                                  uint32_t *ops, uint64_t ops_cap, uint8_t *status, void *scratch) {
    if (!ctx || !op_off) return RB_E_INVALID;
    if (n && (!data || !rec_off || !rec_len || !tid || !pos || !flag || !l_seq || !has_md || !md_off || !md_end || !status || !scratch)) return RB_E_INVALID;
    if (ops_cap && !ops) return RB_E_INVALID;
    if ((((uintptr_t)data | (uintptr_t)ops) & 15u) != 0) return fail(ctx, RB_E_INVALID, "rb_dev_bam_records: data and ops must be 16-byte aligned");
    if (((uintptr_t)scratch & 7u) != 0) return fail(ctx, RB_E_INVALID, "rb_dev_bam_records: scratch must be 8-byte aligned");
    rb_bam_params p;
    p.n = n;
    p.data = data, p.rec_off = rec_off, p.rec_len = rec_len;
    p.tid = tid, p.pos = pos, p.flag = flag, p.l_seq = l_seq, p.has_md = has_md, p.md_off = md_off, p.md_end = md_end;
    p.op_off = op_off, p.ops = ops, p.ops_cap = ops_cap, p.status = status;
    p.src = (uint64_t *)scratch;
    HIPCHK(ctx, rb_fill_async(op_off + n, 0, 8, ctx->stream));
    if (n == 0) return RB_OK;
    HIPCHK(ctx, rb_launch_bam_peek(&p, ctx->stream));
    HIPCHK(ctx, rb_launch_exclusive_scan(op_off, n, (uint64_t *)((uint8_t *)scratch + bam_src_bytes(n)), nullptr, ctx->stream));
    HIPCHK(ctx, rb_launch_bam_copy(&p, ctx->stream));
    return RB_OK;
}
// ---- the per-read index of nucfreq on the columns of rb_dev_bam_records (k_bamreads.hip) ------------------
// scratch of rb_dev_bam_reads: the maxima of the scan's workgroups, level by level
extern "C" size_t rb_bam_reads_scratch_bytes(uint64_t n) { return (rb_bam_reads_blk_count(n) * 8 + 255) & ~(size_t)255; }
extern "C" void rb_bam_reads_shape(uint32_t out[4]) {
    out[0] = rb_bam_reads_row_step(), out[1] = rb_bam_reads_row_max(), out[2] = rb_bam_reads_wave_step(), out[3] = rb_bam_reads_scan_block();
}
extern "C" int rb_dev_bam_reads(rb_ctx *ctx, const uint8_t *data, const uint64_t *rec_off, const uint32_t *rec_len, uint64_t n, const int32_t *tid,
                                const int64_t *pos, const uint32_t *flag, const uint64_t *op_off, const uint32_t *ops, const uint8_t *status,
                                uint64_t *seq_off, uint64_t *start_key, uint64_t *end_key_pmax, uint64_t *first_unsorted, void *scratch) {
    if (!ctx || !first_unsorted) return RB_E_INVALID;
    if (n && (!data || !rec_off || !rec_len || !tid || !pos || !flag || !op_off || !status || !seq_off || !start_key || !end_key_pmax || !scratch))
        return RB_E_INVALID;
    if (((uintptr_t)data | (uintptr_t)ops) & 15u) return fail(ctx, RB_E_INVALID, "rb_dev_bam_reads: data and ops must be 16-byte aligned");
    if ((uintptr_t)scratch & 255u) return fail(ctx, RB_E_INVALID, "rb_dev_bam_reads: scratch must be 256-byte aligned");
    rb_bam_reads_params p;
    p.n = n;
    p.data = data, p.rec_off = rec_off, p.rec_len = rec_len;
    p.tid = tid, p.pos = pos, p.flag = flag, p.op_off = op_off, p.ops = ops, p.status = status;
    p.seq_off = seq_off, p.start_key = start_key, p.end_key_pmax = end_key_pmax;
    p.first_unsorted = (unsigned long long *)first_unsorted;
    p.blk = (uint64_t *)scratch;
    HIPCHK(ctx, rb_fill_async(first_unsorted, 0xFF, 8, ctx->stream));
    HIPCHK(ctx, rb_launch_bam_reads(&p, ctx->stream));
    return RB_OK;
}
// rb_host_bam_records, and with `reads` rb_host_bam_reads: the two share upload, columns and downloads
static int bam_host(rb_ctx *ctx, bool reads, const uint8_t *data, uint64_t data_bytes, const uint64_t *rec_off, const uint32_t *rec_len, uint64_t n, int32_t *tid,
                    int64_t *pos, uint32_t *flag, uint32_t *l_seq, uint8_t *has_md, uint64_t *md_off, uint64_t *md_end, uint64_t *op_off, uint32_t *ops,
                    uint64_t ops_cap, uint8_t *status, uint64_t *seq_off, uint64_t *start_key, uint64_t *end_key_pmax, uint64_t *first_unsorted) {
    if (!ctx || !op_off || (data_bytes && !data) || (ops_cap && !ops) || (reads && !first_unsorted)) return RB_E_INVALID;
    if (n && (!rec_off || !rec_len || !tid || !pos || !flag || !l_seq || !has_md || !md_off || !md_end || !status)) return RB_E_INVALID;
    if (n && reads && (!seq_off || !start_key || !end_key_pmax)) return RB_E_INVALID;
    for (uint64_t r = 0; r < n; r++)
        if (rec_off[r] > data_bytes || rec_len[r] > data_bytes - rec_off[r]) return fail(ctx, RB_E_INVALID, "record %llu: outside the data", (unsigned long long)r);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevBatch b(ctx);
    uint8_t *d_data = nullptr, *d_has = nullptr, *d_status = nullptr, *d_scr = nullptr, *d_scr2 = nullptr;
    const uint64_t *d_roff = nullptr;
    const uint32_t *d_rlen = nullptr;
    int32_t *d_tid = nullptr;
    int64_t *d_pos = nullptr;
    uint32_t *d_flag = nullptr, *d_lseq = nullptr, *d_ops = nullptr;
    uint64_t *d_moff = nullptr, *d_mend = nullptr, *d_opoff = nullptr, *d_sqo = nullptr, *d_sk = nullptr, *d_ek = nullptr, *d_fu = nullptr;
    int rc = b.alloc((size_t)data_bytes + 32, &d_data); // (the slack the device calls ask for)
    if (!rc && data_bytes) rc = rb_dev_upload(ctx, d_data, data, (size_t)data_bytes);
    if (!rc) rc = b.up(rec_off, (size_t)n, &d_roff);
    if (!rc) rc = b.up(rec_len, (size_t)n, &d_rlen);
    if (!rc) rc = b.alloc((size_t)n + 1, &d_tid);
    if (!rc) rc = b.alloc((size_t)n + 1, &d_pos);
    if (!rc) rc = b.alloc((size_t)n + 1, &d_flag);
    if (!rc) rc = b.alloc((size_t)n + 1, &d_lseq);
    if (!rc) rc = b.alloc((size_t)n + 1, &d_has);
    if (!rc) rc = b.alloc((size_t)n + 1, &d_moff);
    if (!rc) rc = b.alloc((size_t)n + 1, &d_mend);
    if (!rc) rc = b.alloc((size_t)n + 2, &d_opoff);
    if (!rc) rc = b.alloc((size_t)ops_cap + 4, &d_ops);
    if (!rc) rc = b.alloc((size_t)n + 1, &d_status);
    if (!rc) rc = b.alloc(rb_bam_scratch_bytes(n), &d_scr);
    if (!rc) rc = rb_dev_bam_records(ctx, d_data, d_roff, d_rlen, n, d_tid, d_pos, d_flag, d_lseq, d_has, d_moff, d_mend, d_opoff, d_ops, ops_cap, d_status, d_scr);
    if (!rc) rc = rb_dev_download(ctx, op_off, d_opoff, ((size_t)n + 1) * 8); // (rb_dev_download returns with the bytes there: op_off[n] is read below)
    if (!rc && reads) {
        if (op_off[n] > ops_cap) return fail(ctx, RB_E_INVALID, "rb_host_bam_reads: %llu ops do not fit ops_cap", (unsigned long long)op_off[n]);
        rc = b.alloc((size_t)n + 1, &d_sqo);
        if (!rc) rc = b.alloc((size_t)n + 1, &d_sk);
        if (!rc) rc = b.alloc((size_t)n + 1, &d_ek);
        if (!rc) rc = b.alloc(1, &d_fu);
        if (!rc) rc = b.alloc(rb_bam_reads_scratch_bytes(n) + 256, &d_scr2);
        d_scr2 = (uint8_t *)(((uintptr_t)d_scr2 + 255) & ~(uintptr_t)255);
        if (!rc) rc = rb_dev_bam_reads(ctx, d_data, d_roff, d_rlen, n, d_tid, d_pos, d_flag, d_opoff, d_ops, d_status, d_sqo, d_sk, d_ek, d_fu, d_scr2);
        if (!rc && n) rc = rb_dev_download(ctx, seq_off, d_sqo, (size_t)n * 8);
        if (!rc && n) rc = rb_dev_download(ctx, start_key, d_sk, (size_t)n * 8);
        if (!rc && n) rc = rb_dev_download(ctx, end_key_pmax, d_ek, (size_t)n * 8);
        if (!rc) rc = rb_dev_download(ctx, first_unsorted, d_fu, 8);
    }
    if (!rc && n) rc = rb_dev_download(ctx, tid, d_tid, (size_t)n * 4);
    if (!rc && n) rc = rb_dev_download(ctx, pos, d_pos, (size_t)n * 8);
    if (!rc && n) rc = rb_dev_download(ctx, flag, d_flag, (size_t)n * 4);
    if (!rc && n) rc = rb_dev_download(ctx, l_seq, d_lseq, (size_t)n * 4);
    if (!rc && n) rc = rb_dev_download(ctx, has_md, d_has, (size_t)n);
    if (!rc && n) rc = rb_dev_download(ctx, md_off, d_moff, (size_t)n * 8);
    if (!rc && n) rc = rb_dev_download(ctx, md_end, d_mend, (size_t)n * 8);
    if (!rc && n) rc = rb_dev_download(ctx, status, d_status, (size_t)n);
    if (!rc) {
        const uint64_t got = op_off[n] < ops_cap ? op_off[n] : ops_cap;
        if (got) rc = rb_dev_download(ctx, ops, d_ops, (size_t)got * 4);
    }
    return rc ? rc : rb_ctx_sync(ctx);
}
extern "C" int rb_host_bam_records(rb_ctx *ctx, const uint8_t *data, uint64_t data_bytes, const uint64_t *rec_off, const uint32_t *rec_len, uint64_t n,
                                   int32_t *tid, int64_t *pos, uint32_t *flag, uint32_t *l_seq, uint8_t *has_md, uint64_t *md_off, uint64_t *md_end,
                                   uint64_t *op_off, uint32_t *ops, uint64_t ops_cap, uint8_t *status) {
    return bam_host(ctx, false, data, data_bytes, rec_off, rec_len, n, tid, pos, flag, l_seq, has_md, md_off, md_end, op_off, ops, ops_cap, status, nullptr,
                    nullptr, nullptr, nullptr);
}
extern "C" int rb_host_bam_reads(rb_ctx *ctx, const uint8_t *data, uint64_t data_bytes, const uint64_t *rec_off, const uint32_t *rec_len, uint64_t n,
                                 int32_t *tid, int64_t *pos, uint32_t *flag, uint32_t *l_seq, uint8_t *has_md, uint64_t *md_off, uint64_t *md_end,
                                 uint64_t *op_off, uint32_t *ops, uint64_t ops_cap, uint8_t *status, uint64_t *seq_off, uint64_t *start_key,
                                 uint64_t *end_key_pmax, uint64_t *first_unsorted) {
    return bam_host(ctx, true, data, data_bytes, rec_off, rec_len, n, tid, pos, flag, l_seq, has_md, md_off, md_end, op_off, ops, ops_cap, status, seq_off,
                    start_key, end_key_pmax, first_unsorted);
}

// ---- the hit rows of a clip call as a dense batch (k_rows_batch.hip) ----------------------------------
// scratch of rb_dev_rows_to_batch: [ops per row (n_rows + 1) u64][1 per OK row (n_rows + 1) u64][block sums of the scans]
static size_t rtb_cnt_bytes(uint64_t n_rows) { return ((size_t)(n_rows + 1) * 8 + 255) & ~(size_t)255; }
extern "C" size_t rb_rows_to_batch_scratch_bytes(uint64_t n_rows) { return 2 * rtb_cnt_bytes(n_rows) + (rb_scan_block_sums_count(n_rows) + 4) * 8; }
extern "C" void rb_rows_to_batch_shape(uint32_t out[3]) { out[0] = rb_rtb_row_step(), out[1] = rb_rtb_row_max(), out[2] = rb_rtb_wave_step(); }
extern "C" int rb_dev_rows_to_batch(rb_ctx *ctx, const rb_batch_view *src, const rb_hit_row *rows, uint64_t n_rows, const uint32_t *out_ops,
                                    uint64_t pieces_cap, uint64_t ops_cap, uint32_t *new_ops, uint64_t *new_op_off, uint64_t *t_st, uint64_t *t_en,
                                    uint64_t *q_st, uint64_t *q_en, uint8_t *strand, uint32_t *contig, uint32_t *parent, rb_pieces_info *info,
                                    void *scratch) {
    if (!ctx || !src || !info || (n_rows && (!rows || !out_ops || !scratch))) return RB_E_INVALID;
    if (new_ops && (!new_op_off || !t_st || !t_en || !q_st || !q_en || !strand || !contig || !parent)) return RB_E_INVALID;
    if ((((uintptr_t)rows | (uintptr_t)out_ops | (uintptr_t)src->ops | (uintptr_t)new_ops) & 15u) != 0)
        return fail(ctx, RB_E_INVALID, "rb_dev_rows_to_batch: rows, out_ops, the batch's ops and new_ops must be 16-byte aligned");
    rb_rows_batch_params p;
    memset(&p, 0, sizeof p);
    p.ops = src->ops, p.op_off = src->op_off, p.src_strand = src->strand, p.src_contig = src->contig;
    p.rows = rows, p.n_rows = n_rows, p.out_ops = out_ops;
    p.pieces_cap = pieces_cap, p.ops_cap = ops_cap;
    p.cnt_ops = (uint64_t *)scratch;
    p.cnt_pieces = (uint64_t *)((char *)scratch + rtb_cnt_bytes(n_rows));
    uint64_t *blk = (uint64_t *)((char *)scratch + 2 * rtb_cnt_bytes(n_rows));
    p.new_ops = new_ops, p.new_op_off = new_op_off;
    p.t_st = t_st, p.t_en = t_en, p.q_st = q_st, p.q_en = q_en, p.strand = strand, p.contig = contig, p.parent = parent;
    p.info = info;
    HIPCHK(ctx, rb_fill_async(info, 0, sizeof *info, ctx->stream));
    if (n_rows == 0) {
        if (new_ops) HIPCHK(ctx, rb_fill_async(new_op_off, 0, 8, ctx->stream));
        return RB_OK;
    }
    HIPCHK(ctx, rb_launch_rows_batch_count(&p, ctx->stream));
    HIPCHK(ctx, rb_launch_exclusive_scan(p.cnt_ops, n_rows, blk, &info->n_ops, ctx->stream));
    HIPCHK(ctx, rb_launch_exclusive_scan(p.cnt_pieces, n_rows, blk, &info->n_pieces, ctx->stream));
    if (new_ops) HIPCHK(ctx, rb_launch_rows_batch_fill(&p, ctx->stream)); // (NULL: sizes only -- info says what the dense batch holds)
    return RB_OK;
}

// ---- orient / filter over hit rows (k_pairs.hip) -------------------------------------------------------
// scratch of rb_dev_pairs_rows: [orient n_keys i64][tspan n_keys u64][fspan n_keys u64][1 per kept row (n_rows + 1) u64][block sums of the scan]
static size_t pairs_sum_bytes(uint64_t n_keys) { return ((size_t)n_keys * 8 + 255) & ~(size_t)255; }
static size_t pairs_cnt_bytes(uint64_t n_rows) { return ((size_t)(n_rows + 1) * 8 + 255) & ~(size_t)255; }
extern "C" size_t rb_pairs_scratch_bytes(uint64_t n_keys, uint64_t n_rows) {
    return 3 * pairs_sum_bytes(n_keys) + pairs_cnt_bytes(n_rows) + (rb_scan_block_sums_count(n_rows) + 4) * 8;
}
extern "C" void rb_pairs_shape(uint32_t out[2]) { out[0] = rb_pairs_wave_rows(), out[1] = rb_pairs_block_rows(); }
extern "C" int rb_dev_pairs_rows(rb_ctx *ctx, const rb_hit_row *rows, uint64_t n_rows, const uint32_t *rec_key, const uint64_t *rec_q_len,
                                 const uint8_t *strand, uint64_t n_rec, uint64_t n_keys, uint32_t mode, uint64_t paired_len, uint64_t min_aln,
                                 uint64_t min_query, rb_hit_row *rows_out, uint64_t rows_cap, uint8_t *key_flip, rb_pairs_info *info, void *scratch) {
    if (!ctx || !info || (n_rows && (!rows || !scratch)) || (n_rec && (!rec_key || !rec_q_len || !strand)) || (n_keys && (!key_flip || !scratch)) ||
        (rows_cap && !rows_out) || (mode & ~(uint32_t)(RB_PAIRS_ORIENT | RB_PAIRS_FILTER)))
        return RB_E_INVALID;
    if ((((uintptr_t)rows | (uintptr_t)rows_out) & 15u) != 0) return fail(ctx, RB_E_INVALID, "rb_dev_pairs_rows: rows and rows_out must be 16-byte aligned");
    if (n_rows >> 32) return fail(ctx, RB_E_INVALID, "rb_dev_pairs_rows: %llu rows (the call counts kept and flipped rows in the halves of one u64: below 2^32)", (unsigned long long)n_rows);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    rb_pairs_params p;
    memset(&p, 0, sizeof p);
    char *sc = (char *)scratch;
    p.rows = rows, p.n_rows = n_rows, p.rec_key = rec_key, p.rec_q_len = rec_q_len, p.strand = strand, p.n_rec = n_rec, p.n_keys = n_keys;
    p.mode = mode, p.paired_len = paired_len, p.min_aln = min_aln, p.min_query = min_query;
    p.orient = (unsigned long long *)sc;
    p.tspan = (unsigned long long *)(sc + pairs_sum_bytes(n_keys));
    p.fspan = (unsigned long long *)(sc + 2 * pairs_sum_bytes(n_keys));
    p.cnt = (uint64_t *)(sc + 3 * pairs_sum_bytes(n_keys));
    p.rows_out = rows_out, p.rows_cap = rows_cap, p.key_flip = key_flip, p.info = info;
    HIPCHK(ctx, rb_fill_async(info, 0, sizeof *info, ctx->stream));
    if (n_keys) HIPCHK(ctx, rb_fill_async(sc, 0, 3 * pairs_sum_bytes(n_keys), ctx->stream)); // (every call: nothing of the last one counts)
    HIPCHK(ctx, rb_launch_pairs(&p, (uint64_t *)(sc + 3 * pairs_sum_bytes(n_keys) + pairs_cnt_bytes(n_rows)), ctx->stream));
    return RB_OK;
}
// the same rules on host arrays, in the reference's order of steps (no device: the record route's self-check, the tests' second opinion)
extern "C" int rb_host_pairs_rows(const rb_hit_row *rows, uint64_t n_rows, const uint32_t *rec_key, const uint64_t *rec_q_len, const uint8_t *strand,
                                  uint64_t n_rec, uint64_t n_keys, uint32_t mode, uint64_t paired_len, uint64_t min_aln, uint64_t min_query,
                                  rb_hit_row *rows_out, uint64_t rows_cap, uint8_t *key_flip, rb_pairs_info *info) {
    if (!info || (n_rows && !rows) || (n_rec && (!rec_key || !rec_q_len || !strand)) || (n_keys && !key_flip) || (rows_cap && !rows_out) ||
        (mode & ~(uint32_t)(RB_PAIRS_ORIENT | RB_PAIRS_FILTER)))
        return RB_E_INVALID;
    memset(info, 0, sizeof *info);
    std::vector<int64_t> orient((size_t)n_keys, 0);
    std::vector<uint64_t> tspan((size_t)n_keys, 0), fspan((size_t)n_keys, 0);
    std::vector<uint8_t> has((size_t)n_keys, 0), part((size_t)n_rows, 0);
    const bool do_orient = (mode & RB_PAIRS_ORIENT) != 0, do_filter = (mode & RB_PAIRS_FILTER) != 0;
    auto passes = [&](const rb_hit_row &h) { return !do_filter || (rec_q_len[h.rec] > min_query && h.t_en - h.t_st > min_aln); };
    for (uint64_t k = 0; k < n_rows; k++) {
        const rb_hit_row &h = rows[k];
        if (h.status >= RB_ST_PANIC_NOTFOUND) info->declined |= RB_PAIRS_DECL_PANIC;
        if (h.status != RB_ST_OK) continue;
        if (h.rec >= n_rec || rec_key[h.rec] >= n_keys) {
            info->declined |= RB_PAIRS_DECL_KEY;
            continue;
        }
        part[k] = 1;
        const uint32_t key = rec_key[h.rec];
        has[key] = 1;
        const uint64_t q = h.q_en - h.q_st;
        if (do_orient) orient[key] = (int64_t)((uint64_t)orient[key] + (strand[h.rec] == (uint8_t)'-' ? 0 - q : q)); // paf.rs:124-128
        tspan[key] += h.t_en - h.t_st;
        if (do_filter && passes(h)) fspan[key] += h.t_en - h.t_st; // paf.rs:97, behind main.rs:242-243
    }
    for (uint64_t i = 0; i < n_keys; i++) {
        key_flip[i] = orient[i] < 0 ? 1 : 0; // paf.rs:146
        if (do_orient && has[i] && tspan[i] == 0) info->declined |= RB_PAIRS_DECL_ZERO_SPAN; // paf.rs:143
    }
    for (uint64_t k = 0; k < n_rows; k++) {
        if (!part[k]) continue;
        rb_hit_row h = rows[k];
        const uint32_t key = rec_key[h.rec];
        const uint64_t q_len = rec_q_len[h.rec];
        if (key_flip[key]) {
            if (q_len < h.q_en) info->declined |= RB_PAIRS_DECL_WRAP;
            const uint64_t st = q_len - h.q_en, en = q_len - h.q_st; // paf.rs:148-151
            h.q_st = st, h.q_en = en;
        }
        if (!(passes(rows[k]) && (!do_filter || paired_len < fspan[key]))) continue; // paf.rs:100
        if (info->n_kept < rows_cap) rows_out[info->n_kept] = h;
        else info->overflow = 1;
        info->n_kept++;
        if (key_flip[key]) info->n_flipped_rows++;
    }
    return RB_OK;
}

// ---- orient / filter over the records of a batch (k_pairs.hip) ------------------------------------------
// scratch of rb_dev_pairs_records: [orient][tspan][fspan][order] n_keys u64 each, [1 per kept record (n_rec + 1) u64][block sums of the scan]
extern "C" size_t rb_pairs_records_scratch_bytes(uint64_t n_keys, uint64_t n_rec) {
    return 4 * pairs_sum_bytes(n_keys) + pairs_cnt_bytes(n_rec) + (rb_scan_block_sums_count(n_rec) + 4) * 8;
}
extern "C" void rb_pairs_records_shape(uint32_t out[2]) { out[0] = rb_pairs_wave_rows(), out[1] = rb_pairs_block_rows(); }
// what both forms refuse; *why: what rb_ctx_last_error says (NULL: a null pointer)
static bool pairs_records_args_ok(const uint64_t *t_st, const uint64_t *t_en, const uint64_t *q_st, const uint64_t *q_en, const uint8_t *strand,
                                  const uint32_t *rec_key, const uint64_t *rec_q_len, uint64_t n_rec, uint64_t n_keys, uint32_t mode, const uint32_t *kept,
                                  uint64_t kept_cap, const uint64_t *q_st_out, const uint64_t *q_en_out, const uint8_t *key_flip, const uint64_t *key_order,
                                  const rb_pairs_info *info, const char **why) {
    *why = nullptr;
    if (!info || (n_rec && (!t_st || !t_en || !q_st || !q_en || !strand || !rec_key || !rec_q_len)) || (n_keys && !key_flip) || (kept_cap && !kept) ||
        (!q_st_out != !q_en_out))
        return false;
    if (mode & ~(uint32_t)(RB_PAIRS_ORIENT | RB_PAIRS_FILTER)) return *why = "an unknown mode bit (RB_PAIRS_ORIENT | RB_PAIRS_FILTER)", false;
    if (n_rec >> 32) return *why = "2^32 records and more (kept and flipped records are counted in the halves of one u64)", false;
    const uintptr_t a8 = (uintptr_t)t_st | (uintptr_t)t_en | (uintptr_t)q_st | (uintptr_t)q_en | (uintptr_t)rec_q_len | (uintptr_t)q_st_out |
                         (uintptr_t)q_en_out | (uintptr_t)key_order | (uintptr_t)info;
    if ((a8 & 7u) || (((uintptr_t)rec_key | (uintptr_t)kept) & 3u)) return *why = "a misaligned pointer (u64 columns and info: 8 bytes, u32 columns: 4)", false;
    return true;
}
extern "C" int rb_dev_pairs_records(rb_ctx *ctx, const uint64_t *t_st, const uint64_t *t_en, const uint64_t *q_st, const uint64_t *q_en,
                                    const uint8_t *strand, const uint32_t *rec_key, const uint64_t *rec_q_len, uint64_t n_rec, uint64_t n_keys,
                                    uint32_t mode, uint64_t paired_len, uint64_t min_aln, uint64_t min_query, uint32_t *kept, uint64_t kept_cap,
                                    uint64_t *q_st_out, uint64_t *q_en_out, uint8_t *key_flip, uint64_t *key_order, rb_pairs_info *info, void *scratch) {
    const char *why;
    if (!ctx) return RB_E_INVALID;
    if (!pairs_records_args_ok(t_st, t_en, q_st, q_en, strand, rec_key, rec_q_len, n_rec, n_keys, mode, kept, kept_cap, q_st_out, q_en_out, key_flip, key_order,
                               info, &why))
        return why ? fail(ctx, RB_E_INVALID, "rb_dev_pairs_records: %s", why) : RB_E_INVALID;
    if ((n_rec || n_keys) && !scratch) return RB_E_INVALID;
    if ((uintptr_t)scratch & 255u) return fail(ctx, RB_E_INVALID, "rb_dev_pairs_records: the scratch must be 256-byte aligned");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    rb_pairs_rec_params p;
    memset(&p, 0, sizeof p);
    char *sc = (char *)scratch;
    const size_t sb = pairs_sum_bytes(n_keys);
    p.t_st = t_st, p.t_en = t_en, p.q_st = q_st, p.q_en = q_en, p.strand = strand, p.rec_key = rec_key, p.rec_q_len = rec_q_len;
    p.n_rec = n_rec, p.n_keys = n_keys, p.mode = mode, p.paired_len = paired_len, p.min_aln = min_aln, p.min_query = min_query;
    p.orient = (unsigned long long *)sc, p.tspan = (unsigned long long *)(sc + sb), p.fspan = (unsigned long long *)(sc + 2 * sb);
    p.order = (unsigned long long *)(sc + 3 * sb);
    p.cnt = (uint64_t *)(sc + 4 * sb);
    p.kept = kept, p.kept_cap = kept_cap, p.q_st_out = q_st_out, p.q_en_out = q_en_out, p.key_flip = key_flip, p.key_order = key_order, p.info = info;
    HIPCHK(ctx, rb_fill_async(info, 0, sizeof *info, ctx->stream));
    if (n_keys) HIPCHK(ctx, rb_fill_async(sc, 0, 4 * sb, ctx->stream)); // (every call: nothing of the last one counts)
    HIPCHK(ctx, rb_launch_pairs_records(&p, (uint64_t *)(sc + 4 * sb + pairs_cnt_bytes(n_rec)), ctx->stream));
    return RB_OK;
}
// the same rules on host arrays, in the reference's order of steps (no device: the tests' second opinion)
extern "C" int rb_host_pairs_records(const uint64_t *t_st, const uint64_t *t_en, const uint64_t *q_st, const uint64_t *q_en, const uint8_t *strand,
                                     const uint32_t *rec_key, const uint64_t *rec_q_len, uint64_t n_rec, uint64_t n_keys, uint32_t mode,
                                     uint64_t paired_len, uint64_t min_aln, uint64_t min_query, uint32_t *kept, uint64_t kept_cap, uint64_t *q_st_out,
                                     uint64_t *q_en_out, uint8_t *key_flip, uint64_t *key_order, rb_pairs_info *info) {
    const char *why;
    if (!pairs_records_args_ok(t_st, t_en, q_st, q_en, strand, rec_key, rec_q_len, n_rec, n_keys, mode, kept, kept_cap, q_st_out, q_en_out, key_flip, key_order,
                               info, &why))
        return RB_E_INVALID;
    memset(info, 0, sizeof *info);
    std::vector<int64_t> orient((size_t)n_keys, 0);
    std::vector<uint64_t> tspan((size_t)n_keys, 0), fspan((size_t)n_keys, 0), order((size_t)n_keys, 0);
    std::vector<uint8_t> has((size_t)n_keys, 0);
    const bool do_orient = (mode & RB_PAIRS_ORIENT) != 0, do_filter = (mode & RB_PAIRS_FILTER) != 0;
    auto passes = [&](uint64_t r) { return !do_filter || (rec_q_len[r] > min_query && t_en[r] - t_st[r] > min_aln); }; // main.rs:242-243
    for (uint64_t r = 0; r < n_rec; r++) {
        const uint32_t key = rec_key[r];
        if (key >= n_keys) {
            info->declined |= RB_PAIRS_DECL_KEY;
            continue;
        }
        has[key] = 1;
        const uint64_t q = q_en[r] - q_st[r], w = t_en[r] - t_st[r];
        if (do_orient) {
            orient[key] = (int64_t)((uint64_t)orient[key] + (strand[r] == (uint8_t)'-' ? 0 - q : q)); // paf.rs:124-128
            order[key] += (w * (t_st[r] + t_en[r])) / 2;                                              // paf.rs:133
        }
        tspan[key] += w;
        if (do_filter && passes(r)) fspan[key] += w; // paf.rs:97, behind main.rs:242-243
    }
    for (uint64_t i = 0; i < n_keys; i++) {
        key_flip[i] = orient[i] < 0 ? 1 : 0; // paf.rs:146
        if (key_order) key_order[i] = do_orient && tspan[i] ? order[i] / tspan[i] : 0; // paf.rs:143
        if (do_orient && has[i] && tspan[i] == 0) info->declined |= RB_PAIRS_DECL_ZERO_SPAN;
    }
    for (uint64_t r = 0; r < n_rec; r++) {
        const uint32_t key = rec_key[r];
        const bool part = key < n_keys, flip = part && key_flip[key];
        if (flip && rec_q_len[r] < q_en[r]) info->declined |= RB_PAIRS_DECL_WRAP;
        if (q_st_out) {
            q_st_out[r] = flip ? rec_q_len[r] - q_en[r] : q_st[r]; // paf.rs:148-151
            q_en_out[r] = flip ? rec_q_len[r] - q_st[r] : q_en[r];
        }
        if (!part || !(passes(r) && (!do_filter || paired_len < fspan[key]))) continue; // paf.rs:100
        if (info->n_kept < kept_cap) kept[info->n_kept] = (uint32_t)r;
        else info->overflow = 1;
        info->n_kept++;
        if (flip) info->n_flipped_rows++;
    }
    return RB_OK;
}

// ---- the box: what this GPU moves at the clip kernel's memory mix, and the clock it holds meanwhile (diagnostics for bench.py) ----
extern "C" int rb_dev_box_probe(rb_ctx *ctx, const void *src, uint64_t src_bytes, void *dst0, void *dst1, int reps, int scatter, double *ms_out, double *mhz_out) {
    if (!ctx || !src || !dst0 || !dst1 || !ms_out || reps < 1) return RB_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const uint64_t n_stretch = src_bytes / (10 * 2048);
    if (n_stretch == 0) return RB_E_INVALID;
    uint32_t *stamps = nullptr;
    HIPCHK(ctx, hipMalloc((void **)&stamps, 64));
    hipEvent_t a = nullptr, b = nullptr;
    int rc = RB_OK;
    auto chk = [&](hipError_t e) {
        if (e != hipSuccess && rc == RB_OK) rc = fail(ctx, RB_E_HIP, "rb_dev_box_probe: %s", hipGetErrorString(e));
    };
    chk(hipEventCreate(&a));
    chk(hipEventCreate(&b));
    chk(rb_launch_box_probe(src, dst0, dst1, n_stretch, stamps, scatter, ctx->stream)); // (untimed: first touch)
    chk(rb_fill_async(stamps, 0, 64, ctx->stream));
    chk(hipEventRecord(a, ctx->stream));
    for (int i = 0; i < reps && rc == RB_OK; i++) chk(rb_launch_box_probe(src, dst0, dst1, n_stretch, stamps, scatter, ctx->stream));
    chk(hipEventRecord(b, ctx->stream));
    chk(hipEventSynchronize(b));
    float ms = 0;
    if (rc == RB_OK) chk(hipEventElapsedTime(&ms, a, b));
    uint32_t h[4] = {0, 0, 0, 0};
    if (rc == RB_OK) chk(hipMemcpy(h, stamps, 16, hipMemcpyDeviceToHost));
    *ms_out = ms / reps;
    if (mhz_out) *mhz_out = h[1] ? (double)h[0] * 64.0 / (double)h[1] * 100.0 : 0.0; // cycles per 10 ns tick x 100 MHz
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
    (void)hipFree(stamps);
    return rc;
}

// ---- a buffer that will be WRITTEN at the clip kernel's rate, placed by measurement ----
// On MI355X the time of a launch that streams its output into a buffer depends on WHICH physical pages the buffer has: the same
// process, the same launch, the output arena allocated four times over -- 9.10, 9.17, 9.25 and 11.04 ms (profiles/r04_alloc_summary.md).
// Reads do not care; writes do, and the library's store sweep (the box probe's write side alone, over the whole buffer) sees most of
// it.  rb_dev_alloc_placed allocates up to `tries` candidates of `bytes` (fewer when the device has not the room: a candidate is only
// taken while twice its size stays free), times the sweep on each, keeps the fastest and gives the others back.  sweep_ms[i] (may be
// NULL, room for `tries`) = what candidate i took, -1 where none was made; *kept = the index of the one returned.
// rb_dev_alloc_placed_by: the same with the caller's own measure -- score(candidate, user) is called once per candidate, with nothing
// of the library locked, and may launch on the context (bench.py: the clip kernel itself on its batch, which is what the placement
// is for; the store sweep ranks a 9.9 ms arena behind a 10.1 ms one now and then).  The lowest score wins; a negative score ends the
// search with RB_E_INVALID.
extern "C" int rb_dev_alloc_placed_by(rb_ctx *ctx, uint64_t bytes, int tries, double (*score)(void *candidate, void *user), void *user, void **out,
                                      double *scores, int *kept);
namespace {
struct sweep_arg { rb_ctx *ctx; uint64_t half; int rc; };
double sweep_score(void *q, void *user) {
    sweep_arg *a = (sweep_arg *)user;
    double t0 = 0, t1 = 0;
    char *p0 = (char *)q, *p1 = (char *)q + a->half;
    int r = rb_dev_box_probe(a->ctx, p0, a->half, p0, p1, 3, 1 | 8, &t0, nullptr); // (8: no loads -- src is not read)
    if (r == RB_OK) r = rb_dev_box_probe(a->ctx, p1, a->half, p1, p0, 3, 1 | 8, &t1, nullptr);
    if (r != RB_OK) {
        a->rc = r;
        return -1.0;
    }
    return t0 + t1;
}
} // namespace
extern "C" int rb_dev_alloc_placed(rb_ctx *ctx, uint64_t bytes, int tries, void **out, double *sweep_ms, int *kept) {
    if (!ctx || !out || tries < 1) return RB_E_INVALID;
    sweep_arg a{ctx, bytes / 2 / 20480 * 20480, RB_OK}; // (the sweep writes 20 KiB stretches: the buffer as two halves, each one fully written once)
    const bool sweep = a.half >= 20480 && tries > 1;
    const int rc = rb_dev_alloc_placed_by(ctx, bytes, sweep ? tries : 1, sweep ? sweep_score : nullptr, &a, out, sweep_ms, kept);
    for (int i = 1; sweep_ms && !sweep && i < tries; i++) sweep_ms[i] = -1.0;
    return (rc != RB_OK && a.rc != RB_OK) ? a.rc : rc;
}
extern "C" int rb_dev_alloc_placed_by(rb_ctx *ctx, uint64_t bytes, int tries, double (*score)(void *candidate, void *user), void *user, void **out,
                                      double *sweep_ms, int *kept) {
    if (!ctx || !out || tries < 1) return RB_E_INVALID;
    *out = nullptr;
    if (kept) *kept = -1;
    for (int i = 0; sweep_ms && i < tries; i++) sweep_ms[i] = -1.0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (tries > 1) { // a buffer of this size that this context placed before and released (rb_dev_release): as it is, nothing is measured again
        const size_t want = bytes ? ((bytes + 255) & ~(size_t)255) : 256;
        for (size_t k = 0; k < ctx->cache.size(); k++)
            if (ctx->cache[k].bytes == want && ctx->cache[k].placed) {
                *out = ctx->cache[k].p;
                ctx->cache_bytes -= want;
                ctx->cache.erase(ctx->cache.begin() + (long)k);
                return RB_OK; // (*kept = -1, every score -1: no candidate was made)
            }
    }
    std::vector<void *> cand;
    std::vector<double> ms;
    int rc = RB_OK, best = -1;
    for (int i = 0; i < tries && rc == RB_OK; i++) {
        if (i > 0) { // (never the last of the memory: the winner's neighbours -- workspace, rows -- still have to fit)
            size_t fr = 0, tot = 0;
            if (hipMemGetInfo(&fr, &tot) != hipSuccess || (uint64_t)fr < 2 * bytes + ((uint64_t)8 << 30)) break;
        }
        void *q = nullptr;
        const auto t_a = std::chrono::steady_clock::now();
        const int r1 = rb_dev_alloc(ctx, bytes, &q);
        if (r1 != RB_OK) {
            if (i == 0) rc = r1;
            break;
        }
        if (getenv("RB_ALLOC_LOG"))
            fprintf(stderr, "[rb_dev_alloc_placed] candidate %d: %.2f s to allocate\n", i, std::chrono::duration<double>(std::chrono::steady_clock::now() - t_a).count());
        cand.push_back(q);
        double t = 0;
        if (score && tries > 1) {
            t = score(q, user);
            if (!(t >= 0)) {
                rc = fail(ctx, RB_E_INVALID, "rb_dev_alloc_placed_by: the score of candidate %d is negative", i);
                break;
            }
        }
        ms.push_back(t);
        if (sweep_ms) sweep_ms[i] = t;
        if (best < 0 || t < ms[(size_t)best]) best = i;
    }
    const auto t_f = std::chrono::steady_clock::now();
    for (size_t i = 0; i < cand.size(); i++)
        if ((int)i != best || rc != RB_OK) {
            const int r3 = rb_dev_free(ctx, cand[i]);
            if (r3 != RB_OK && rc == RB_OK) rc = r3;
        }
    if (getenv("RB_ALLOC_LOG"))
        fprintf(stderr, "[rb_dev_alloc_placed] %zu candidates, kept %d, %.2f s to give the others back\n", cand.size(), best,
                std::chrono::duration<double>(std::chrono::steady_clock::now() - t_f).count());
    if (rc != RB_OK) return rc;
    *out = cand[(size_t)best];
    if (kept) *kept = best;
    if (cand.size() > 1) { // chosen by measurement: the context's cache keeps that in mind (rb_dev_release)
        std::lock_guard<std::mutex> lk(g_vmm_mu);
        auto it = g_vmm.find(*out);
        if (it != g_vmm.end()) it->second.placed = true;
    }
    return RB_OK;
}

// ---- nucfreq ----------------------------------------------------------------------------------------------------------
namespace {
struct nf_layout {
    size_t end_key, rd_end, tile_off, blk, tile_lo, tile_hi, drop_off, deep_list, drop_pool, tdesc, wide_list, total;
    uint64_t max_tiles, drop_words;
};
nf_layout nf_ws_layout(uint64_t n_reads, uint64_t n_regions, uint64_t n_positions) {
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    nf_layout L;
    L.max_tiles = n_positions / rb_nf_tile_positions() + n_regions;
    size_t o = 0;
    L.end_key = o, o = up(o + ((size_t)n_reads + 1) * 8);
    L.rd_end = o, o = up(o + ((size_t)n_reads + 1) * 48);
    L.tile_off = o, o = up(o + ((size_t)n_regions + 2) * 8);
    L.blk = o, o = up(o + (std::max(rb_nf_scan_blocks(n_reads), rb_scan_block_sums_count(n_regions)) + 2) * 8);
    L.tile_lo = o, o = up(o + ((size_t)L.max_tiles + 1) * 8);
    L.tile_hi = o, o = up(o + ((size_t)L.max_tiles + 1) * 8);
    // the depth cap's bookkeeping: a bitmap of dropped reads per region that can reach the cap, from a pool of 64 bits per read
    L.drop_off = o, o = up(o + ((size_t)n_regions + 1) * 8);
    L.deep_list = o, o = up(o + ((size_t)n_regions + 2) * 4);
    L.drop_words = n_reads + 1024;
    L.drop_pool = o, o = up(o + ((size_t)L.drop_words + 1) * 8); // (word 0: the pool's cursor)
    L.tdesc = o, o = up(o + ((size_t)L.max_tiles + 1) * 64);     // one 64-byte descriptor per tile (rb_k_nf_tile_desc)
    L.wide_list = o, o = up(o + ((size_t)L.max_tiles + 2) * 4);  // the tiles of the 16-bit build: count, then indices
    L.total = o;
    return L;
}
} // namespace

extern "C" size_t rb_nucfreq_workspace_bytes(uint64_t n_reads, uint64_t n_regions, uint64_t n_positions) {
    return nf_ws_layout(n_reads, n_regions, n_positions).total;
}

extern "C" int rb_dev_nucfreq(rb_ctx *ctx, const rb_reads_view *reads, uint64_t n_regions, const int32_t *rg_tid, const uint64_t *rg_st,
                              const uint64_t *rg_en, const uint64_t *out_off, uint64_t n_positions, uint32_t *counts, uint32_t *read_status,
                              rb_nucfreq_counters *counters, void *ws, size_t ws_bytes) {
    if (!ctx || !reads || !counters || (n_regions && (!rg_tid || !rg_st || !rg_en || !out_off)) || (n_positions && !counts)) return RB_E_INVALID;
    if (reads->n_reads && (!reads->ops || !reads->op_off || !reads->seq || !reads->seq_off || !reads->l_seq || !reads->tid || !reads->pos ||
                           !reads->flag || !read_status))
        return RB_E_INVALID;
    const nf_layout L = nf_ws_layout(reads->n_reads, n_regions, n_positions);
    if (!ws || ((uintptr_t)ws & 255) || ws_bytes < L.total) return fail(ctx, RB_E_INVALID, "nucfreq workspace: %zu bytes, 256-byte aligned, needed", L.total);
    if (L.max_tiles >= 0x7FFFFFFFull) return fail(ctx, RB_E_INVALID, "nucfreq: too many positions for one call");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, rb_fill_async(counters, 0, sizeof(rb_nucfreq_counters), ctx->stream));
    uint8_t *w = (uint8_t *)ws;
    rb_nf_params p{};
    p.n_reads = reads->n_reads;
    p.ops = reads->ops, p.op_off = reads->op_off, p.seq = reads->seq, p.seq_off = reads->seq_off, p.l_seq = reads->l_seq;
    p.tid = reads->tid, p.pos = reads->pos, p.flag = reads->flag;
    p.n_regions = n_regions;
    p.rg_tid = rg_tid, p.rg_st = rg_st, p.rg_en = rg_en, p.out_off = out_off;
    p.counts = counts, p.read_status = read_status, p.counters = counters;
    p.end_key = (uint64_t *)(w + L.end_key), p.hd = (nf_read *)(w + L.rd_end), p.tile_off = (uint64_t *)(w + L.tile_off);
    p.blk = (uint64_t *)(w + L.blk), p.tile_lo = (uint64_t *)(w + L.tile_lo), p.tile_hi = (uint64_t *)(w + L.tile_hi);
    p.max_tiles = L.max_tiles;
    p.drop_off = (uint64_t *)(w + L.drop_off), p.deep_list = (uint32_t *)(w + L.deep_list);
    p.drop_bits = (uint64_t *)(w + L.drop_pool) + 1, p.drop_words = L.drop_words;
    p.flags = 0;
    p.tdesc = (nf_tdesc *)(w + L.tdesc);
    p.wide_list = (uint32_t *)(w + L.wide_list);
    HIPCHK(ctx, rb_fill_async(p.drop_bits - 1, 0, 8, ctx->stream));
    HIPCHK(ctx, rb_fill_async(p.deep_list + n_regions, 0, 8, ctx->stream)); // (how many deep regions; can the cap be reached at all)
    HIPCHK(ctx, rb_launch_nucfreq(&p, ctx->stream));
    return RB_OK;
}

namespace {
// the reads, the regions and the outputs of one rb_dev_nucfreq call made from host arrays, resident until this goes out of scope
struct NfDev {
    DevBatch b;
    std::vector<uint64_t> out_off, opo, sqo; // (the asynchronous uploads read them until the stream is synchronised)
    uint64_t n_pos = 0;
    uint32_t *d_counts = nullptr;
    explicit NfDev(rb_ctx *c) : b(c) {}
    // where the regions' counts go: region r at the sum of en - st of the regions in front
    int layout(rb_ctx *ctx, uint64_t n_regions, const uint64_t *rg_st, const uint64_t *rg_en) {
        out_off.assign(n_regions + 1, 0);
        for (uint64_t r = 0; r < n_regions; r++) {
            if (rg_en[r] < rg_st[r]) return fail(ctx, RB_E_INVALID, "region %llu ends before it starts", (unsigned long long)r);
            out_off[r + 1] = out_off[r] + (rg_en[r] - rg_st[r]);
        }
        n_pos = out_off[n_regions];
        return RB_OK;
    }
    // upload, rb_dev_nucfreq into d_counts, counters and read_status back (layout() first).  resident: *reads is a DEVICE view already
    // (rb_devreads_nucfreq) and nothing of the reads goes up
    int run(rb_ctx *ctx, const rb_reads_view *reads, bool resident, uint64_t n_regions, const int32_t *rg_tid, const uint64_t *rg_st,
            const uint64_t *rg_en, uint32_t *read_status, rb_nucfreq_counters *counters) {
        const uint64_t n = reads->n_reads;
        rb_reads_view d{};
        d.n_reads = n;
        int rc;
        if (resident) {
            d = *reads;
        } else if (n) {
            // only the part of ops / seq these reads use goes up, offsets rebased
            const uint64_t op0 = reads->op_off[0], op1 = reads->op_off[n];
            uint64_t s0 = ~0ull, s1 = 0;
            for (uint64_t i = 0; i < n; i++) {
                const uint64_t a = reads->seq_off[i], e = a + ((uint64_t)reads->l_seq[i] + 1) / 2;
                s0 = std::min(s0, a), s1 = std::max(s1, e);
            }
            opo.resize(n + 1), sqo.resize(n);
            for (uint64_t i = 0; i <= n; i++) opo[i] = reads->op_off[i] - op0;
            for (uint64_t i = 0; i < n; i++) sqo[i] = reads->seq_off[i] - s0;
            if ((rc = b.up(reads->ops + op0, (size_t)(op1 - op0), &d.ops))) return rc;
            if ((rc = b.up(opo.data(), (size_t)n + 1, &d.op_off))) return rc;
            {   // (32 readable bytes behind the last read, as the kernel asks)
                uint8_t *dsq = nullptr;
                if ((rc = b.alloc((size_t)(s1 - s0) + 32, &dsq))) return rc;
                if (s1 > s0 && (rc = rb_dev_upload(ctx, dsq, reads->seq + s0, (size_t)(s1 - s0)))) return rc;
                d.seq = dsq;
            }
            if ((rc = b.up(sqo.data(), (size_t)n, &d.seq_off))) return rc;
            if ((rc = b.up(reads->l_seq, (size_t)n, &d.l_seq))) return rc;
            if ((rc = b.up(reads->tid, (size_t)n, &d.tid))) return rc;
            if ((rc = b.up(reads->pos, (size_t)n, &d.pos))) return rc;
            if ((rc = b.up(reads->flag, (size_t)n, &d.flag))) return rc;
        }
        const int32_t *d_tid = nullptr;
        const uint64_t *d_st = nullptr, *d_en = nullptr, *d_off = nullptr;
        if ((rc = b.up(rg_tid, (size_t)n_regions, &d_tid))) return rc;
        if ((rc = b.up(rg_st, (size_t)n_regions, &d_st))) return rc;
        if ((rc = b.up(rg_en, (size_t)n_regions, &d_en))) return rc;
        if ((rc = b.up(out_off.data(), (size_t)n_regions + 1, &d_off))) return rc;
        uint32_t *d_status = nullptr;
        rb_nucfreq_counters *d_ctr = nullptr;
        uint8_t *d_ws = nullptr;
        if ((rc = b.alloc((size_t)n_pos * 4 + 4, &d_counts))) return rc;
        if ((rc = b.alloc((size_t)n + 1, &d_status))) return rc;
        if ((rc = b.alloc(1, &d_ctr))) return rc;
        const size_t wsb = rb_nucfreq_workspace_bytes(n, n_regions, n_pos);
        if ((rc = b.alloc(wsb, &d_ws))) return rc;
        if ((rc = rb_dev_nucfreq(ctx, &d, n_regions, d_tid, d_st, d_en, d_off, n_pos, d_counts, d_status, d_ctr, d_ws, wsb))) return rc;
        if ((rc = rb_dev_download(ctx, counters, d_ctr, sizeof(*counters)))) return rc;
        if (read_status && n && (rc = rb_dev_download(ctx, read_status, d_status, (size_t)n * 4))) return rc;
        return RB_OK;
    }
};
// counts that are not the reference's
int nf_refuse(rb_ctx *ctx, const rb_nucfreq_counters *counters) {
    if (counters->unsorted) return fail(ctx, RB_E_INVALID, "nucfreq: the reads are not sorted by (tid, pos)");
    if (counters->cap_overflow)
        return fail(ctx, RB_E_INVALID, "nucfreq: the bookkeeping of htslib's cap of %u buffered reads does not fit (depth %llu)", RB_NF_DEPTH_CAP,
                    (unsigned long long)counters->max_depth);
    if (counters->max_depth > 65535) return fail(ctx, RB_E_INVALID, "nucfreq: depth %llu does not fit the 16-bit counters", (unsigned long long)counters->max_depth);
    return RB_OK;
}
} // namespace

static int nf_counts(rb_ctx *ctx, const rb_reads_view *reads, bool resident, uint64_t n_regions, const int32_t *rg_tid, const uint64_t *rg_st,
                     const uint64_t *rg_en, uint32_t *counts, uint32_t *read_status, rb_nucfreq_counters *counters) {
    if (!ctx || !reads || !counters || (n_regions && (!rg_tid || !rg_st || !rg_en))) return RB_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    NfDev D(ctx);
    int rc;
    if ((rc = D.layout(ctx, n_regions, rg_st, rg_en))) return rc;
    if (D.n_pos && !counts) return RB_E_INVALID;
    if ((rc = D.run(ctx, reads, resident, n_regions, rg_tid, rg_st, rg_en, read_status, counters))) return rc;
    if (D.n_pos && (rc = rb_dev_download(ctx, counts, D.d_counts, (size_t)D.n_pos * 16))) return rc;
    return nf_refuse(ctx, counters);
}
extern "C" int rb_host_nucfreq(rb_ctx *ctx, const rb_reads_view *reads, uint64_t n_regions, const int32_t *rg_tid, const uint64_t *rg_st,
                               const uint64_t *rg_en, uint32_t *counts, uint32_t *read_status, rb_nucfreq_counters *counters) {
    return nf_counts(ctx, reads, false, n_regions, rg_tid, rg_st, rg_en, counts, read_status, counters);
}
extern "C" int rb_devreads_nucfreq(rb_ctx *ctx, const rb_reads_view *reads, uint64_t n_regions, const int32_t *rg_tid, const uint64_t *rg_st,
                                   const uint64_t *rg_en, uint32_t *counts, uint32_t *read_status, rb_nucfreq_counters *counters) {
    if (ctx && reads && ((uintptr_t)reads->seq & 3u)) return fail(ctx, RB_E_INVALID, "rb_devreads_nucfreq: seq must be 4-byte aligned");
    return nf_counts(ctx, reads, true, n_regions, rg_tid, rg_st, rg_en, counts, read_status, counters);
}

// ---- nucfreq: the lines (k_nftext.hip) ------------------------------------------------------------------------------------
namespace {
struct nft_layout {
    size_t seg, unit0, unit_off, blk, total;
    uint64_t max_units;
};
nft_layout nft_scratch_layout(uint64_t n_seg, uint64_t n_positions) {
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    nft_layout L;
    L.max_units = n_positions / rb_nft_run() + n_seg; // a segment of n positions is ceil(n / run) runs
    size_t o = 0;
    L.seg = o, o = up(o + (size_t)n_seg * sizeof(rb_nft_seg));
    L.unit0 = o, o = up(o + ((size_t)n_seg + 1) * 4);
    L.unit_off = o, o = up(o + ((size_t)L.max_units + 2) * 8);
    L.blk = o, o = up(o + (rb_scan_block_sums_count(L.max_units) + 4) * 8);
    L.total = o;
    return L;
}
} // namespace

extern "C" size_t rb_nucfreq_text_scratch_bytes(uint64_t n_seg, uint64_t n_positions) { return nft_scratch_layout(n_seg, n_positions).total; }
extern "C" void rb_nucfreq_text_shape(uint32_t out[4]) {
    out[0] = rb_nft_step(), out[1] = rb_nft_block(), out[2] = rb_nft_fix(), out[3] = rb_nft_fix();
}

extern "C" int rb_dev_nucfreq_text(rb_ctx *ctx, const uint32_t *counts, uint64_t n_seg, const uint64_t *seg_cnt, const uint64_t *seg_pos,
                                   const uint32_t *seg_n, const uint8_t *strings, const uint32_t *pre_off, const uint32_t *pre_len,
                                   const uint32_t *suf_off, const uint32_t *suf_len, int mode, uint64_t *seg_text_off, uint64_t *seg_first,
                                   uint64_t *seg_lines, uint8_t *text, uint64_t text_cap, void *scratch) {
    if (!ctx) return RB_E_INVALID;
    if (mode != RB_NFT_FULL && mode != RB_NFT_SMALL) return fail(ctx, RB_E_INVALID, "nucfreq text: mode %d is neither RB_NFT_FULL nor RB_NFT_SMALL", mode);
    if (!seg_text_off || !scratch || (n_seg && (!seg_cnt || !seg_pos || !seg_n || !seg_first || !seg_lines)))
        return fail(ctx, RB_E_INVALID, "nucfreq text: a pointer that is needed is NULL");
    if (mode == RB_NFT_FULL && n_seg && (!strings || !pre_off || !pre_len || !suf_off || !suf_len))
        return fail(ctx, RB_E_INVALID, "nucfreq text: RB_NFT_FULL needs strings and the prefix and suffix arrays");
    if (n_seg >= 0xFFFFFFFFull) return fail(ctx, RB_E_INVALID, "nucfreq text: too many segments for one call");
    if (((uintptr_t)counts & 15u) || ((uintptr_t)text & 15u) || ((uintptr_t)scratch & 255u))
        return fail(ctx, RB_E_INVALID, "nucfreq text: counts and text must be 16-byte aligned, the scratch 256-byte aligned");
    // the segments as the kernel reads them, and the runs numbered through
    std::vector<rb_nft_seg> seg((size_t)n_seg);
    std::vector<uint32_t> unit0((size_t)n_seg + 1);
    uint64_t n_units = 0, n_positions = 0;
    for (uint64_t s = 0; s < n_seg; s++) {
        if (seg_pos[s] > (1ull << 32) || seg_pos[s] + seg_n[s] > (1ull << 32))
            return fail(ctx, RB_E_INVALID, "nucfreq text: segment %llu reaches behind position 2^32", (unsigned long long)s);
        rb_nft_seg &g = seg[(size_t)s];
        g.cnt = seg_cnt[s], g.pos = (uint32_t)seg_pos[s], g.n = seg_n[s];
        g.pre_off = g.suf_off = g.pre_len = g.suf_len = 0;
        if (mode == RB_NFT_FULL) {
            if (pre_len[s] > rb_nft_fix() || suf_len[s] > rb_nft_fix())
                return fail(ctx, RB_E_INVALID, "nucfreq text: the prefix or suffix of segment %llu is longer than %u bytes", (unsigned long long)s, rb_nft_fix());
            g.pre_off = pre_off[s], g.suf_off = suf_off[s], g.pre_len = pre_len[s], g.suf_len = suf_len[s];
        }
        unit0[(size_t)s] = (uint32_t)n_units;
        n_units += ((uint64_t)seg_n[s] + rb_nft_run() - 1) / rb_nft_run();
        n_positions += seg_n[s];
        if (n_units >= 0xFFFFFFFFull) return fail(ctx, RB_E_INVALID, "nucfreq text: too many positions for one call");
    }
    unit0[(size_t)n_seg] = (uint32_t)n_units;
    if (n_units && !counts) return fail(ctx, RB_E_INVALID, "nucfreq text: counts is NULL");
    const nft_layout L = nft_scratch_layout(n_seg, n_positions);
    uint8_t *w = (uint8_t *)scratch;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc;
    if (n_seg && (rc = rb_dev_upload(ctx, w + L.seg, seg.data(), seg.size() * sizeof(rb_nft_seg)))) return rc; // (consumed when it returns)
    if ((rc = rb_dev_upload(ctx, w + L.unit0, unit0.data(), unit0.size() * 4))) return rc;
    rb_nft_params p{};
    p.counts = counts, p.n_seg = n_seg, p.seg = (const rb_nft_seg *)(w + L.seg), p.unit0 = (const uint32_t *)(w + L.unit0), p.n_units = n_units;
    p.strings = strings, p.mode = mode;
    p.unit_off = (uint64_t *)(w + L.unit_off);
    p.seg_text_off = seg_text_off, p.seg_first = seg_first, p.seg_lines = seg_lines;
    p.text = text, p.text_cap = text_cap;
    if (n_seg) {
        HIPCHK(ctx, rb_fill_async(seg_first, 0xFF, (size_t)n_seg * 8, ctx->stream));
        HIPCHK(ctx, rb_fill_async(seg_lines, 0, (size_t)n_seg * 8, ctx->stream));
    }
    HIPCHK(ctx, rb_fill_async(p.unit_off + n_units, 0, 8, ctx->stream));
    HIPCHK(ctx, rb_launch_nft(&p, false, ctx->stream));
    HIPCHK(ctx, rb_launch_exclusive_scan(p.unit_off, n_units, (uint64_t *)(w + L.blk), nullptr, ctx->stream));
    HIPCHK(ctx, rb_launch_nft_seg_off(&p, ctx->stream));
    if (text) HIPCHK(ctx, rb_launch_nft(&p, true, ctx->stream));
    return RB_OK;
}

typedef void (*nft_sink)(void *user, uint64_t first_seg, uint64_t n_seg, const uint64_t *seg_text_off, const uint64_t *seg_first, const uint8_t *text);
static int nf_text(rb_ctx *ctx, const rb_reads_view *reads, bool resident, uint64_t n_regions, const int32_t *rg_tid, const uint64_t *rg_st,
                   const uint64_t *rg_en, uint64_t n_seg, const uint64_t *seg_cnt, const uint64_t *seg_pos, const uint32_t *seg_n, const uint8_t *strings,
                   uint64_t strings_bytes, const uint32_t *pre_off, const uint32_t *pre_len, const uint32_t *suf_off, const uint32_t *suf_len, int mode,
                   uint32_t *read_status, rb_nucfreq_counters *counters, nft_sink sink, void *user) {
    if (!ctx || !reads || !counters || !sink || (n_regions && (!rg_tid || !rg_st || !rg_en))) return RB_E_INVALID;
    if (n_seg && (!seg_cnt || !seg_pos || !seg_n)) return RB_E_INVALID;
    if (mode == RB_NFT_FULL && n_seg && (!pre_off || !pre_len || !suf_off || !suf_len || (strings_bytes && !strings))) return RB_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    NfDev D(ctx);
    int rc;
    if ((rc = D.layout(ctx, n_regions, rg_st, rg_en))) return rc;
    uint64_t seg_positions = 0;
    for (uint64_t s = 0; s < n_seg; s++) {
        if (seg_cnt[s] > D.n_pos || seg_n[s] > D.n_pos - seg_cnt[s])
            return fail(ctx, RB_E_INVALID, "nucfreq text: segment %llu lies outside the %llu positions of the regions", (unsigned long long)s, (unsigned long long)D.n_pos);
        seg_positions += seg_n[s];
        if (mode == RB_NFT_FULL && ((uint64_t)pre_off[s] + pre_len[s] > strings_bytes || (uint64_t)suf_off[s] + suf_len[s] > strings_bytes))
            return fail(ctx, RB_E_INVALID, "nucfreq text: a string of segment %llu lies outside strings", (unsigned long long)s);
    }
    if ((rc = D.run(ctx, reads, resident, n_regions, rg_tid, rg_st, rg_en, read_status, counters))) return rc;
    if ((rc = nf_refuse(ctx, counters))) return rc;
    if (n_seg == 0) return RB_OK;
    // sizes first, then runs of whole segments into a bounded buffer
    const uint8_t *d_strings = nullptr;
    if ((rc = D.b.up(strings, (size_t)strings_bytes, &d_strings))) return rc;
    uint64_t *d_off = nullptr, *d_first = nullptr, *d_lines = nullptr;
    uint8_t *d_scr = nullptr, *d_text = nullptr;
    if ((rc = D.b.alloc((size_t)n_seg + 1, &d_off)) || (rc = D.b.alloc((size_t)n_seg, &d_first)) || (rc = D.b.alloc((size_t)n_seg, &d_lines))) return rc;
    if ((rc = D.b.alloc(rb_nucfreq_text_scratch_bytes(n_seg, seg_positions) + 256, &d_scr))) return rc;
    d_scr = (uint8_t *)(((uintptr_t)d_scr + 255) & ~(uintptr_t)255);
    if ((rc = rb_dev_nucfreq_text(ctx, D.d_counts, n_seg, seg_cnt, seg_pos, seg_n, d_strings, pre_off, pre_len, suf_off, suf_len, mode, d_off, d_first,
                                  d_lines, nullptr, 0, d_scr)))
        return rc;
    std::vector<uint64_t> off((size_t)n_seg + 1), first((size_t)n_seg), rel;
    if ((rc = rb_dev_download(ctx, off.data(), d_off, off.size() * 8)) || (rc = rb_dev_download(ctx, first.data(), d_first, first.size() * 8))) return rc;
    uint64_t SLAB = 1ull << 30;
    if (const char *e = getenv("RB_DEBUG_NFT_SLAB")) SLAB = std::max<uint64_t>(strtoull(e, nullptr, 10), 1); // tests: several slabs, and a segment longer than one, at a small size
    uint64_t cap = 0; // the largest slab: whole segments up to SLAB bytes, a longer segment alone
    for (uint64_t s0 = 0, s1; s0 < n_seg; s0 = s1) {
        for (s1 = s0 + 1; s1 < n_seg && off[(size_t)s1 + 1] - off[(size_t)s0] <= SLAB; s1++) {}
        cap = std::max(cap, off[(size_t)s1] - off[(size_t)s0]);
    }
    uint8_t *h_text = nullptr;
    if (cap) {
        if ((rc = D.b.alloc((size_t)cap + 16, &d_text))) return rc;
        h_text = (uint8_t *)malloc((size_t)cap);
        if (!h_text) return fail(ctx, RB_E_NOMEM, "nucfreq text: %llu bytes of host memory", (unsigned long long)cap);
        rb_advise_huge(h_text, (size_t)cap);
    }
    for (uint64_t s0 = 0, s1; s0 < n_seg; s0 = s1) {
        for (s1 = s0 + 1; s1 < n_seg && off[(size_t)s1 + 1] - off[(size_t)s0] <= SLAB; s1++) {}
        const uint64_t bytes = off[(size_t)s1] - off[(size_t)s0];
        if (bytes) {
            rc = rb_dev_nucfreq_text(ctx, D.d_counts, s1 - s0, seg_cnt + s0, seg_pos + s0, seg_n + s0, d_strings, pre_off ? pre_off + s0 : nullptr,
                                     pre_len ? pre_len + s0 : nullptr, suf_off ? suf_off + s0 : nullptr, suf_len ? suf_len + s0 : nullptr, mode, d_off,
                                     d_first, d_lines, d_text, bytes, d_scr);
            if (!rc) rc = rb_dev_download(ctx, h_text, d_text, (size_t)bytes);
            if (rc) {
                free(h_text);
                return rc;
            }
        }
        rel.resize((size_t)(s1 - s0) + 1);
        for (uint64_t s = s0; s <= s1; s++) rel[(size_t)(s - s0)] = off[(size_t)s] - off[(size_t)s0];
        sink(user, s0, s1 - s0, rel.data(), first.data() + s0, h_text);
    }
    free(h_text);
    return RB_OK;
}
extern "C" int rb_host_nucfreq_text(rb_ctx *ctx, const rb_reads_view *reads, uint64_t n_regions, const int32_t *rg_tid, const uint64_t *rg_st,
                                    const uint64_t *rg_en, uint64_t n_seg, const uint64_t *seg_cnt, const uint64_t *seg_pos, const uint32_t *seg_n,
                                    const uint8_t *strings, uint64_t strings_bytes, const uint32_t *pre_off, const uint32_t *pre_len,
                                    const uint32_t *suf_off, const uint32_t *suf_len, int mode, uint32_t *read_status, rb_nucfreq_counters *counters,
                                    void (*sink)(void *user, uint64_t first_seg, uint64_t n_seg, const uint64_t *seg_text_off,
                                                 const uint64_t *seg_first, const uint8_t *text),
                                    void *user) {
    return nf_text(ctx, reads, false, n_regions, rg_tid, rg_st, rg_en, n_seg, seg_cnt, seg_pos, seg_n, strings, strings_bytes, pre_off, pre_len, suf_off,
                   suf_len, mode, read_status, counters, sink, user);
}
extern "C" int rb_devreads_nucfreq_text(rb_ctx *ctx, const rb_reads_view *reads, uint64_t n_regions, const int32_t *rg_tid, const uint64_t *rg_st,
                                        const uint64_t *rg_en, uint64_t n_seg, const uint64_t *seg_cnt, const uint64_t *seg_pos, const uint32_t *seg_n,
                                        const uint8_t *strings, uint64_t strings_bytes, const uint32_t *pre_off, const uint32_t *pre_len,
                                        const uint32_t *suf_off, const uint32_t *suf_len, int mode, uint32_t *read_status, rb_nucfreq_counters *counters,
                                        void (*sink)(void *user, uint64_t first_seg, uint64_t n_seg, const uint64_t *seg_text_off,
                                                     const uint64_t *seg_first, const uint8_t *text),
                                        void *user) {
    if (ctx && reads && ((uintptr_t)reads->seq & 3u)) return fail(ctx, RB_E_INVALID, "rb_devreads_nucfreq_text: seq must be 4-byte aligned");
    return nf_text(ctx, reads, true, n_regions, rg_tid, rg_st, rg_en, n_seg, seg_cnt, seg_pos, seg_n, strings, strings_bytes, pre_off, pre_len, suf_off,
                   suf_len, mode, read_status, counters, sink, user);
}
