// pcpx_runtime.hip -- what the entry points of every source stand on: the thread's error text, the device pools and caches,
// the pinned upload ring and device selection.  The prologues that use them are in pcpx_internal.h.
#include "pcpx_internal.h"

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <unordered_map>

namespace pcpx {

thread_local std::string g_err;

void set_error(const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    try {
        g_err = buf;
    } catch (...) {  // (out of host memory: the text is lost, the code still tells; nothing leaves through the ABI)
    }
}

int check_hip(hipError_t e, const char* what, const char* file, int line)
{
    if (e == hipSuccess) return PCPX_OK;
    set_error("HIP error %d (%s) at %s:%d in %s", static_cast<int>(e), hipGetErrorString(e), file, line, what);
    (void)hipGetLastError();
    return (e == hipErrorOutOfMemory) ? PCPX_ERR_ALLOC : PCPX_ERR_DEVICE;
}

// ---- DevPool / PinnedStage (pcpx_internal.h) --------------------------------------------------------
void* DevPool::acquire(size_t bytes)
{
    if (bytes == 0) bytes = 16;
    int best = -1;
    for (size_t i = 0; i < blocks.size(); ++i)  // best fit among the free blocks that are not wastefully large
        if (!blocks[i].used && blocks[i].bytes >= bytes && blocks[i].bytes <= 2 * bytes + (1u << 20) &&
            (best < 0 || blocks[i].bytes < blocks[static_cast<size_t>(best)].bytes))
            best = static_cast<int>(i);
    if (best >= 0) {
        blocks[static_cast<size_t>(best)].used = true;
        return blocks[static_cast<size_t>(best)].p;
    }
    void* p = nullptr;
    const size_t rounded = (bytes + 4095) / 4096 * 4096;
    hipError_t e = hipMalloc(&p, rounded);
    if (e != hipSuccess) {  // give back what is cached and try once more
        (void)hipGetLastError();
        trim();
        e = hipMalloc(&p, rounded);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("hipMalloc(%zu bytes) failed: %s", rounded, hipGetErrorString(e));
        return nullptr;
    }
    blocks.push_back(Block{p, rounded, true});
    return p;
}
void DevPool::release(void* p)
{
    for (auto& b : blocks)
        if (b.p == p) {
            b.used = false;
            break;
        }
    // a cap on what sits idle: calls with differing sizes each leave a block behind (a block is reused only for a request of
    // at least half its size); beyond MAX_IDLE the largest idle blocks go back to the driver
    constexpr size_t MAX_IDLE = size_t(16) << 30;  // (of 288 GB)
    for (;;) {
        size_t idle = 0;
        int largest = -1;
        for (size_t i = 0; i < blocks.size(); ++i)
            if (!blocks[i].used) {
                idle += blocks[i].bytes;
                if (largest < 0 || blocks[i].bytes > blocks[static_cast<size_t>(largest)].bytes) largest = static_cast<int>(i);
            }
        if (idle <= MAX_IDLE || largest < 0) break;
        (void)hipFree(blocks[static_cast<size_t>(largest)].p);
        blocks.erase(blocks.begin() + largest);
    }
}
void DevPool::trim()
{
    size_t keep = 0;
    for (size_t i = 0; i < blocks.size(); ++i) {
        if (blocks[i].used) blocks[keep++] = blocks[i];
        else (void)hipFree(blocks[i].p);
    }
    blocks.resize(keep);
}
int DevPool::poison(int byte, hipStream_t s, u64* filled)
{
    for (auto const& b : blocks)
        if (!b.used) {
            PCPX_HIP(hipMemsetAsync(b.p, byte, b.bytes, s));
            *filled += b.bytes;
        }
    return PCPX_OK;
}
size_t DevPool::cached_bytes() const
{
    size_t t = 0;
    for (auto const& b : blocks) t += b.bytes;
    return t;
}
DevPool::~DevPool()
{
    for (auto& b : blocks) (void)hipFree(b.p);
}
// ---- device blocks of indexes, cached per device (pcpx_internal.h) ----------------------------------------------------------
namespace {
struct IndexBlocks {
    std::mutex mu;
    struct Idle {
        void* p;
        size_t bytes;
        int device;
    };
    std::vector<Idle> idle;
    std::unordered_map<void*, size_t> handed_out;  // block -> its real size
    size_t cap_bytes()
    {
        static const size_t cap = [] {
            const char* e = std::getenv("PCPX_DEVICE_CACHE_MB");
            const long long mb = e ? std::atoll(e) : 2048;
            return static_cast<size_t>(mb < 0 ? 0 : mb) << 20;
        }();
        return cap;
    }
};
IndexBlocks& index_blocks()
{
    static IndexBlocks* b = new IndexBlocks();  // (never destroyed: the HIP runtime may be gone by the time statics are)
    return *b;
}
void free_idle_blocks(IndexBlocks& c, int dev)  // (the caller holds c.mu)
{
    size_t keep = 0;
    for (size_t i = 0; i < c.idle.size(); ++i) {
        if (c.idle[i].device == dev) (void)hipFree(c.idle[i].p);
        else c.idle[keep++] = c.idle[i];
    }
    c.idle.resize(keep);
}
}  // namespace

hipError_t index_block_alloc(void** p, size_t bytes)
{
    *p = nullptr;
    if (bytes == 0) bytes = 16;
    int dev = 0;
    (void)hipGetDevice(&dev);
    IndexBlocks& c = index_blocks();
    std::lock_guard<std::mutex> lock(c.mu);
    int best = -1;
    for (size_t i = 0; i < c.idle.size(); ++i)
        if (c.idle[i].device == dev && c.idle[i].bytes >= bytes && c.idle[i].bytes <= bytes + bytes / 4 + (size_t(64) << 10) &&
            (best < 0 || c.idle[i].bytes < c.idle[static_cast<size_t>(best)].bytes))
            best = static_cast<int>(i);
    if (best >= 0) {
        *p = c.idle[static_cast<size_t>(best)].p;
        c.handed_out[*p] = c.idle[static_cast<size_t>(best)].bytes;
        c.idle.erase(c.idle.begin() + best);
        return hipSuccess;
    }
    const size_t rounded = (bytes + 4095) / 4096 * 4096;
    hipError_t e = hipMalloc(p, rounded);
    if (e == hipErrorOutOfMemory) {  // what sits idle here may be what is missing
        (void)hipGetLastError();
        free_idle_blocks(c, dev);
        e = hipMalloc(p, rounded);
    }
    if (e == hipSuccess) c.handed_out[*p] = rounded;
    else *p = nullptr;
    return e;
}

void index_block_free(void* p)
{
    if (!p) return;
    int dev = 0;
    (void)hipGetDevice(&dev);
    IndexBlocks& c = index_blocks();
    std::lock_guard<std::mutex> lock(c.mu);
    auto it = c.handed_out.find(p);
    if (it == c.handed_out.end()) {  // not one of ours (cannot happen; be safe)
        (void)hipFree(p);
        return;
    }
    const size_t bytes = it->second;
    c.handed_out.erase(it);
    size_t idle_here = 0;
    for (auto const& b : c.idle)
        if (b.device == dev) idle_here += b.bytes;
    bool keep = idle_here + bytes <= c.cap_bytes();
    if (keep && idle_here + bytes > (size_t(256) << 20)) {
        // beyond a quarter of a gigabyte the cache also yields to whoever else lives on the device (a co-resident framework sees idle
        // blocks as used memory): never more than a quarter of what is free now
        size_t free_now = 0, total = 0;
        if (hipMemGetInfo(&free_now, &total) == hipSuccess) keep = idle_here + bytes <= free_now / 4;
        else (void)hipGetLastError();
    }
    if (keep) c.idle.push_back(IndexBlocks::Idle{p, bytes, dev});
    else (void)hipFree(p);
}

void index_blocks_trim()
{
    int dev = 0;
    (void)hipGetDevice(&dev);
    IndexBlocks& c = index_blocks();
    std::lock_guard<std::mutex> lock(c.mu);
    free_idle_blocks(c, dev);
}

int index_blocks_poison(int byte, hipStream_t s, u64* filled)
{
    int dev = 0;
    (void)hipGetDevice(&dev);
    IndexBlocks& c = index_blocks();
    std::lock_guard<std::mutex> lock(c.mu);
    for (auto const& b : c.idle)
        if (b.device == dev) {
            PCPX_HIP(hipMemsetAsync(b.p, byte, b.bytes, s));
            *filled += b.bytes;
        }
    PCPX_HIP(hipStreamSynchronize(s));  // (before the cache's lock goes: the next index built on the device may take these blocks)
    return PCPX_OK;
}

namespace {
struct IdleStreams {
    std::mutex mu;
    std::vector<std::pair<int, hipStream_t>> idle;  // (device, stream)
};
IdleStreams& idle_streams()
{
    static IdleStreams* s = new IdleStreams();  // (never destroyed: the HIP runtime may be gone by the time statics are)
    return *s;
}
}  // namespace

hipError_t pooled_stream_get(hipStream_t* out)
{
    int dev = 0;
    (void)hipGetDevice(&dev);
    {
        IdleStreams& p = idle_streams();
        std::lock_guard<std::mutex> lock(p.mu);
        for (size_t i = 0; i < p.idle.size(); ++i)
            if (p.idle[i].first == dev) {
                *out = p.idle[i].second;
                p.idle.erase(p.idle.begin() + static_cast<long>(i));
                return hipSuccess;
            }
    }
    return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
}

void pooled_stream_put(hipStream_t s)
{
    if (!s) return;
    int dev = 0;
    (void)hipGetDevice(&dev);
    {
        IdleStreams& p = idle_streams();
        std::lock_guard<std::mutex> lock(p.mu);
        size_t here = 0;
        for (auto const& e : p.idle) here += e.first == dev ? 1u : 0u;
        if (here < 8) {
            p.idle.emplace_back(dev, s);
            return;
        }
    }
    (void)hipStreamDestroy(s);
}

int PinnedStage::ensure(size_t need)
{
    if (need <= bytes) return PCPX_OK;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    bytes = 0;
    const size_t want = need < (1u << 16) ? (1u << 16) : (need + 4095) / 4096 * 4096;
    hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
    if (e != hipSuccess) {
        p = nullptr;
        (void)hipGetLastError();
        set_error("hipHostMalloc(%zu bytes) failed: %s", want, hipGetErrorString(e));
        return PCPX_ERR_ALLOC;
    }
    bytes = want;
    *static_cast<volatile u32*>(p) = 0u;  // (the latency paths' completion word, when they keep it at offset 0)
    return PCPX_OK;
}
PinnedStage::~PinnedStage()
{
    if (p) (void)hipHostFree(p);
}

int wait_epoch(const volatile u32* done, u32 epoch, hipStream_t s)
{
    // poll the completion word the kernel stores into pinned memory: no trip through the runtime's completion signal (the stream
    // stays in order: the next launch on it runs after this kernel has retired)
    bool seen = false;
    for (u32 spin = 0; spin < 400000u && !seen; ++spin) seen = *done == epoch;
    if (!seen) PCPX_HIP(hipStreamSynchronize(s));
    std::atomic_thread_fence(std::memory_order_acquire);
    return PCPX_OK;
}

namespace {
template <class T>
T& per_device(int device)  // one T per device, made on first use
{
    static std::mutex table_mu;
    static std::vector<T*> table;  // never freed: the HIP runtime may be gone at exit
    std::lock_guard<std::mutex> lock(table_mu);
    if (static_cast<size_t>(device) >= table.size()) table.resize(static_cast<size_t>(device) + 1, nullptr);
    if (!table[static_cast<size_t>(device)]) table[static_cast<size_t>(device)] = new T();
    return *table[static_cast<size_t>(device)];
}
}  // namespace

DeviceShared& shared_of(int device) { return per_device<DeviceShared>(device); }

// Pageable host memory -> device on `stream`; the source may be reused when this returns (64 KB and more: the bytes have arrived).  hipMemcpy from a pageable buffer it has not seen before took 12-24 ms for 12 MB on this stack (0.5-1 GB/s: the 2^20-point
// cloud of a construction; 200 MB take 4-7 ms), against 0.46 ms for a host memcpy of 12 MB plus 0.29 ms for the same copy from pinned
// memory (tools/h2d_probe.hip).  So copies of up to 64 MB go through a per-device ring of two pinned 4-MB blocks --
// the host fills one while the other is on its way -- and larger ones are left to the runtime.
namespace {
struct Uploader {
    std::mutex mu;
    void* pin = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    static constexpr size_t CHUNK = size_t(4) << 20;
};
}  // namespace

int upload_pageable(void* d_dst, const void* src, size_t bytes, hipStream_t stream)
{
    if (bytes == 0) return PCPX_OK;
    if (bytes < (size_t(64) << 10)) {  // (a query or a few hundred: the runtime has taken its copy of a pageable source when this returns)
        PCPX_HIP(hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, stream));
        return PCPX_OK;
    }
    if (bytes > (size_t(64) << 20)) {
        PCPX_HIP(hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, stream));
        return check_hip(hipStreamSynchronize(stream), "upload", __FILE__, __LINE__);
    }
    int dev = 0;
    PCPX_HIP(hipGetDevice(&dev));
    Uploader& u = per_device<Uploader>(dev);
    std::lock_guard<std::mutex> lock(u.mu);
    if (!u.ev[1]) {  // (first use, or an earlier attempt that got part of the way)
        if (!u.pin) PCPX_HIP(hipHostMalloc(&u.pin, 2 * Uploader::CHUNK, hipHostMallocDefault));
        if (!u.ev[0]) PCPX_HIP(hipEventCreateWithFlags(&u.ev[0], hipEventDisableTiming));
        PCPX_HIP(hipEventCreateWithFlags(&u.ev[1], hipEventDisableTiming));
    }
    const char* from = static_cast<const char*>(src);
    char* to = static_cast<char*>(d_dst);
    hipError_t e = hipSuccess;
    size_t piece = 0;
    for (size_t off = 0; off < bytes && e == hipSuccess; off += Uploader::CHUNK, ++piece) {
        const size_t len = bytes - off < Uploader::CHUNK ? bytes - off : Uploader::CHUNK;
        const int b = static_cast<int>(piece & 1);
        char* stage = static_cast<char*>(u.pin) + static_cast<size_t>(b) * Uploader::CHUNK;
        if (piece >= 2 && (e = hipEventSynchronize(u.ev[b])) != hipSuccess) break;  // the copy that last read this block has finished
        std::memcpy(stage, from + off, len);
        if ((e = hipMemcpyAsync(to + off, stage, len, hipMemcpyHostToDevice, stream)) != hipSuccess) break;
        e = hipEventRecord(u.ev[b], stream);
    }
    // whatever happened, the stream is drained before the ring is anyone else's (copies queued before a failure still read it)
    const hipError_t drained = hipStreamSynchronize(stream);
    return check_hip(e != hipSuccess ? e : drained, "upload", __FILE__, __LINE__);
}

int select_device(int device, int out_of_range)
{
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        set_error("pcpx: no HIP device available (%s); libpcpx has no CPU fallback",
                  e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
        (void)hipGetLastError();
        return PCPX_ERR_DEVICE;
    }
    if (device < 0 || device >= count) {
        set_error("pcpx: device %d out of range [0,%d)", device, count);
        return out_of_range;
    }
    PCPX_HIP(hipSetDevice(device));
    return PCPX_OK;
}

// pcpx_build_params as this library knows it, from what the caller passed: ABI 3 callers pass the first 32 bytes
constexpr size_t BUILD_PARAMS_ABI3 = 32, BUILD_PARAMS_ABI4 = 48;  // (ABI 4 ends before shard_first / shard_count)
int normalise_params(const pcpx_build_params* in, bool device_form, pcpx_build_params& out, const pcpx_build_params*& use)
{
    use = nullptr;
    if (!in) return PCPX_OK;
    static_assert(sizeof(pcpx_build_params) == 64, "pcpx_build_params is part of the ABI");
    if (in->struct_size != sizeof(pcpx_build_params) && in->struct_size != BUILD_PARAMS_ABI3 && in->struct_size != BUILD_PARAMS_ABI4) {
        set_error("pcpx: params->struct_size mismatch");
        return PCPX_ERR_INVALID;
    }
    std::memset(&out, 0, sizeof(out));
    std::memcpy(&out, in, in->struct_size);
    out.struct_size = sizeof(pcpx_build_params);
    if (in->struct_size == BUILD_PARAMS_ABI3) out.flags &= (PCPX_BUILD_USE_GRID | PCPX_BUILD_COARSE_ORDER);
    if (in->struct_size == BUILD_PARAMS_ABI4) out.flags &= ~PCPX_BUILD_SHARD_RANGE;
    if ((out.flags & PCPX_BUILD_SHARD_RANGE) && (!(out.flags & PCPX_BUILD_SHARD) || out.shard_first % GROUP != 0)) {
        set_error("pcpx: PCPX_BUILD_SHARD_RANGE goes with PCPX_BUILD_SHARD, and shard_first must be a multiple of %d", GROUP);
        return PCPX_ERR_INVALID;
    }
    if ((out.flags & PCPX_BUILD_BORROW_CLOUD) && !device_form) {
        set_error("pcpx: PCPX_BUILD_BORROW_CLOUD needs a device-pointer build (the host-pointer forms stage the cloud in a temporary)");
        return PCPX_ERR_INVALID;
    }
    if ((out.flags & PCPX_BUILD_BORROW_CLOUD) && !(out.flags & PCPX_BUILD_SHARD)) {
        set_error("pcpx: PCPX_BUILD_BORROW_CLOUD is a property of rank-local builds (PCPX_BUILD_SHARD)");
        return PCPX_ERR_INVALID;
    }
    use = &out;
    return PCPX_OK;
}

void free_index(Index* ix)
{
    if (!ix) return;
    DeviceScope dscope;
    (void)dscope.use(ix->device);
    (void)hipStreamSynchronize(ix->stream);  // (nullptr = the legacy default stream)
    for (auto& iv : ix->intervals) {
        (void)hipEventDestroy(iv.a);
        (void)hipEventDestroy(iv.b);
    }
    // (the stream is drained: the blocks may serve the next index of this device -- index_block_free)
    index_block_free(ix->d_xyz);
    for (int b = 0; b < 2; ++b) index_block_free(ix->d_codes[b]);
    index_block_free(ix->d_perm);
    index_block_free(ix->d_rec);
    index_block_free(ix->d_sort_tmp);
    index_block_free(ix->d_leaves);
    index_block_free(ix->d_nodes);
    index_block_free(ix->d_scalars);
    index_block_free(ix->d_scratch);
    index_block_free(ix->d_nc4);
    index_block_free(ix->d_pos_of);
    index_block_free(ix->sched.d_gtime);
    index_block_free(ix->sched.d_order);
    (void)hipFree(ix->d_queue);
    (void)hipFree(ix->d_multi);
    free_shard(*ix);
    if (ix->copy_stream) {
        (void)hipStreamSynchronize(ix->copy_stream);
        pooled_stream_put(ix->copy_stream);
    }
    if (ix->own_stream && ix->stream) pooled_stream_put(ix->stream);  // (synchronised above)
    delete ix;  // (the pool and the pinned stage free their memory in their destructors, while the device is still current)
}

}  // namespace pcpx
