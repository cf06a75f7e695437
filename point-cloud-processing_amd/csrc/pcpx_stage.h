// pcpx_stage.h -- what the host-pointer entry points of both families share: where the arrays lie in a call's scratch (Carve), the
// caller's arrays staged in blocks of a pool on one stream (Staged), and the prologue of the handle family's host forms
// (on_index_host).  The device-number family builds on it in pcpx_lease.h.
#ifndef PCPX_STAGE_H
#define PCPX_STAGE_H

#include "pcpx_internal.h"

#include <deque>

namespace pcpx {

inline u32 blocks_of(u64 n, u32 per) { return static_cast<u32>((n + per - 1) / per); }

// Where everything lies in the scratch of a call: byte offsets from its start, each a multiple of 256.
inline size_t padded(u64 bytes) { return (bytes + 255) / 256 * 256; }
struct Carve {
    size_t at = 0;
    size_t take(u64 bytes)
    {
        const size_t here = at;
        at += padded(bytes);
        return here;
    }
    size_t bytes() const { return at; }
};

// The staging of a host-pointer call: the caller's arrays in blocks of `pool`, blocks for the outputs, the copies back and the wait,
// all on stream s.  A failed step makes the later ones do nothing and stays in `st`.  Destruction order: the destructor's body runs
// before the members go, so a call that handed out blocks and did not reach a successful wait() (a step failed, or the caller left
// with a worker's error) waits for the stream before its blocks go back to the pool and before the caller may free its arrays.
struct Staged {
    DevPool& pool;
    hipStream_t s;
    std::deque<DevBuf> blocks;
    int st = PCPX_OK;
    bool waited = true;  // (nothing is queued yet)
    Staged(DevPool& pool_, hipStream_t s_) : pool(pool_), s(s_) {}
    ~Staged() { if (!waited) (void)hipStreamSynchronize(s); }
    // `bytes` of device memory; null for none
    void* alloc(size_t bytes)
    {
        if (st != PCPX_OK || !bytes) return nullptr;
        blocks.emplace_back(pool);
        st = blocks.back().alloc(bytes);
        waited = false;  // (what the caller queues on s may use the block)
        return blocks.back().p;
    }
    template <class T>
    T* alloc(size_t bytes) { return static_cast<T*>(alloc(bytes)); }
    // the block of an optional output: null when the caller did not ask for it
    template <class T>
    T* alloc_for(const T* host, size_t bytes) { return host ? alloc<T>(bytes) : nullptr; }
    // this host array of this many bytes on the device, or null when there is none.  plain: by one copy that the runtime stages
    // itself and not through upload_pageable's pinned ring (the score array of pcpx_local_maxima_self, where the ring lost 0.1 ms
    // of a 0.5 ms call at 4 MB: profiles/r22_host_staging.json); the source may be reused when either returns
    template <class T>
    const T* upload(const T* host, size_t bytes, bool plain = false)
    {
        void* d = host ? alloc(bytes) : nullptr;
        if (d && st == PCPX_OK)
            st = plain ? check_hip(hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, s), "upload", __FILE__, __LINE__)
                       : upload_pageable(d, host, bytes, s);
        return static_cast<const T*>(d);
    }
    int download(void* host, const void* d, size_t bytes)
    {
        if (st != PCPX_OK) return st;
        waited = false;
        return st = check_hip(hipMemcpyAsync(host, d, bytes, hipMemcpyDeviceToHost, s), "download", __FILE__, __LINE__);
    }
    // ... of an optional output: nothing for a null host pointer
    int download_opt(void* host, const void* d, size_t bytes) { return host ? download(host, d, bytes) : st; }
    int wait()
    {
        if (st != PCPX_OK) return st;
        waited = true;  // (a stream that cannot be waited on is not waited on again)
        return st = check_hip(hipStreamSynchronize(s), "wait", __FILE__, __LINE__);
    }
};

// The prologue of a host-pointer entry point that takes a pcpx_index*: on_index, and the staging on the handle's pool and stream;
// body(ix, stage).  The scratch stays the handle's (ensure_scratch).
template <class Body>
int on_index_host(pcpx_index* h, const char* what, int flags, Body&& body)
{
    return on_index(h, what, flags, [&](Index* ix) -> int {
        Staged stage(ix->pool, ix->stream);
        return body(ix, stage);
    });
}

}  // namespace pcpx

#endif
