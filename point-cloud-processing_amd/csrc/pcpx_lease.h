// pcpx_lease.h -- the scratch of the entry points that do not wait for their kernels, and the two prologues around it: the _dev
// forms that take a device number and a stream (pcpx_match.hip, pcpx_register.hip, pcpx_planes.hip; pcpx_icp.hip comes in with a
// handle and its stream) and the host-pointer forms of the same files, which stage their arrays on a stream of the pool and wait.
// Included by .hip translation units only.
#ifndef PCPX_LEASE_H
#define PCPX_LEASE_H

#include "pcpx_stage.h"

#include <vector>

namespace pcpx {

// A block of the device's pool goes back to the pool when the host knows that nothing queued reads it.  A _dev call returns before
// that, so it leaves the block here with an event recorded behind its last kernel; the next such call on the device gives
// back the blocks whose events have passed, and takes over a block that its own stream still holds (the stream orders the two calls).
// Guarded by the device's DeviceShared::mu, which every caller holds.
struct HeldScratch {
    hipStream_t stream;
    void* p;
    size_t bytes;
    hipEvent_t passed;
};
constexpr int LEASE_MAX_DEVICES = 64;
inline std::vector<HeldScratch> g_held[LEASE_MAX_DEVICES];  // (one list per device for the whole library)

struct ScratchLease {
    DevPool& pool;
    std::vector<HeldScratch>& held;
    hipStream_t stream;
    void* p = nullptr;
    size_t bytes = 0;
    ScratchLease(DeviceShared& sh, int device, hipStream_t s) : pool(sh.pool), held(g_held[device]), stream(s) {}
    ScratchLease(const ScratchLease&) = delete;
    ScratchLease& operator=(const ScratchLease&) = delete;
    int take(size_t need)
    {
        bytes = need;
        for (size_t i = 0; i < held.size();) {
            HeldScratch& h = held[i];
            const hipError_t e = hipEventQuery(h.passed);
            const bool mine = !p && h.stream == stream && h.bytes >= need && h.bytes <= 2 * need + (1u << 20);
            if (e != hipSuccess) (void)hipGetLastError();  // (hipErrorNotReady)
            if (e != hipSuccess && !mine) {
                ++i;
                continue;
            }
            if (mine) p = h.p, bytes = h.bytes;
            else pool.release(h.p);
            (void)hipEventDestroy(h.passed);
            held.erase(held.begin() + static_cast<std::ptrdiff_t>(i));
        }
        if (!p) p = pool.acquire(need);
        return p ? PCPX_OK : PCPX_ERR_ALLOC;
    }
    // the call's kernels are queued: the block is given back once the stream has passed this point
    int leave_queued()
    {
        HeldScratch h{stream, p, bytes, nullptr};
        PCPX_HIP(hipEventCreateWithFlags(&h.passed, hipEventDisableTiming));
        const hipError_t e = hipEventRecord(h.passed, stream);
        if (e != hipSuccess) {
            (void)hipEventDestroy(h.passed);
            PCPX_HIP(e);
        }
        held.push_back(h);
        p = nullptr;
        return PCPX_OK;
    }
    ~ScratchLease()  // (a host-form call has synchronised its stream; a failed call waits here)
    {
        if (!p) return;
        (void)hipStreamSynchronize(stream);
        pool.release(p);
    }
};

// A lease of `bytes` on s around a body that only enqueues: body(base) gets the block's address, and the block stays held until
// the stream has passed what the body queued.  The caller holds the device's DeviceShared::mu.
template <class Body>
int leased(DeviceShared& sh, int device, hipStream_t s, size_t bytes, Body&& body)
{
    ScratchLease lease(sh, device, s);
    int st;
    if ((st = lease.take(bytes)) != PCPX_OK) return st;
    if ((st = body(static_cast<char*>(lease.p))) != PCPX_OK) return st;
    return lease.leave_queued();
}

// The prologue of a _dev entry point that takes a device number and the caller's stream (after its argument checks): the device
// made current and locked, `bytes` of scratch leased, body(base, stream).
template <class Body>
int on_leased(int device, const char* what, void* stream, size_t bytes, Body&& body)
{
    if (device < 0 || device >= LEASE_MAX_DEVICES) return select_device(device);
    return on_shared(device, what, [&](DeviceShared& sh) -> int {
        const hipStream_t s = static_cast<hipStream_t>(stream);
        return leased(sh, device, s, bytes, [&](char* base) -> int { return body(base, s); });
    });
}

// A host-pointer call on the device: the staging (pcpx_stage.h) on a stream of the pool, and the scratch.  Destruction order, which
// the order of the bases and the member fixes: the lease goes first (a failed call that holds a block waits for the stream there),
// then the staging (it waits if the call did not reach a successful wait(), and its blocks go back to the pool), and the pooled
// stream goes back last, when nothing queued on it is left.
struct HostCallStream {
    PooledStream ps;
};
struct HostCall : HostCallStream, Staged {
    ScratchLease lease;
    HostCall(DeviceShared& sh, int device) : Staged(sh.pool, nullptr), lease(sh, device, nullptr) {}
    int begin()
    {
        PCPX_HIP(pooled_stream_get(&ps.s));
        s = lease.stream = ps.s;
        return PCPX_OK;
    }
    char* scratch(size_t bytes)
    {
        if (st == PCPX_OK) st = lease.take(bytes);
        return static_cast<char*>(lease.p);
    }
};

// The prologue of a host-pointer entry point that takes a device number (after its argument checks): body(call).
template <class Body>
int on_host_call(int device, const char* what, Body&& body)
{
    if (device < 0 || device >= LEASE_MAX_DEVICES) return select_device(device);
    return on_shared(device, what, [&](DeviceShared& sh) -> int {
        HostCall call(sh, device);
        const int st = call.begin();
        return st != PCPX_OK ? st : body(call);
    });
}

}  // namespace pcpx

#endif
