// pcpx_lease.h -- the scratch of the entry points that take a device number and do not wait for their kernels (pcpx_match.hip,
// pcpx_register.hip).  Included by .hip translation units only.
#ifndef PCPX_LEASE_H
#define PCPX_LEASE_H

#include "pcpx_internal.h"

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

}  // namespace pcpx

#endif
