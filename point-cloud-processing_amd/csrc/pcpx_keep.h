// pcpx_keep.h -- from a keep mask by input row to the ascending list of kept rows and their number: the tail of Poisson-disk
// subsampling (pcpx_subsample.hip) and of the local maxima (pcpx_keypoints.hip; section 21), beside the
// label tail of pcpx_labels.h, and the copy of that list back to a host caller.  Included by .hip translation units only.
#ifndef PCPX_KEEP_H
#define PCPX_KEEP_H

#include "pcpx_device.h"
#include "pcpx_scan.h"
#include "pcpx_stage.h"

namespace pcpx {
namespace {

constexpr u32 KEEP_BLOCK = 256;

// ---- the kept rows, ascending: the exclusive scan of the keep mask is a kept row's place in the list ---------------------------------
struct IsKept {
    const uint8_t* keep;
    __device__ u32 operator()(u32 i) const { return keep[i] ? 1u : 0u; }
};
__global__ __launch_bounds__(KEEP_BLOCK) void k_keep_compact(const uint8_t* __restrict__ keep, u32 n, const u32* __restrict__ place,
                                                             u32* __restrict__ kept_rows)
{
    const u32 i = blockIdx.x * KEEP_BLOCK + threadIdx.x;
    if (i < n && keep[i]) kept_rows[place[i]] = i;
}

// The tail of a call that leaves a keep mask: the number of kept rows among `rows` into *d_kept_count and the rows themselves,
// ascending, into d_kept_rows (either may be null).  place: `rows` words (used only with d_kept_rows), place[i] = kept rows among
// [0, i); sums: the scan's tile sums.  On stream s, no synchronisation.
inline int count_and_compact_kept(const uint8_t* d_keep, u64 rows, u32* place, u32* sums, u32* d_kept_rows, u64* d_kept_count, hipStream_t s)
{
    if (!d_kept_rows && !d_kept_count) return PCPX_OK;
    int st;
    if (!d_kept_rows) place = nullptr;
    if ((st = exclusive_scan(IsKept{d_keep}, rows, sums, place, d_kept_count, s)) != PCPX_OK) return st;
    if (d_kept_rows) k_keep_compact<<<blocks_of(rows, KEEP_BLOCK), KEEP_BLOCK, 0, s>>>(d_keep, static_cast<u32>(rows), place, d_kept_rows);
    PCPX_HIP(hipGetLastError());
    return PCPX_OK;
}

// The end of a host form: the count first, then that many kept rows (count <= rows), and the wait.  d_count: null when the caller
// asked for neither.
inline int download_kept(Staged& stage, const u64* d_count, const u32* d_kept_rows, u64* opt_kept_count, u32* opt_kept_rows)
{
    u64 count = 0;
    if (d_count) stage.download(&count, d_count, sizeof(u64));
    if (stage.wait() != PCPX_OK) return stage.st;
    if (opt_kept_count) *opt_kept_count = count;
    if (!opt_kept_rows || !count) return PCPX_OK;
    stage.download(opt_kept_rows, d_kept_rows, count * sizeof(u32));
    return stage.wait();
}

}  // namespace
}  // namespace pcpx

#endif
