// pcpx_ransac.h -- what the hypothesis-and-score entry points share (pcpx_register.hip: rigid poses, DESIGN.md section 24;
// pcpx_planes.hip: planes, section 26): the plan that cuts the records into segments, the count word of an invalid hypothesis, the
// best-key reduction over the counts, the compaction of flagged records, the scratch of their least-squares fits (whose float64 sums
// are pcpx_fixed_sum.h's) and the copy-out of a host-form call.  Included by .hip translation units only.
#ifndef PCPX_RANSAC_H
#define PCPX_RANSAC_H

#include "pcpx_device.h"
#include "pcpx_fixed_sum.h"
#include "pcpx_lease.h"

#include <algorithm>

namespace pcpx {
namespace {

constexpr u32 RG_BLOCK = 256;  // threads of the row-wise kernels
constexpr u32 RG_BEST_PER_THREAD = 16;  // hypotheses of a k_ransac_best thread
constexpr u32 RG_INVALID = 0xFFFFFFFFu;  // the count word of an invalid hypothesis (a count is at most C < 2^32 - 1)
constexpr u32 FIT_TERMS = 16;  // the doubles a block's partial sums of a fit are apart (pcpx_fixed_sum.h)
// the scratch of a fit whose state is `state` doubles: the blocks' partial sums, then the state
constexpr size_t fit_bytes(u32 state) { return (static_cast<size_t>(FIT_BLOCKS) * FIT_TERMS + state) * sizeof(double); }


// The plan: a wave is 64 hypotheses on one segment of the records, a call should be several rounds of what the device holds
// (PLAN_TARGET_WAVES), a segment is never shorter than PLAN_MIN_SEGMENT_ROWS (a wave's prologue -- three gathers and what it makes
// of them -- is paid per segment) and there are never more than PLAN_MAX_SEGMENTS (the best-key reduction reads a word per
// hypothesis and segment).
constexpr u64 PLAN_TARGET_WAVES = 16384;
constexpr u64 PLAN_MAX_SEGMENTS = 256;
constexpr u64 PLAN_MIN_SEGMENT_ROWS = 256;
constexpr u64 PLAN_LAUNCH_HYPOTHESES = 1ull << 30;  // hypotheses of one launch (a grid's thread count stays below 2^32)
struct SegmentPlan {
    u32 segments = 0;
    u64 rows = 0;  // per segment
};
inline SegmentPlan segment_plan(u64 hypotheses, u64 capacity)
{
    SegmentPlan p;
    if (!capacity) return p;
    const u64 groups = std::max<u64>(1, (hypotheses + GROUP - 1) / GROUP);
    const u64 want = (PLAN_TARGET_WAVES + groups - 1) / groups;
    const u64 s0 = std::max<u64>(1, std::min({want, PLAN_MAX_SEGMENTS, capacity / PLAN_MIN_SEGMENT_ROWS}));
    p.rows = ((capacity + s0 - 1) / s0 + PLAN_MIN_SEGMENT_ROWS - 1) / PLAN_MIN_SEGMENT_ROWS * PLAN_MIN_SEGMENT_ROWS;
    p.segments = static_cast<u32>((capacity + p.rows - 1) / p.rows);
    return p;
}

// RG_BEST_PER_THREAD hypotheses per thread, a block's threads side by side in each round: the sum of a hypothesis's segment counts
// (integers: exact, and independent of the split), the key ((count + 1) << 32 | (0xFFFFFFFF - h)) of a valid one -- larger count
// first, then lower h -- and 0 of an invalid one; the largest key of the wave goes to *key by one atomicMax, and only where it is
// above what *key already holds (62 500 atomics on the one word were a quarter of a call of 4 000 000 hypotheses: DESIGN.md
// section 24).  The maximum does not depend on the order; a stale read of *key only costs an atomic.
__global__ __launch_bounds__(RG_BLOCK) void k_ransac_best(const u32* __restrict__ counts, u64 h_base, u64 h_end, u64 T, u32 segments, u64* __restrict__ key)
{
    u64 k = 0;
#pragma unroll 4
    for (u32 j = 0; j < RG_BEST_PER_THREAD; ++j) {
        const u64 h = h_base + (static_cast<u64>(blockIdx.x) * RG_BEST_PER_THREAD + j) * RG_BLOCK + threadIdx.x;
        if (h >= h_end) break;
        u32 sum = counts[h];
        if (sum == RG_INVALID) continue;
        for (u32 s = 1; s < segments; ++s) sum += counts[static_cast<u64>(s) * T + h];
        const u64 mine = (static_cast<u64>(sum + 1u) << 32) | (0xFFFFFFFFu - static_cast<u32>(h));
        k = mine > k ? mine : k;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const u64 other = __shfl_xor(k, off);
        k = other > k ? other : k;
    }
    if ((threadIdx.x & 63u) == 0 && k > __hip_atomic_load(key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMax(reinterpret_cast<unsigned long long*>(key), static_cast<unsigned long long>(k));
}

// done: null, or the word of a loop on the device: 0, or 1 + the round that stopped it; the kernels of a later round return at once
__device__ __forceinline__ bool gone(const u32* done, u32 round)
{
    if (!done) return false;
    const u32 d = *done;
    return d != 0u && d <= round;
}

constexpr u32 PL_FOLD = 16;  // lanes of k_plane_fold that share a hypothesis
// FOLD lanes per hypothesis: counts[h] (segment 0's row) becomes the sum over all segments, so that k_ransac_best reads one word
// per hypothesis.  (Its own loop over the segments is one thread's chain of loads: with 245 segments and 1 024 hypotheses -- a
// single block -- it took 0.23 ms a round, a third of an extraction)  Integer sums: exact in any order.  An
// invalid hypothesis keeps RG_INVALID.  The group's lanes all read counts[h] before lane 0 of the group writes it.  (A template
// so that a file that does not fold has no copy of it: pcpx_planes.hip and pcpx_shapes.hip do.)
template <u32 FOLD>
__global__ __launch_bounds__(RG_BLOCK) void k_plane_fold(u32* counts, const u32* __restrict__ done, u32 round, u64 h_base, u64 h_end, u64 T, u32 segments)
{
    if (gone(done, round)) return;
    const u64 h = h_base + (static_cast<u64>(blockIdx.x) * RG_BLOCK + threadIdx.x) / FOLD;
    const u32 part = threadIdx.x % FOLD;
    const bool in = h < h_end;
    const u32 first = in ? counts[h] : RG_INVALID;
    u32 sum = 0;
    if (first != RG_INVALID) {
        for (u32 s = part ? part : FOLD; s < segments; s += FOLD) sum += counts[static_cast<u64>(s) * T + h];
    }
#pragma unroll
    for (u32 off = FOLD / 2; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    if (part == 0 && first != RG_INVALID) counts[h] = first + sum;
}

struct IsFlagged {
    const uint8_t* flag;
    __device__ u32 operator()(u32 i) const { return flag[i]; }
};

__global__ __launch_bounds__(RG_BLOCK) void k_reg_compact(u32 capacity, const uint8_t* __restrict__ flag, const u32* __restrict__ place,
                                                         u32* __restrict__ positions)
{
    const u32 k = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (k < capacity && flag[k]) positions[place[k]] = k;
}

// The small outputs of a host-form RANSAC call as one block on the device (the model is the transform's 16 doubles or the plane's 4),
// and their way back: the block after one wait, then the `score` inlier positions after a second one, only where there are some.
template <int DOUBLES>
struct RansacSmall {
    u32 found, h, score, pad;
    double model[DOUBLES], refit[DOUBLES];
};
template <int DOUBLES>
int ransac_copy_out(HostCall& call, const RansacSmall<DOUBLES>* d, const u32* d_inliers, u32* out_found, u32* opt_out_hypothesis, u32* opt_out_score,
                    u32* opt_out_inliers, double* opt_out_model, double* opt_out_refit)
{
    RansacSmall<DOUBLES> host;
    int st;
    if ((st = call.download(&host, d, sizeof(host))) != PCPX_OK || (st = call.wait()) != PCPX_OK) return st;
    if (opt_out_inliers && host.score) {
        if ((st = call.download(opt_out_inliers, d_inliers, static_cast<size_t>(host.score) * sizeof(u32))) != PCPX_OK || (st = call.wait()) != PCPX_OK) return st;
    }
    *out_found = host.found;
    if (opt_out_hypothesis) *opt_out_hypothesis = host.h;
    if (opt_out_score) *opt_out_score = host.score;
    if (opt_out_model) std::copy(host.model, host.model + DOUBLES, opt_out_model);
    if (opt_out_refit) std::copy(host.refit, host.refit + DOUBLES, opt_out_refit);
    return PCPX_OK;
}

}  // namespace
}  // namespace pcpx

#endif
