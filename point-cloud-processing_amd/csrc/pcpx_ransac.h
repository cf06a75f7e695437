// pcpx_ransac.h -- what the hypothesis-and-score entry points share (pcpx_register.hip: rigid poses, DESIGN.md section 24;
// pcpx_planes.hip: planes, section 26): the count word of an invalid hypothesis, the best-key reduction over the counts, the
// compaction of flagged records, and the fixed order of the float64 sums of their least-squares fits.  Included by .hip translation
// units only.
#ifndef PCPX_RANSAC_H
#define PCPX_RANSAC_H

#include "pcpx_device.h"

namespace pcpx {
namespace {

constexpr u32 RG_BLOCK = 256;  // threads of the row-wise kernels
constexpr u32 RG_BEST_PER_THREAD = 16;  // hypotheses of a k_ransac_best thread
constexpr u32 RG_INVALID = 0xFFFFFFFFu;  // the count word of an invalid hypothesis (a count is at most C < 2^32 - 1)
// the fit: FIT_BLOCKS blocks of RG_BLOCK threads stride over the pairs; a block leaves FIT_TERMS doubles
constexpr u32 FIT_BLOCKS = 64;
constexpr u32 FIT_TERMS = 16;

inline u32 blocks_of(u64 n, u32 per) { return static_cast<u32>((n + per - 1) / per); }
inline size_t padded(u64 bytes) { return (bytes + 255) / 256 * 256; }

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

// The order of a fit's float64 sums.  A thread has added its items in ascending order (a stride of the grid apart) into acc; the
// block's threads are added by a fixed tree, and the block leaves its sums in partial[block * FIT_TERMS + term].  Every thread of
// the block calls this.
template <int NT>
__device__ __forceinline__ void fit_block_sums(const double (&acc)[NT], double* __restrict__ partial)
{
    __shared__ double tree[RG_BLOCK];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        tree[threadIdx.x] = acc[i];
        __syncthreads();
        for (u32 off = RG_BLOCK / 2; off > 0; off >>= 1) {
            if (threadIdx.x < off) tree[threadIdx.x] += tree[threadIdx.x + off];
            __syncthreads();
        }
        if (threadIdx.x == 0) partial[blockIdx.x * FIT_TERMS + i] = tree[0];
        __syncthreads();
    }
}
// ... and the blocks' partial sums of one term in block order
__device__ __forceinline__ double fit_sum_blocks(const double* __restrict__ partial, u32 nblocks, u32 term)
{
    double sum = 0.0;
#pragma unroll 16
    for (u32 b = 0; b < nblocks; ++b) sum += partial[b * FIT_TERMS + term];  // (in block order; the loads of a batch are issued together)
    return sum;
}

}  // namespace
}  // namespace pcpx

#endif
