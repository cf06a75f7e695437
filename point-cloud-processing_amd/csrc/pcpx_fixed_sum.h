// pcpx_fixed_sum.h -- the float64 sums of the least-squares steps (the rigid fit of pcpx_register.hip, the plane fit of
// pcpx_planes.hip, the point-to-plane system of pcpx_icp.hip) in ONE fixed order, so that every bit of a result depends on the items
// alone, not on the capacities of the call:
//   a thread adds its items in ascending order, a stride of the grid (FIT_BLOCKS x FIT_THREADS) apart;
//   the block's FIT_THREADS threads are added by a fixed tree (offsets 128 ... 1);
//   thread `term` of one last block adds the FIT_BLOCKS partial sums of its term in block order.
// The order is the contract (tests/test_gpu_fit_bits.py pins it to a recording); it is written down here and nowhere else.
// A user supplies a "sum" type, passed to both kernels by value:
//   TERMS, STRIDE    the number of sums (at most 64) and the doubles a block's partial sums are apart
//   live()           false: the launch writes nothing, neither partial sums nor state (block-uniform)
//   items()          the number of items; called once per thread, before any add (it may read the launch's count words into the copy)
//   add(j, acc)      adds item j's products to acc[TERMS], or nothing for an item that is not usable
//   finish(t, total) thread t of the last block has term t's total: where it goes
// Included by .hip translation units only.
#ifndef PCPX_FIXED_SUM_H
#define PCPX_FIXED_SUM_H

#include "pcpx_device.h"

namespace pcpx {
namespace {

constexpr u32 FIT_BLOCKS = 64;
constexpr u32 FIT_THREADS = 256;

// the number of items behind a count word on the device: null means the capacity, a larger count is cut to it
__device__ __forceinline__ u32 clamped_count(const u64* d_count, u32 capacity)
{
    if (!d_count) return capacity;
    const u64 c = *d_count;
    return c < capacity ? static_cast<u32>(c) : capacity;
}

template <class Sum>
__global__ __launch_bounds__(FIT_THREADS) void k_fixed_partial(Sum sum, double* __restrict__ partial)
{
    constexpr int NT = Sum::TERMS;
    __shared__ double tree[FIT_THREADS];
    if (!sum.live()) return;
    const u32 n = sum.items();
    double acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[i] = 0.0;
    for (u64 j = static_cast<u64>(blockIdx.x) * FIT_THREADS + threadIdx.x; j < n; j += static_cast<u64>(gridDim.x) * FIT_THREADS)
        sum.add(static_cast<u32>(j), acc);
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        tree[threadIdx.x] = acc[i];
        __syncthreads();
        for (u32 off = FIT_THREADS / 2; off > 0; off >>= 1) {
            if (threadIdx.x < off) tree[threadIdx.x] += tree[threadIdx.x + off];
            __syncthreads();
        }
        if (threadIdx.x == 0) partial[blockIdx.x * Sum::STRIDE + i] = tree[0];
        __syncthreads();
    }
}

template <class Sum>
__global__ __launch_bounds__(64) void k_fixed_final(Sum sum, const double* __restrict__ partial)
{
    static_assert(Sum::TERMS <= 64 && Sum::TERMS <= Sum::STRIDE, "a thread of one wave per term");
    if (!sum.live() || threadIdx.x >= Sum::TERMS) return;
    double total = 0.0;
#pragma unroll 16
    for (u32 b = 0; b < FIT_BLOCKS; ++b) total += partial[b * Sum::STRIDE + threadIdx.x];  // (in block order; the loads of a batch are issued together)
    sum.finish(threadIdx.x, total);
}

// both kernels on s, with the fixed grid.  partial: FIT_BLOCKS x Sum::STRIDE doubles.
template <class Sum>
inline void fixed_sum(const Sum& sum, double* partial, hipStream_t s)
{
    k_fixed_partial<Sum><<<FIT_BLOCKS, FIT_THREADS, 0, s>>>(sum, partial);
    k_fixed_final<Sum><<<1, 64, 0, s>>>(sum, partial);
}

}  // namespace
}  // namespace pcpx

#endif
