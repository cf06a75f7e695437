// pcpx_scan.h -- the device-wide exclusive scan, three launches: the sum of each tile of 1024 rows, the scan of those sums by one
// block, the tiles.  What row i contributes is a functor over i (f(i), for i < n only); sums inside a tile are formed in f's result
// type, sums across tiles and the output in Out (32-bit counts into 64-bit offsets: pcpx_range.hip).  The in-place scan of an
// array is the same scan with the array as contribution and as output: a thread of the third launch has read its four rows
// before it writes them, and no other thread touches them.
#ifndef PCPX_SCAN_H
#define PCPX_SCAN_H

#include "pcpx_internal.h"

namespace pcpx {
namespace {

constexpr u32 SCAN_TILE = 1024, SCAN_BLOCK = 256, SCAN_ITEMS = SCAN_TILE / SCAN_BLOCK;
inline u32 scan_tiles(u64 n) { return static_cast<u32>((n + SCAN_TILE - 1) / SCAN_TILE); }  // the length of a scan's tile_sum scratch

// inclusive scan over the lanes of a wave
template <class T>
__device__ __forceinline__ T wave_inclusive_scan(T v, u32 lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T up = __shfl_up(v, off);
        if (lane >= static_cast<u32>(off)) v += up;
    }
    return v;
}

template <class Out, class F>
__global__ __launch_bounds__(SCAN_BLOCK) void k_scan_tile_sums(F f, u32 n, Out* __restrict__ tile_sum)
{
    __shared__ Out w[SCAN_BLOCK / 64];
    const u32 base = blockIdx.x * SCAN_TILE;
    Out v = 0;
#pragma unroll
    for (u32 j = 0; j < SCAN_ITEMS; ++j) {
        const u32 i = base + j * SCAN_BLOCK + threadIdx.x;
        if (i < n) v += f(i);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63u) == 0) w[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = w[0] + w[1] + w[2] + w[3];
}
// one block: tile sums -> their exclusive scan in place, and the total
template <class Out>
__global__ __launch_bounds__(1024) void k_scan_sums(Out* __restrict__ tile_sum, u32 ntiles, u64* __restrict__ total_out)
{
    __shared__ Out wsum[16];
    __shared__ Out carry_s;
    const u32 t = threadIdx.x, lane = t & 63u, w = t >> 6;
    if (t == 0) carry_s = 0;
    __syncthreads();
    for (u32 base = 0; base < ntiles; base += 1024) {
        const u32 i = base + t;
        const Out v = i < ntiles ? tile_sum[i] : Out(0);
        const Out incl = wave_inclusive_scan(v, lane);
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        Out before = carry_s, total = 0;
        for (u32 j = 0; j < 16; ++j) {
            before += j < w ? wsum[j] : Out(0);
            total += wsum[j];
        }
        if (i < ntiles) tile_sum[i] = before + incl - v;
        __syncthreads();
        if (t == 0) carry_s += total;
        __syncthreads();
    }
    if (t == 0 && total_out) *total_out = carry_s;
}
// out[i] = the contributions of rows [0, i)
template <class Out, class F>
__global__ __launch_bounds__(SCAN_BLOCK) void k_scan_tiles(F f, u32 n, const Out* __restrict__ tile_base, Out* out)
{
    using In = decltype(f(0u));
    __shared__ In w[SCAN_BLOCK / 64];
    const u32 base = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
    In c[SCAN_ITEMS], s = 0;
#pragma unroll
    for (u32 j = 0; j < SCAN_ITEMS; ++j) {
        c[j] = base + j < n ? f(base + j) : In(0);
        s += c[j];
    }
    const In incl = wave_inclusive_scan(s, threadIdx.x & 63u);
    if ((threadIdx.x & 63u) == 63u) w[threadIdx.x >> 6] = incl;
    __syncthreads();
    In before = 0;
    for (u32 j = 0; j < (threadIdx.x >> 6); ++j) before += w[j];
    Out at = tile_base[blockIdx.x] + before + incl - s;
#pragma unroll
    for (u32 j = 0; j < SCAN_ITEMS; ++j) {
        if (base + j < n) out[base + j] = at;
        at += c[j];
    }
}

// out[i] = f(0) + ... + f(i - 1) for i < n (out null: only the total is wanted); *total_out = the sum over all n rows (device
// memory, may be null).  tile_sum: scratch of scan_tiles(n) entries.  On stream s, no synchronisation.
template <class Out, class F>
int exclusive_scan(F f, u64 n, Out* tile_sum, Out* out, u64* total_out, hipStream_t s)
{
    if (n == 0) return PCPX_OK;
    if (n > 0xFFFFFFFFull) {
        set_error("pcpx: scan of %llu entries is too long", static_cast<unsigned long long>(n));
        return PCPX_ERR_INVALID;
    }
    const u32 n32 = static_cast<u32>(n), ntiles = scan_tiles(n);
    k_scan_tile_sums<Out, F><<<ntiles, SCAN_BLOCK, 0, s>>>(f, n32, tile_sum);
    k_scan_sums<Out><<<1, 1024, 0, s>>>(tile_sum, ntiles, total_out);
    if (out) k_scan_tiles<Out, F><<<ntiles, SCAN_BLOCK, 0, s>>>(f, n32, tile_sum, out);
    PCPX_HIP(hipGetLastError());
    return PCPX_OK;
}

template <class T>
struct ArrayRows {
    const T* a;
    __device__ T operator()(u32 i) const { return a[i]; }
};
// a[i] = a[0] + ... + a[i - 1], in place (a caller whose last entry is 0 finds the total there)
template <class T>
int exclusive_scan_in_place(T* a, u64 n, T* tile_sum, hipStream_t s)
{
    return exclusive_scan<T>(ArrayRows<T>{a}, n, tile_sum, a, nullptr, s);
}

}  // namespace
}  // namespace pcpx

#endif
