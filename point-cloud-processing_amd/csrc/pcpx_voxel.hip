// pcpx_voxel.hip -- voxel-grid downsampling (include/pcpx_voxel.h): the rows keyed by their cell, ordered by
// (key, row) with two stable sorts, cut into voxels at the key changes, and every column summed per voxel in the contract's fixed
// two-level order.  No LDS outside the scan (pcpx_scan.h) and the sort (pcpx_sort.hip), no floating-point atomics, and nothing is
// handed between workgroups inside a launch: the integer atomics below (agent scope, relaxed) are read by later launches only.
//   k_voxel_begin     the words of the call's state
//   k_voxel_bounds    without an explicit origin: the per-axis minimum of the usable rows as ordered integers, one atomic per wave
//   k_voxel_keys      one thread per row: word 1 = key[31:0] << 32 | row, key[62:32] beside it; the dropped rows counted per wave
//   sort_keys_u64     word 1 on its upper half (stable: ascending (key[31:0], row))
//   k_voxel_second    word 2 = key[62:32] << 32 | position in that order
//   sort_keys_u64     word 2 on its upper half (stable: ascending (key, row)) -- a 63-bit key and a 32-bit row are not one word
//   k_voxel_gather    position -> (key, row)
//   pcpx_scan.h       over the head flags (the key differs from its predecessor's): a position's voxel, and V
//   k_voxel_starts    where every voxel starts, and the owner of every indexed row
//   k_voxel_heads     keys and counts
//   k_voxel_chunks    one lane per chunk of 64 members, four columns at a time: a voxel of one chunk is finished here
//   k_voxel_combine   one lane per longer voxel: its chunk sums in order, the division
//   k_voxel_nearest / k_voxel_rows    the member nearest the centroid: a 64-bit integer minimum (order-independent)
#include "pcpx_device.h"
#include "pcpx_lease.h"
#include "pcpx_scan.h"
#include "pcpx_voxel.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace pcpx {

namespace {

constexpr u32 VX_BLOCK = 256;
constexpr u32 VX_CHUNK = 64;  // members of a chunk (the contract's)
constexpr u32 VX_COLS = 4;    // columns of one k_voxel_chunks launch
constexpr u64 VX_N_LIMIT = (1ull << 32) - SORT_TILE_WORDS;
constexpr u64 VX_NO_KEY = ~0ull;       // the key of a row that is not indexed: it sorts last
constexpr u32 VX_NO_HIGH = 0xFFFFFFFFu;  // ... and its upper half (an indexed row's is below 2^31)
constexpr float VX_CELLS = 2097152.f;  // 2^21

// The words of a call on the device.  lo: the ordered integers of the coordinate minima (all ones: no usable row).
struct State {
    u32 lo[3], pad;
    u64 dropped;
};

// The chunk sums of the voxels of more than one chunk live in slots by position.  Such a voxel spans more than 64 positions, so a
// window of 64 aligned positions meets at most two of them, the later of which starts inside the window: a chunk that starts at
// position i of a voxel that starts at s has slot 2 (i / 64) + (s / 64 == i / 64), and no two chunks share one.
__host__ __device__ inline u64 chunk_slots(u64 n) { return 2 * ((n + VX_CHUNK - 1) / VX_CHUNK); }
__device__ __forceinline__ u32 chunk_slot(u32 i, u32 s) { return 2u * (i / VX_CHUNK) + ((s / VX_CHUNK == i / VX_CHUNK) ? 1u : 0u); }

struct Layout {
    size_t state = 0, word[3] = {0, 0, 0}, high = 0, row = 0, rank = 0, sums = 0, start = 0, chunk = 0, near = 0, centroid = 0, sort = 0, sort_bytes = 0,
           bytes = 0;
    u64 cap = 0;  // the voxels the per-voxel arrays have room for
    Layout(u64 n, u64 capacity) : cap(std::min(capacity, n))
    {
        Carve c;
        state = c.take(sizeof(State));
        for (size_t& w : word) w = c.take(n * sizeof(u64));
        high = c.take(n * sizeof(u32));
        row = c.take(n * sizeof(u32));
        rank = c.take(n * sizeof(u32));
        sums = c.take(static_cast<u64>(scan_tiles(n)) * sizeof(u32));
        start = c.take((n + 1) * sizeof(u32));
        chunk = c.take(chunk_slots(n) * VX_COLS * sizeof(double));
        near = c.take(cap * sizeof(u64));
        centroid = c.take(cap * 3 * sizeof(float));
        sort_keys_u64(nullptr, sort_bytes, nullptr, nullptr, n, nullptr, 32);
        sort = c.take(sort_bytes);
        bytes = c.bytes();
    }
};

// unsigned integers in the order of the floats they are the bits of (-0 below +0)
__device__ __forceinline__ u32 ordered_of(float f)
{
    const u32 b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float float_of_ordered(u32 o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o); }

struct Grid {
    float leaf[3], origin[3];
    u32 fixed;  // the origin is `origin`, not the state's minima
    __device__ __forceinline__ void origin_of(const State* st, float (&o)[3]) const
    {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const u32 lo = st->lo[a];
            o[a] = fixed ? origin[a] : (lo == 0xFFFFFFFFu ? 0.f : float_of_ordered(lo));
        }
    }
};

__device__ __forceinline__ bool load_usable(const float* __restrict__ points, u32 row, float (&p)[3])
{
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        p[a] = points[static_cast<u64>(row) * 3 + a];
        ok = ok && std::isfinite(p[a]);
    }
    return ok;
}

__global__ __launch_bounds__(64) void k_voxel_begin(State* __restrict__ st)
{
    if (threadIdx.x != 0) return;
    st->lo[0] = st->lo[1] = st->lo[2] = 0xFFFFFFFFu;
    st->pad = 0u;
    st->dropped = 0ull;
}

// A fixed grid striding over the rows: a thread's minimum, the wave's, one atomic per axis per wave -- 3 x 4 VX_BOUNDS_BLOCKS of them on
// three words.  (One atomic per axis per 64 rows, 470 000 of them at 10 M rows, took 5.3 ms: DESIGN.md section 27.)
// (above: 3 axes x 4 waves x VX_BOUNDS_BLOCKS atomics)
constexpr u32 VX_BOUNDS_BLOCKS = 1024;
__global__ __launch_bounds__(VX_BLOCK) void k_voxel_bounds(const float* __restrict__ points, u32 n, State* __restrict__ st)
{
    u32 lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    for (u64 i = blockIdx.x * VX_BLOCK + threadIdx.x; i < n; i += static_cast<u64>(gridDim.x) * VX_BLOCK) {
        float p[3];
        if (!load_usable(points, static_cast<u32>(i), p)) continue;
#pragma unroll
        for (int a = 0; a < 3; ++a) lo[a] = min(lo[a], ordered_of(p[a]));
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        u32 v = lo[a];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v = min(v, static_cast<u32>(__shfl_xor(v, off)));
        if ((threadIdx.x & 63u) == 0 && v != 0xFFFFFFFFu) __hip_atomic_fetch_min(&st->lo[a], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(VX_BLOCK) void k_voxel_keys(const float* __restrict__ points, u32 n, Grid g, State* st, u64* __restrict__ word1,
                                                        u32* __restrict__ high, u32* __restrict__ out_owner, float* __restrict__ out_origin)
{
    const u32 i = blockIdx.x * VX_BLOCK + threadIdx.x;
    float o[3];
    g.origin_of(st, o);
    if (i < 3 && out_origin) out_origin[i] = i == 0 ? o[0] : i == 1 ? o[1] : o[2];
    float p[3] = {0.f, 0.f, 0.f};
    bool in = i < n && load_usable(points, i < n ? i : 0u, p);
    u64 c[3] = {0, 0, 0};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float t = p[a] - o[a];
        const float q = t / g.leaf[a];
        in = in && q >= 0.f && q < VX_CELLS;  // (false for a NaN)
        c[a] = in ? static_cast<u64>(floorf(q)) : 0ull;
    }
    const u64 key = in ? (c[2] << 42) | (c[1] << 21) | c[0] : VX_NO_KEY;
    const u64 gone = __builtin_amdgcn_ballot_w64(i < n && !in);
    if ((threadIdx.x & 63u) == 0 && gone != 0ull)
        __hip_atomic_fetch_add(&st->dropped, static_cast<u64>(__builtin_popcountll(gone)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (i >= n) return;
    word1[i] = (key << 32) | i;
    high[i] = in ? static_cast<u32>(key >> 32) : VX_NO_HIGH;
    if (!in && out_owner) out_owner[i] = PCPX_VOXEL_NONE;
}

__global__ __launch_bounds__(VX_BLOCK) void k_voxel_second(const u64* __restrict__ sorted1, const u32* __restrict__ high, u32 n, u64* __restrict__ word2)
{
    const u32 i = blockIdx.x * VX_BLOCK + threadIdx.x;
    if (i >= n) return;
    const u32 row = static_cast<u32>(sorted1[i]);
    word2[i] = (static_cast<u64>(high[row < n ? row : 0u]) << 32) | i;
}

__global__ __launch_bounds__(VX_BLOCK) void k_voxel_gather(const u64* __restrict__ sorted1, const u64* __restrict__ sorted2, u32 n, u64* __restrict__ skey,
                                                          u32* __restrict__ srow)
{
    const u32 i = blockIdx.x * VX_BLOCK + threadIdx.x;
    if (i >= n) return;
    const u64 w2 = sorted2[i];
    const u32 at = static_cast<u32>(w2), hi = static_cast<u32>(w2 >> 32);
    const u64 w1 = sorted1[at < n ? at : 0u];
    skey[i] = hi == VX_NO_HIGH ? VX_NO_KEY : (static_cast<u64>(hi) << 32) | (w1 >> 32);
    srow[i] = static_cast<u32>(w1);
}

// 1 where a voxel starts in the (key, row) order
struct IsHead {
    const u64* skey;
    __device__ u32 operator()(u32 i) const
    {
        const u64 k = skey[i];
        return (k != VX_NO_KEY && (i == 0 || skey[i - 1] != k)) ? 1u : 0u;
    }
};

// rank[i]: the heads before position i.  Position i of voxel v = rank[i] + head(i) - 1: start[v] at its head, start[v + 1] behind
// its last member when that is the last indexed position (so start[v + 1] is where voxel v ends for every v); the row's owner.
__global__ __launch_bounds__(VX_BLOCK) void k_voxel_starts(const u64* __restrict__ skey, const u32* __restrict__ srow, u32* rank, u32 n,
                                                          u32* __restrict__ start, u32* __restrict__ out_owner)
{
    const u32 i = blockIdx.x * VX_BLOCK + threadIdx.x;
    if (i >= n) return;
    const u64 k = skey[i];
    if (k == VX_NO_KEY) return;
    const u32 head = IsHead{skey}(i);
    const u32 v = rank[i] + head - 1u;
    rank[i] = v;  // (from here on: the position's voxel)
    if (head) start[v] = i;
    if (i + 1 == n || skey[i + 1] == VX_NO_KEY) start[v + 1] = i + 1;
    const u32 row = srow[i];
    if (out_owner && row < n) out_owner[row] = v;
}

__global__ __launch_bounds__(VX_BLOCK) void k_voxel_heads(const u64* __restrict__ skey, const u32* __restrict__ voxel, const u32* __restrict__ start,
                                                         u32 n, u32 cap, u64* __restrict__ out_keys, u32* __restrict__ out_counts)
{
    const u32 i = blockIdx.x * VX_BLOCK + threadIdx.x;
    if (i >= n) return;
    const u64 k = skey[i];
    if (k == VX_NO_KEY) return;
    const u32 v = voxel[i];
    if (v >= cap || start[v] != i) return;
    if (out_keys) out_keys[v] = k;
    if (out_counts) out_counts[v] = start[v + 1] - i;
}

// columns [col0, col0 + ncols) of `src` (rows of `stride` floats), ncols <= VX_COLS, to columns of the same numbers of `out`
struct Columns {
    const float* src;
    float* out;
    u32 stride, col0, ncols;
};

// One lane per chunk: the position where a chunk starts sums its members in order.  A voxel of one chunk is divided and written
// here; a longer voxel's chunk sums go to their slots.
__global__ __launch_bounds__(VX_BLOCK) void k_voxel_chunks(const u64* __restrict__ skey, const u32* __restrict__ srow, const u32* __restrict__ voxel,
                                                          const u32* __restrict__ start, u32 n, u32 cap, Columns cols, double* __restrict__ chunk)
{
    const u32 i = blockIdx.x * VX_BLOCK + threadIdx.x;
    if (i >= n || skey[i] == VX_NO_KEY) return;
    const u32 v = voxel[i];
    if (v >= cap) return;
    const u32 s = start[v], e = start[v + 1];
    if ((i - s) % VX_CHUNK != 0u) return;
    const u32 end = e - i < VX_CHUNK ? e : i + VX_CHUNK;
    double sum[VX_COLS] = {0.0, 0.0, 0.0, 0.0};
    // (four members' gathers issued together before their adds measured no faster, up to 15 % slower on short voxels: DESIGN.md section 27)
    for (u32 j = i; j < end; ++j) {
        const u32 row = srow[j];
        const float* at = cols.src + static_cast<u64>(row < n ? row : 0u) * cols.stride + cols.col0;
#pragma unroll
        for (u32 k = 0; k < VX_COLS; ++k) {
            if (k < cols.ncols) {
                const double x = static_cast<double>(at[k]);
                sum[k] = j == i ? x : sum[k] + x;  // (S_j starts from its first member, not from zero: -0 stays -0)
            }
        }
    }
    const u32 c = e - s;
    if (c <= VX_CHUNK) {
#pragma unroll
        for (u32 k = 0; k < VX_COLS; ++k)
            if (k < cols.ncols) cols.out[static_cast<u64>(v) * cols.stride + cols.col0 + k] = static_cast<float>(sum[k] / static_cast<double>(c));
    } else {
        double* slot = chunk + static_cast<u64>(chunk_slot(i, s)) * VX_COLS;
#pragma unroll
        for (u32 k = 0; k < VX_COLS; ++k)
            if (k < cols.ncols) slot[k] = sum[k];
    }
}

// One lane per voxel of more than one chunk (the position where it starts): T = S_0, T += S_j in order, T / c.
__global__ __launch_bounds__(VX_BLOCK) void k_voxel_combine(const u64* __restrict__ skey, const u32* __restrict__ voxel, const u32* __restrict__ start, u32 n,
                                                           u32 cap, Columns cols, const double* __restrict__ chunk)
{
    const u32 i = blockIdx.x * VX_BLOCK + threadIdx.x;
    if (i >= n || skey[i] == VX_NO_KEY) return;
    const u32 v = voxel[i];
    if (v >= cap || start[v] != i) return;
    const u32 e = start[v + 1], c = e - i;
    if (c <= VX_CHUNK) return;
    double total[VX_COLS] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (u32 j = i; j < e; j += VX_CHUNK) {
        const double* slot = chunk + static_cast<u64>(chunk_slot(j, i)) * VX_COLS;
#pragma unroll
        for (u32 k = 0; k < VX_COLS; ++k)
            if (k < cols.ncols) total[k] = j == i ? slot[k] : total[k] + slot[k];
        if (e - j <= VX_CHUNK) break;  // (j + 64 may pass 2^32)
    }
#pragma unroll
    for (u32 k = 0; k < VX_COLS; ++k)
        if (k < cols.ncols) cols.out[static_cast<u64>(v) * cols.stride + cols.col0 + k] = static_cast<float>(total[k] / static_cast<double>(c));
}

// near[v] = the minimum over the voxel's members of bits(d2) << 32 | row (d2 >= 0: its bits order as it does).  A wave all of whose
// lanes are members of one voxel -- positions are in voxel order, so most waves of a long voxel -- folds first and adds one atomic.
__global__ __launch_bounds__(VX_BLOCK) void k_voxel_nearest(const float* __restrict__ points, const u64* __restrict__ skey, const u32* __restrict__ srow,
                                                           const u32* __restrict__ voxel, u32 n, u32 cap, const float* __restrict__ centroid,
                                                           u64* __restrict__ near)
{
    const u32 i = blockIdx.x * VX_BLOCK + threadIdx.x;
    const bool in = i < n && skey[i] != VX_NO_KEY;
    const u32 v = in ? voxel[i] : 0xFFFFFFFFu;
    const bool mine = in && v < cap;
    u64 word = ~0ull;
    if (mine) {
        const u32 row = srow[i];
        const u64 at = static_cast<u64>(row < n ? row : 0u) * 3;
        const float dx = points[at] - centroid[static_cast<u64>(v) * 3], dy = points[at + 1] - centroid[static_cast<u64>(v) * 3 + 1],
                    dz = points[at + 2] - centroid[static_cast<u64>(v) * 3 + 2];
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        word = (static_cast<u64>(__float_as_uint(d2)) << 32) | row;
    }
    const u32 first = __builtin_amdgcn_readfirstlane(v);
    const bool one_voxel = __builtin_amdgcn_ballot_w64(mine && v == first) == ~0ull;  // (all 64 lanes, of one voxel)
    if (one_voxel) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const u64 other = __shfl_xor(word, off);
            word = other < word ? other : word;
        }
        if ((threadIdx.x & 63u) == 0) __hip_atomic_fetch_min(&near[v], word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (mine) {
        __hip_atomic_fetch_min(&near[v], word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(VX_BLOCK) void k_voxel_rows(const u64* __restrict__ near, const u64* __restrict__ count, u32 cap, u32* __restrict__ out_rows)
{
    const u32 v = blockIdx.x * VX_BLOCK + threadIdx.x;
    if (v < cap && v < *count) out_rows[v] = static_cast<u32>(near[v]);
}

__global__ __launch_bounds__(64) void k_voxel_finish(const State* __restrict__ st, u64* __restrict__ out_dropped)
{
    if (threadIdx.x == 0) *out_dropped = st->dropped;
}

struct VoxelOut {
    u64* count;
    float *xyz, *attrs;
    u32* counts;
    u64* keys;
    u32 *rows, *owner;
    u64* dropped;
    float* origin;
};

// Everything is enqueued on s, no synchronisation.  base: L.bytes of scratch.
int voxel_device(const Layout& L, char* base, const float* d_points, u64 n64, const float* d_attrs, const pcpx_voxel_params& a, const VoxelOut& o,
                 hipStream_t s)
{
    PCPX_HIP(hipMemsetAsync(o.count, 0, sizeof(u64), s));  // (a scan of nothing writes no total)
    if (n64 == 0) return PCPX_OK;
    const u32 n = static_cast<u32>(n64), cap = static_cast<u32>(L.cap), blocks = blocks_of(n, VX_BLOCK);
    State* st = reinterpret_cast<State*>(base + L.state);
    u64* word[3] = {reinterpret_cast<u64*>(base + L.word[0]), reinterpret_cast<u64*>(base + L.word[1]), reinterpret_cast<u64*>(base + L.word[2])};
    u32* high = reinterpret_cast<u32*>(base + L.high);
    u32* srow = reinterpret_cast<u32*>(base + L.row);
    u32* rank = reinterpret_cast<u32*>(base + L.rank);
    u32* sums = reinterpret_cast<u32*>(base + L.sums);
    u32* start = reinterpret_cast<u32*>(base + L.start);
    double* chunk = reinterpret_cast<double*>(base + L.chunk);
    u64* near = reinterpret_cast<u64*>(base + L.near);
    float* centroid = o.xyz ? o.xyz : reinterpret_cast<float*>(base + L.centroid);
    size_t sort_bytes = L.sort_bytes;
    int r;
    Grid g{{a.leaf[0], a.leaf[1], a.leaf[2]}, {a.origin[0], a.origin[1], a.origin[2]}, (a.flags & PCPX_VOXEL_ORIGIN) ? 1u : 0u};
    k_voxel_begin<<<1, 64, 0, s>>>(st);
    if (!g.fixed) k_voxel_bounds<<<std::min(blocks, VX_BOUNDS_BLOCKS), VX_BLOCK, 0, s>>>(d_points, n, st);
    k_voxel_keys<<<blocks, VX_BLOCK, 0, s>>>(d_points, n, g, st, word[0], high, o.owner, o.origin);
    if ((r = sort_keys_u64(base + L.sort, sort_bytes, word[0], word[1], n, s, 32)) != PCPX_OK) return r;
    k_voxel_second<<<blocks, VX_BLOCK, 0, s>>>(word[1], high, n, word[0]);
    if ((r = sort_keys_u64(base + L.sort, sort_bytes, word[0], word[2], n, s, 32)) != PCPX_OK) return r;
    u64* skey = word[0];
    k_voxel_gather<<<blocks, VX_BLOCK, 0, s>>>(word[1], word[2], n, skey, srow);
    if ((r = exclusive_scan(IsHead{skey}, n, sums, rank, o.count, s)) != PCPX_OK) return r;
    k_voxel_starts<<<blocks, VX_BLOCK, 0, s>>>(skey, srow, rank, n, start, o.owner);
    if (o.dropped) k_voxel_finish<<<1, 64, 0, s>>>(st, o.dropped);
    if (cap) {
        if (o.keys || o.counts) k_voxel_heads<<<blocks, VX_BLOCK, 0, s>>>(skey, rank, start, n, cap, o.keys, o.counts);
        auto columns = [&](const float* src, float* out, u32 stride) {
            for (u32 c0 = 0; c0 < stride; c0 += VX_COLS) {
                const Columns cols{src, out, stride, c0, std::min(VX_COLS, stride - c0)};
                k_voxel_chunks<<<blocks, VX_BLOCK, 0, s>>>(skey, srow, rank, start, n, cap, cols, chunk);
                if (n > VX_CHUNK) k_voxel_combine<<<blocks, VX_BLOCK, 0, s>>>(skey, rank, start, n, cap, cols, chunk);
            }
        };
        if (o.xyz || o.rows) columns(d_points, centroid, 3);
        if (o.attrs) columns(d_attrs, o.attrs, a.attr_columns);
        if (o.rows) {
            PCPX_HIP(hipMemsetAsync(near, 0xFF, static_cast<size_t>(cap) * sizeof(u64), s));
            k_voxel_nearest<<<blocks, VX_BLOCK, 0, s>>>(d_points, skey, srow, rank, n, cap, centroid, near);
            k_voxel_rows<<<blocks_of(cap, VX_BLOCK), VX_BLOCK, 0, s>>>(near, o.count, cap, o.rows);
        }
    }
    PCPX_HIP(hipGetLastError());
    return PCPX_OK;
}

// ---- the refusals ------------------------------------------------------------------------------------------------------------------------
int check_size(const char* what, u64 n)
{
    if (n < VX_N_LIMIT) return PCPX_OK;
    set_error("%s: %llu points: 2^32 - 4096 or more of them", what, static_cast<unsigned long long>(n));
    return PCPX_ERR_INVALID;
}

int check_voxel(const char* what, const void* points, u64 n, const void* attrs, const pcpx_voxel_params* a, const void* count, const void* out_attrs)
{
    int st = check_size(what, n);
    if (st != PCPX_OK) return st;
    if (!points && n) {
        set_error("%s: a NULL array of points with a non-zero size", what);
        return PCPX_ERR_INVALID;
    }
    if (!a) {
        set_error("%s: params is NULL", what);
        return PCPX_ERR_INVALID;
    }
    if (!count) {
        set_error("%s: the count word is NULL", what);
        return PCPX_ERR_INVALID;
    }
    if (a->flags & ~PCPX_VOXEL_ORIGIN) {
        set_error("%s: unknown flag bits 0x%x", what, a->flags & ~PCPX_VOXEL_ORIGIN);
        return PCPX_ERR_INVALID;
    }
    if (a->reserved != 0u) {
        set_error("%s: reserved = %u is not 0", what, a->reserved);
        return PCPX_ERR_INVALID;
    }
    for (int j = 0; j < 3; ++j) {
        if (!(a->leaf[j] > 0.f) || !std::isfinite(a->leaf[j])) {  // (false for a NaN)
            set_error("%s: leaf[%d] = %g is not a finite size above 0", what, j, static_cast<double>(a->leaf[j]));
            return PCPX_ERR_INVALID;
        }
        if ((a->flags & PCPX_VOXEL_ORIGIN) && !std::isfinite(a->origin[j])) {
            set_error("%s: origin[%d] = %g is not finite", what, j, static_cast<double>(a->origin[j]));
            return PCPX_ERR_INVALID;
        }
    }
    if (a->attr_columns > PCPX_VOXEL_ATTRS_MAX) {
        set_error("%s: attr_columns = %u is above %u", what, a->attr_columns, PCPX_VOXEL_ATTRS_MAX);
        return PCPX_ERR_INVALID;
    }
    if (a->attr_columns && !attrs) {
        set_error("%s: attr_columns = %u with a NULL array of attributes", what, a->attr_columns);
        return PCPX_ERR_INVALID;
    }
    if (out_attrs && (!a->attr_columns || !attrs)) {
        set_error("%s: an output for attributes without attributes", what);
        return PCPX_ERR_INVALID;
    }
    return PCPX_OK;
}

}  // namespace
}  // namespace pcpx

using namespace pcpx;

extern "C" {

int pcpx_voxel_plan(uint64_t n, uint64_t capacity, uint64_t* opt_out_sort_bytes, uint64_t* opt_out_scratch_bytes)
{
    static const char* what = "pcpx_voxel_plan";
    return on_host(what, [&]() -> int {
        const int st = check_size(what, n);
        if (st != PCPX_OK) return st;
        const Layout L(n, capacity);
        if (opt_out_sort_bytes) *opt_out_sort_bytes = L.sort_bytes;
        if (opt_out_scratch_bytes) *opt_out_scratch_bytes = L.bytes;
        return PCPX_OK;
    });
}

int pcpx_voxel_grid_dev(const float* d_points, uint64_t n, const float* d_opt_attrs, const pcpx_voxel_params* params, uint64_t capacity,
                        int device, void* stream, uint64_t* d_out_count, float* d_opt_out_xyz, float* d_opt_out_attrs,
                        uint32_t* d_opt_out_counts, uint64_t* d_opt_out_keys, uint32_t* d_opt_out_rows, uint32_t* d_opt_out_owner,
                        uint64_t* d_opt_out_dropped, float* d_opt_out_origin)
{
    static const char* what = "pcpx_voxel_grid_dev";
    const int st = check_voxel(what, d_points, n, d_opt_attrs, params, d_out_count, d_opt_out_attrs);
    if (st != PCPX_OK) return st;
    const Layout L(n, capacity);
    return on_leased(device, what, stream, L.bytes, [&](char* base, hipStream_t s) -> int {
        const VoxelOut out{d_out_count, d_opt_out_xyz, d_opt_out_attrs, d_opt_out_counts, d_opt_out_keys, d_opt_out_rows, d_opt_out_owner,
                           d_opt_out_dropped, d_opt_out_origin};
        return voxel_device(L, base, d_points, n, d_opt_attrs, *params, out, s);
    });
}

int pcpx_voxel_grid(const float* points, uint64_t n, const float* opt_attrs, const pcpx_voxel_params* params, uint64_t capacity, int device,
                    uint64_t* out_count, float* opt_out_xyz, float* opt_out_attrs, uint32_t* opt_out_counts, uint64_t* opt_out_keys,
                    uint32_t* opt_out_rows, uint32_t* opt_out_owner, uint64_t* opt_out_dropped, float* opt_out_origin)
{
    static const char* what = "pcpx_voxel_grid";
    const int st = check_voxel(what, points, n, opt_attrs, params, out_count, opt_out_attrs);
    if (st != PCPX_OK) return st;
    return on_host_call(device, what, [&](HostCall& call) -> int {
        // (without out_xyz the call only counts: nothing per voxel is made)
        const Layout L(n, opt_out_xyz ? capacity : 0);
        const u64 cap = L.cap, A = params->attr_columns;
        struct Small {
            u64 count, dropped;
            float origin[4];
        } host{0, 0, {0.f, 0.f, 0.f, 0.f}};
        const float* d_points = call.upload(points, n * 3 * sizeof(float));
        const float* d_attrs = call.upload(opt_out_attrs ? opt_attrs : nullptr, n * A * sizeof(float));
        Small* d = call.alloc<Small>(sizeof(Small));
        float* xyz = call.alloc_for(opt_out_xyz, cap * 3 * sizeof(float));
        float* attrs = call.alloc_for(opt_out_attrs, cap * A * sizeof(float));
        u32* counts = call.alloc_for(opt_out_counts, cap * sizeof(u32));
        u64* keys = call.alloc_for(opt_out_keys, cap * sizeof(u64));
        u32* rows = call.alloc_for(opt_out_rows, cap * sizeof(u32));
        u32* owner = call.alloc_for(opt_out_owner, n * sizeof(u32));
        char* base = call.scratch(L.bytes);
        int r;
        if ((r = call.st) != PCPX_OK) return r;
        PCPX_HIP(hipMemsetAsync(d, 0, sizeof(Small), call.s));
        const VoxelOut out{&d->count, xyz, attrs, counts, keys, rows, owner, &d->dropped, d->origin};
        if ((r = voxel_device(L, base, d_points, n, d_attrs, *params, out, call.s)) != PCPX_OK || (r = call.download(&host, d, sizeof(Small))) != PCPX_OK ||
            (r = call.wait()) != PCPX_OK)
            return r;
        *out_count = host.count;
        if (n == 0) return PCPX_OK;
        if (!opt_out_xyz || capacity < host.count) {
            set_error("%s: %llu voxels, room for %llu", what, static_cast<unsigned long long>(host.count),
                      static_cast<unsigned long long>(opt_out_xyz ? capacity : 0));
            return PCPX_ERR_CAPACITY;
        }
        const u64 V = host.count;
        if (V) {
            call.download(opt_out_xyz, xyz, V * 3 * sizeof(float));
            call.download_opt(opt_out_attrs, attrs, V * A * sizeof(float));
            call.download_opt(opt_out_counts, counts, V * sizeof(u32));
            call.download_opt(opt_out_keys, keys, V * sizeof(u64));
            call.download_opt(opt_out_rows, rows, V * sizeof(u32));
        }
        call.download_opt(opt_out_owner, owner, n * sizeof(u32));
        if ((r = call.wait()) != PCPX_OK) return r;
        if (opt_out_dropped) *opt_out_dropped = host.dropped;
        if (opt_out_origin) std::copy(host.origin, host.origin + 3, opt_out_origin);
        return PCPX_OK;
    });
}

}  // extern "C"
