// pcpx_match.hip -- descriptor matching by brute force over all pairs (include/pcpx_match.h): the nearest and
// second nearest target row of every source row, the ratio test and the mutual test.  The form is k_fpfh's inner loop without a
// walk: one lane per source row with that row in registers, the target's record a wave-uniform scalar load, W x (sub, mul, add)
// per pair.  No neighbour list, no m x n matrix, no LDS, nothing between workgroups:
//   k_match_pack    rows -> zero-padded records of a compiled width W, and a validity byte per row
//   k_match<W, CH>  one wavefront per (64 consecutive sources, one segment of the targets): two keys per lane
//   k_match_merge   one thread per source over its segments' keys
//   k_match_keep    ratio and mutual test, one thread per source; pcpx_scan.h and k_match_compact write the kept pairs
// The mutual test is the same two kernels with the roles of the sets swapped.
#include "pcpx_device.h"
#include "pcpx_lease.h"
#include "pcpx_match.h"
#include "pcpx_scan.h"

#include <algorithm>
#include <limits>

namespace pcpx {

namespace {

constexpr u32 MT_BLOCK = 256;          // threads of the row-wise kernels
constexpr u32 MT_WAVES = 4;            // waves of a k_match block: four consecutive source groups on one segment (they share its records in the scalar cache)
constexpr u32 MT_MAX_DIMS = PCPX_MATCH_MAX_DIMS;
constexpr u32 MT_PAD = 0xFFFFFFFFu;    // d2 word and index of "no target": above every real d2 (a NaN is skipped, +inf is 0x7F800000)
constexpr u64 MT_PAD_KEY = ~0ull;
static_assert(PCPX_MATCH_NONE == MT_PAD, "no match = the padding key's index");
// The plan.  A wave is 64 sources on one segment; the device holds 256 CUs x 4 SIMDs x a handful of such waves, and a call should
// be several rounds of that so that its last round is not a large part of it.  A segment is never shorter than MT_MIN_SEGMENT_ROWS
// (a wave's prologue -- its source rows, W loads per lane -- is paid per segment) and there are never more than MT_MAX_SEGMENTS
// (k_match_merge reads 16 bytes per source and segment, one thread per source).  Segment lengths are multiples of
// MT_MIN_SEGMENT_ROWS, so the last segment is whatever is left: anything from one row to a full segment.
// (segment_plan of pcpx_ransac.h has this formula and these values.  This file keeps its own: that header defines k_ransac_best and
// k_reg_compact, which would be compiled into this file with it and are no part of a matching call.)
constexpr u64 MT_TARGET_WAVES = 16384;
constexpr u64 MT_MAX_SEGMENTS = 256;
constexpr u64 MT_MIN_SEGMENT_ROWS = 256;

// the compiled record widths: the smallest one >= dims is used (33 floats of an FPFH pay for 36)
constexpr u32 MT_WIDTHS[] = {4, 8, 16, 24, 36, 48, 64};
inline u32 width_for(u32 dims)
{
    for (u32 w : MT_WIDTHS)
        if (w >= dims) return w;
    return 0;
}


struct Split {
    u32 segments = 0;
    u64 rows = 0;  // per segment
};
// how `n` rows are cut for `m` rows on the lanes
inline Split split_for(u64 m, u64 n)
{
    Split s;
    if (n == 0) return s;
    const u64 groups = std::max<u64>(1, (m + GROUP - 1) / GROUP);
    const u64 want = (MT_TARGET_WAVES + groups - 1) / groups;
    const u64 s0 = std::max<u64>(1, std::min({want, MT_MAX_SEGMENTS, n / MT_MIN_SEGMENT_ROWS}));
    s.rows = ((n + s0 - 1) / s0 + MT_MIN_SEGMENT_ROWS - 1) / MT_MIN_SEGMENT_ROWS * MT_MIN_SEGMENT_ROWS;
    s.segments = static_cast<u32>((n + s.rows - 1) / s.rows);
    return s;
}

// Where everything lies in the scratch of a call (byte offsets, each a multiple of 256).  One layout for every call: what a nearest
// call does not use (the reverse keys, the compaction's arrays) is small beside the records.
struct Layout {
    u32 width = 0;
    Split fwd, rev;  // targets cut for the sources on the lanes; sources cut for the targets on the lanes (mutual test)
    size_t tgt_rec = 0, src_rec = 0, tgt_valid = 0, src_valid = 0, part = 0, best_idx = 0, best_d2 = 0, second_d2 = 0, rev_idx = 0, keep = 0, place = 0,
           sums = 0, bytes = 0;
    Layout(u64 m, u64 n, u32 dims)
    {
        width = width_for(dims);
        fwd = split_for(m, n), rev = split_for(n, m);
        Carve c;
        tgt_rec = c.take(n * width * sizeof(float));
        src_rec = c.take(m * width * sizeof(float));
        tgt_valid = c.take(n);
        src_valid = c.take(m);
        // two keys per (row on a lane, segment): the larger of the two directions, which run one after the other
        part = c.take(std::max<u64>(static_cast<u64>(fwd.segments) * m, static_cast<u64>(rev.segments) * n) * 2 * sizeof(u64));
        best_idx = c.take(m * sizeof(u32));
        best_d2 = c.take(m * sizeof(float));
        second_d2 = c.take(m * sizeof(float));
        rev_idx = c.take(n * sizeof(u32));
        keep = c.take(m);
        place = c.take(m * sizeof(u32));
        sums = c.take(static_cast<u64>(scan_tiles(m)) * sizeof(u32));
        bytes = c.bytes();
    }
};

// One thread per row: the row into its record, the tail zero, and valid = 0 for a row that takes no part (skip_zero: every entry +-0;
// a NaN is not zero).  Such a record's first float is made NaN, so every d2 with it is NaN and the pair is skipped: the pair loop has
// no test of its own for it.
__global__ __launch_bounds__(MT_BLOCK) void k_match_pack(const float* __restrict__ rows, u32 n, u32 dims, u32 width, u32 skip_zero,
                                                         float* __restrict__ rec, uint8_t* __restrict__ valid)
{
    const u32 i = blockIdx.x * MT_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float* in = rows + static_cast<u64>(i) * dims;
    float* out = rec + static_cast<u64>(i) * width;
    bool nonzero = false;
    for (u32 b = 0; b < width; ++b) {
        const float v = b < dims ? in[b] : 0.f;
        nonzero = nonzero || v != 0.f;
        out[b] = v;
    }
    const bool ok = !skip_zero || nonzero;
    if (!ok) out[0] = std::numeric_limits<float>::quiet_NaN();
    valid[i] = ok ? 1 : 0;
}

template <int N>
struct Chunk {
    float v[N];
};

// One wavefront per (64 consecutive rows of `a` on the lanes, one segment of the rows of `b`).  The lane's row is W registers,
// statically indexed; a record of b arrives in chunks of CH floats (W or W / 2: two chunks in flight have to fit the scalar
// registers), each a scalar load written one chunk ahead of its arithmetic (where hipcc then issues it: DESIGN.md section 23; the
// other waves of the SIMD cover what is left of its latency).  The rows of b come in ascending order, so "strictly
// smaller d2 word" is the key order (d2 bits, index) and the four words of a lane are its best and second key of the segment.
// part[(segment * na + row) * 2 + {0, 1}] = those keys, MT_PAD_KEY where there is none.
template <int WIDTH, int CH>
__global__ __launch_bounds__(64 * MT_WAVES) void k_match(const float* __restrict__ a_rec, const uint8_t* __restrict__ a_valid, u32 na,
                                                        const float* __restrict__ b_rec, u32 nb, u64 seg_rows, u64* __restrict__ part)
{
    static_assert(WIDTH % CH == 0 && WIDTH % 4 == 0, "chunks of a record");
    constexpr int NCH = WIDTH / CH;
    const u32 lane = threadIdx.x & 63u;
    const u64 g = static_cast<u64>(blockIdx.x) * MT_WAVES + (threadIdx.x >> 6);
    if (g * GROUP >= na) return;  // (wave-uniform)
    const u64 row = g * GROUP + lane;
    const bool active = row < na && a_valid[row] != 0;
    float s[WIDTH];
#pragma unroll
    for (int b = 0; b < WIDTH; b += 4) {
        const float4 v = active ? *reinterpret_cast<const float4*>(a_rec + row * WIDTH + b) : float4{0.f, 0.f, 0.f, 0.f};
        s[b] = v.x, s[b + 1] = v.y, s[b + 2] = v.z, s[b + 3] = v.w;
    }
    const u64 t0 = blockIdx.y * seg_rows, t1 = t0 + seg_rows < nb ? t0 + seg_rows : nb;  // (t0 < nb: the plan's segments cover nb)
    const Chunk<CH>* chunks = reinterpret_cast<const Chunk<CH>*>(b_rec);
    u64 q = t0 * NCH;
    const u64 q_last = t1 * NCH - 1;
    Chunk<CH> cur = load_const(chunks + q);
    u32 u1 = MT_PAD, i1 = MT_PAD, u2 = MT_PAD, i2 = MT_PAD;
    for (u64 t = t0; t < t1; ++t) {
        float acc = 0.f;
#pragma unroll
        for (int h = 0; h < NCH; ++h) {
            ++q;
            const Chunk<CH> next = load_const(chunks + (q < q_last ? q : q_last));  // (the last one again rather than past the end)
#pragma unroll
            for (int b = 0; b < CH; ++b) {
                const float e = s[h * CH + b] - cur.v[b];
                const float p = e * e;
                acc = (h == 0 && b == 0) ? p : acc + p;
            }
            cur = next;
        }
        const u32 u = acc == acc ? __float_as_uint(acc) : MT_PAD;  // (a NaN never compares below anything)
        const u32 ti = static_cast<u32>(t);
        const bool lt1 = u < u1, lt2 = u < u2;
        u2 = lt1 ? u1 : (lt2 ? u : u2);
        i2 = lt1 ? i1 : (lt2 ? ti : i2);
        u1 = lt1 ? u : u1;
        i1 = lt1 ? ti : i1;
    }
    if (row >= na) return;
    ulonglong2 keys;
    keys.x = active ? (static_cast<u64>(u1) << 32) | i1 : MT_PAD_KEY;
    keys.y = active ? (static_cast<u64>(u2) << 32) | i2 : MT_PAD_KEY;
    reinterpret_cast<ulonglong2*>(part)[static_cast<u64>(blockIdx.y) * na + row] = keys;
}

// One thread per row: the smallest and second-smallest of its segments' keys.  The key order is total and no two keys of a row are
// equal (but for the padding), so the result does not depend on how the other set was cut.  Any output may be null.
__global__ __launch_bounds__(MT_BLOCK) void k_match_merge(const u64* __restrict__ part, u32 na, u32 segments, u32* __restrict__ out_idx,
                                                          float* __restrict__ out_d2, u32* __restrict__ out_second_idx,
                                                          float* __restrict__ out_second_d2)
{
    const u32 i = blockIdx.x * MT_BLOCK + threadIdx.x;
    if (i >= na) return;
    const ulonglong2* keys = reinterpret_cast<const ulonglong2*>(part);
    u64 k1 = MT_PAD_KEY, k2 = MT_PAD_KEY;
#pragma unroll 4
    for (u32 s = 0; s < segments; ++s) {
        const ulonglong2 c = keys[static_cast<u64>(s) * na + i];  // (c.x <= c.y)
        if (c.x < k1) {
            k2 = c.y < k1 ? c.y : k1;
            k1 = c.x;
        } else if (c.x < k2) {
            k2 = c.x;
        }
    }
    const float inf = std::numeric_limits<float>::infinity();
    if (out_idx) out_idx[i] = static_cast<u32>(k1);
    if (out_d2) out_d2[i] = k1 == MT_PAD_KEY ? inf : __uint_as_float(static_cast<u32>(k1 >> 32));
    if (out_second_idx) out_second_idx[i] = static_cast<u32>(k2);
    if (out_second_d2) out_second_d2[i] = k2 == MT_PAD_KEY ? inf : __uint_as_float(static_cast<u32>(k2 >> 32));
}

// One thread per source: the keep decision of pcpx_match.h (rev_idx: the best source of every target, or null without the mutual test).
__global__ __launch_bounds__(MT_BLOCK) void k_match_keep(u32 m, const u32* __restrict__ best_idx, const float* __restrict__ best_d2,
                                                         const float* __restrict__ second_d2, float max_ratio_sq, const u32* __restrict__ rev_idx,
                                                         uint8_t* __restrict__ keep)
{
    const u32 i = blockIdx.x * MT_BLOCK + threadIdx.x;
    if (i >= m) return;
    const u32 j = best_idx[i];
    bool k = j != MT_PAD && best_d2[i] <= max_ratio_sq * second_d2[i];
    if (k && rev_idx) k = rev_idx[j] == i;
    keep[i] = k ? 1 : 0;
}

struct IsKept {
    const uint8_t* keep;
    __device__ u32 operator()(u32 i) const { return keep[i]; }
};

__global__ __launch_bounds__(MT_BLOCK) void k_match_compact(u32 m, const uint8_t* __restrict__ keep, const u32* __restrict__ place,
                                                            const u32* __restrict__ best_idx, const float* __restrict__ best_d2,
                                                            u32* __restrict__ out_pairs, float* __restrict__ out_d2)
{
    const u32 i = blockIdx.x * MT_BLOCK + threadIdx.x;
    if (i >= m || !keep[i]) return;
    const u32 at = place[i];
    out_pairs[2ull * at] = i;  // (two words: the caller's array is only 4-byte aligned, include/pcpx.h)
    out_pairs[2ull * at + 1] = best_idx[i];
    if (out_d2) out_d2[at] = best_d2[i];
}

template <int WIDTH, int CH>
void launch_match(const float* a_rec, const uint8_t* a_valid, u32 na, const float* b_rec, u32 nb, const Split& cut, u64* part, hipStream_t s)
{
    const dim3 grid(blocks_of((static_cast<u64>(na) + GROUP - 1) / GROUP, MT_WAVES), cut.segments);
    k_match<WIDTH, CH><<<grid, 64 * MT_WAVES, 0, s>>>(a_rec, a_valid, na, b_rec, nb, cut.rows, part);
}

// best and second of every row of `a` among the rows of `b` (records of `width` floats), the rows of b cut as `cut` says
int match_pass(u32 width, const float* a_rec, const uint8_t* a_valid, u64 na, const float* b_rec, u64 nb, const Split& cut, u64* part, u32* out_idx,
               float* out_d2, u32* out_second_idx, float* out_second_d2, hipStream_t s)
{
    if (na == 0) return PCPX_OK;
    const u32 a = static_cast<u32>(na), b = static_cast<u32>(nb);
    if (nb != 0) {
        switch (width) {
        case 4: launch_match<4, 4>(a_rec, a_valid, a, b_rec, b, cut, part, s); break;
        case 8: launch_match<8, 8>(a_rec, a_valid, a, b_rec, b, cut, part, s); break;
        case 16: launch_match<16, 16>(a_rec, a_valid, a, b_rec, b, cut, part, s); break;
        case 24: launch_match<24, 24>(a_rec, a_valid, a, b_rec, b, cut, part, s); break;
        case 36: launch_match<36, 18>(a_rec, a_valid, a, b_rec, b, cut, part, s); break;
        case 48: launch_match<48, 24>(a_rec, a_valid, a, b_rec, b, cut, part, s); break;
        case 64: launch_match<64, 32>(a_rec, a_valid, a, b_rec, b, cut, part, s); break;
        default: set_error("pcpx_match: no kernel of width %u", width); return PCPX_ERR_INVALID;
        }
    }
    k_match_merge<<<blocks_of(na, MT_BLOCK), MT_BLOCK, 0, s>>>(part, a, cut.segments, out_idx, out_d2, out_second_idx, out_second_d2);
    PCPX_HIP(hipGetLastError());
    return PCPX_OK;
}

int pack_both(const Layout& L, char* base, const float* d_src, u64 m, const float* d_tgt, u64 n, u32 dims, u32 flags, hipStream_t s)
{
    const u32 skip = (flags & PCPX_MATCH_SKIP_ZERO_ROWS) ? 1u : 0u;
    if (m)
        k_match_pack<<<blocks_of(m, MT_BLOCK), MT_BLOCK, 0, s>>>(d_src, static_cast<u32>(m), dims, L.width, skip, reinterpret_cast<float*>(base + L.src_rec),
                                                                reinterpret_cast<uint8_t*>(base + L.src_valid));
    if (n)
        k_match_pack<<<blocks_of(n, MT_BLOCK), MT_BLOCK, 0, s>>>(d_tgt, static_cast<u32>(n), dims, L.width, skip, reinterpret_cast<float*>(base + L.tgt_rec),
                                                                reinterpret_cast<uint8_t*>(base + L.tgt_valid));
    PCPX_HIP(hipGetLastError());
    return PCPX_OK;
}

// Everything is enqueued on s, no synchronisation.  base: L.bytes of scratch.
int nearest_device(const Layout& L, char* base, const float* d_src, u64 m, const float* d_tgt, u64 n, u32 dims, u32 flags, hipStream_t s, u32* d_out_idx,
                   float* d_out_d2, u32* d_out_second_idx, float* d_out_second_d2)
{
    int st;
    if (m == 0) return PCPX_OK;
    if ((st = pack_both(L, base, d_src, m, d_tgt, n, dims, flags, s)) != PCPX_OK) return st;
    return match_pass(L.width, reinterpret_cast<float*>(base + L.src_rec), reinterpret_cast<uint8_t*>(base + L.src_valid), m,
                      reinterpret_cast<float*>(base + L.tgt_rec), n, L.fwd, reinterpret_cast<u64*>(base + L.part), d_out_idx, d_out_d2, d_out_second_idx,
                      d_out_second_d2, s);
}

int correspondences_device(const Layout& L, char* base, const float* d_src, u64 m, const float* d_tgt, u64 n, u32 dims, float max_ratio_sq, u32 flags,
                           hipStream_t s, u32* d_out_pairs, float* d_out_d2, u64* d_out_count)
{
    int st;
    if (m == 0) {
        if (d_out_count) PCPX_HIP(hipMemsetAsync(d_out_count, 0, sizeof(u64), s));
        return PCPX_OK;
    }
    u32* best_idx = reinterpret_cast<u32*>(base + L.best_idx);
    float* best_d2 = reinterpret_cast<float*>(base + L.best_d2);
    float* second_d2 = reinterpret_cast<float*>(base + L.second_d2);
    u32* rev_idx = (flags & PCPX_MATCH_MUTUAL) && n ? reinterpret_cast<u32*>(base + L.rev_idx) : nullptr;
    uint8_t* keep = reinterpret_cast<uint8_t*>(base + L.keep);
    u32* place = reinterpret_cast<u32*>(base + L.place);
    if ((st = nearest_device(L, base, d_src, m, d_tgt, n, dims, flags, s, best_idx, best_d2, nullptr, second_d2)) != PCPX_OK) return st;
    if (rev_idx &&
        (st = match_pass(L.width, reinterpret_cast<float*>(base + L.tgt_rec), reinterpret_cast<uint8_t*>(base + L.tgt_valid), n,
                         reinterpret_cast<float*>(base + L.src_rec), m, L.rev, reinterpret_cast<u64*>(base + L.part), rev_idx, nullptr, nullptr, nullptr,
                         s)) != PCPX_OK)
        return st;
    k_match_keep<<<blocks_of(m, MT_BLOCK), MT_BLOCK, 0, s>>>(static_cast<u32>(m), best_idx, best_d2, second_d2, max_ratio_sq, rev_idx, keep);
    if ((st = exclusive_scan(IsKept{keep}, m, reinterpret_cast<u32*>(base + L.sums), place, d_out_count, s)) != PCPX_OK) return st;
    k_match_compact<<<blocks_of(m, MT_BLOCK), MT_BLOCK, 0, s>>>(static_cast<u32>(m), keep, place, best_idx, best_d2, d_out_pairs, d_out_d2);
    PCPX_HIP(hipGetLastError());
    return PCPX_OK;
}

int check_match_args(const char* what, const void* src, u64 m, const void* tgt, u64 n, u32 dims, u32 flags, u32 known_flags, const void* out)
{
    if (dims == 0 || dims > MT_MAX_DIMS) {
        set_error("%s: dims = %u is not in 1 .. %u", what, dims, MT_MAX_DIMS);
        return PCPX_ERR_INVALID;
    }
    if (m >= 0xFFFFFFFFull || n >= 0xFFFFFFFFull) {
        set_error("%s: %llu x %llu rows: more than 2^32 - 2 of them", what, static_cast<unsigned long long>(m), static_cast<unsigned long long>(n));
        return PCPX_ERR_INVALID;
    }
    if (flags & ~known_flags) {
        set_error("%s: unknown flag bits 0x%x", what, flags & ~known_flags);
        return PCPX_ERR_INVALID;
    }
    if ((!src && m) || (!tgt && n)) {
        set_error("%s: a NULL array of rows with a non-zero count", what);
        return PCPX_ERR_INVALID;
    }
    if (!out && m) {
        set_error("%s: the output array is NULL", what);
        return PCPX_ERR_INVALID;
    }
    return PCPX_OK;
}

int check_ratio(const char* what, float max_ratio_sq)
{
    if (max_ratio_sq >= 0.f && max_ratio_sq <= 1.f) return PCPX_OK;  // (false for a NaN)
    set_error("%s: max_ratio_sq = %g is not in [0, 1]", what, static_cast<double>(max_ratio_sq));
    return PCPX_ERR_INVALID;
}

}  // namespace

}  // namespace pcpx

using namespace pcpx;

extern "C" {

int pcpx_match_plan(uint64_t m, uint64_t n, uint32_t dims, uint32_t* out_width, uint32_t* out_segments, uint64_t* out_segment_rows,
                    uint64_t* out_scratch_bytes)
{
    static const char* what = "pcpx_match_plan";
    return on_host(what, [&]() -> int {
        const int st = check_match_args(what, &m, m, &n, n, dims, 0, 0, &m);  // (dims and the counts; there are no arrays)
        if (st != PCPX_OK) return st;
        const Layout L(m, n, dims);
        if (out_width) *out_width = L.width;
        if (out_segments) *out_segments = L.fwd.segments;
        if (out_segment_rows) *out_segment_rows = L.fwd.rows;
        if (out_scratch_bytes) *out_scratch_bytes = L.bytes;
        return PCPX_OK;
    });
}

int pcpx_match_nearest_dev(const float* d_src, uint64_t m, const float* d_tgt, uint64_t n, uint32_t dims, uint32_t flags, int device,
                           void* stream, uint32_t* d_out_idx, float* d_opt_out_d2, uint32_t* d_opt_out_second_idx,
                           float* d_opt_out_second_d2)
{
    static const char* what = "pcpx_match_nearest_dev";
    int st = check_match_args(what, d_src, m, d_tgt, n, dims, flags, PCPX_MATCH_SKIP_ZERO_ROWS, d_out_idx);
    if (st != PCPX_OK || m == 0) return st;
    const Layout L(m, n, dims);
    return on_leased(device, what, stream, L.bytes, [&](char* base, hipStream_t s) -> int {
        return nearest_device(L, base, d_src, m, d_tgt, n, dims, flags, s, d_out_idx, d_opt_out_d2, d_opt_out_second_idx, d_opt_out_second_d2);
    });
}

int pcpx_match_nearest(const float* src, uint64_t m, const float* tgt, uint64_t n, uint32_t dims, uint32_t flags, int device,
                       uint32_t* out_idx, float* opt_out_d2, uint32_t* opt_out_second_idx, float* opt_out_second_d2)
{
    static const char* what = "pcpx_match_nearest";
    int st = check_match_args(what, src, m, tgt, n, dims, flags, PCPX_MATCH_SKIP_ZERO_ROWS, out_idx);
    if (st != PCPX_OK || m == 0) return st;
    return on_host_call(device, what, [&](HostCall& call) -> int {
        const Layout L(m, n, dims);
        const float* d_src = call.upload(src, m * dims * sizeof(float));
        const float* d_tgt = call.upload(tgt, n * dims * sizeof(float));
        u32* di = call.alloc<u32>(m * sizeof(u32));
        float* dd = opt_out_d2 ? call.alloc<float>(m * sizeof(float)) : nullptr;
        u32* dsi = opt_out_second_idx ? call.alloc<u32>(m * sizeof(u32)) : nullptr;
        float* dsd = opt_out_second_d2 ? call.alloc<float>(m * sizeof(float)) : nullptr;
        char* base = call.scratch(L.bytes);
        int r;
        if ((r = call.st) != PCPX_OK || (r = nearest_device(L, base, d_src, m, d_tgt, n, dims, flags, call.s, di, dd, dsi, dsd)) != PCPX_OK ||
            (r = call.download(out_idx, di, m * sizeof(u32))) != PCPX_OK || (dd && (r = call.download(opt_out_d2, dd, m * sizeof(float))) != PCPX_OK) ||
            (dsi && (r = call.download(opt_out_second_idx, dsi, m * sizeof(u32))) != PCPX_OK) ||
            (dsd && (r = call.download(opt_out_second_d2, dsd, m * sizeof(float))) != PCPX_OK))
            return r;
        return call.wait();
    });
}

int pcpx_match_correspondences_dev(const float* d_src, uint64_t m, const float* d_tgt, uint64_t n, uint32_t dims, float max_ratio_sq,
                                   uint32_t flags, int device, void* stream, uint32_t* d_out_pairs, float* d_opt_out_d2,
                                   uint64_t* d_opt_out_count)
{
    static const char* what = "pcpx_match_correspondences_dev";
    int st = check_match_args(what, d_src, m, d_tgt, n, dims, flags, PCPX_MATCH_SKIP_ZERO_ROWS | PCPX_MATCH_MUTUAL, d_out_pairs);
    if (st != PCPX_OK || (st = check_ratio(what, max_ratio_sq)) != PCPX_OK) return st;
    if (m == 0 && !d_opt_out_count) return PCPX_OK;
    const Layout L(m, n, dims);
    if (m == 0) {  // (only the count word is cleared: no scratch)
        if (device < 0 || device >= LEASE_MAX_DEVICES) return select_device(device);
        return on_shared(device, what, [&](DeviceShared&) -> int {
            return correspondences_device(L, nullptr, d_src, m, d_tgt, n, dims, max_ratio_sq, flags, static_cast<hipStream_t>(stream), d_out_pairs, d_opt_out_d2,
                                          d_opt_out_count);
        });
    }
    return on_leased(device, what, stream, L.bytes, [&](char* base, hipStream_t s) -> int {
        return correspondences_device(L, base, d_src, m, d_tgt, n, dims, max_ratio_sq, flags, s, d_out_pairs, d_opt_out_d2, d_opt_out_count);
    });
}

int pcpx_match_correspondences(const float* src, uint64_t m, const float* tgt, uint64_t n, uint32_t dims, float max_ratio_sq, uint32_t flags,
                               int device, uint32_t* out_pairs, float* opt_out_d2, uint64_t* out_count)
{
    static const char* what = "pcpx_match_correspondences";
    if (!out_count) {
        set_error("%s: the count is NULL", what);
        return PCPX_ERR_INVALID;
    }
    *out_count = 0;
    int st = check_match_args(what, src, m, tgt, n, dims, flags, PCPX_MATCH_SKIP_ZERO_ROWS | PCPX_MATCH_MUTUAL, out_pairs);
    if (st != PCPX_OK || (st = check_ratio(what, max_ratio_sq)) != PCPX_OK || m == 0) return st;
    return on_host_call(device, what, [&](HostCall& call) -> int {
        const Layout L(m, n, dims);
        const float* d_src = call.upload(src, m * dims * sizeof(float));
        const float* d_tgt = call.upload(tgt, n * dims * sizeof(float));
        u32* dp = call.alloc<u32>(m * 2 * sizeof(u32));
        float* dd = opt_out_d2 ? call.alloc<float>(m * sizeof(float)) : nullptr;
        u64* dc = call.alloc<u64>(sizeof(u64));
        char* base = call.scratch(L.bytes);
        u64 count = 0;
        int r;
        if ((r = call.st) != PCPX_OK || (r = correspondences_device(L, base, d_src, m, d_tgt, n, dims, max_ratio_sq, flags, call.s, dp, dd, dc)) != PCPX_OK ||
            (r = call.download(&count, dc, sizeof(u64))) != PCPX_OK || (r = call.wait()) != PCPX_OK)
            return r;
        if (count) {
            if ((r = call.download(out_pairs, dp, count * 2 * sizeof(u32))) != PCPX_OK ||
                (dd && (r = call.download(opt_out_d2, dd, count * sizeof(float))) != PCPX_OK) || (r = call.wait()) != PCPX_OK)
                return r;
        }
        *out_count = count;
        return PCPX_OK;
    });
}

}  // extern "C"
