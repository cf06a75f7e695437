// pcpx_boundary.hip -- boundary points of the indexed cloud by the angle criterion (include/pcpx_boundary.h).
// A ninth form of the leaf-direct sphere walk of pcpx_device.h: its pair work is "within r, then the sector of the partner's
// direction in my tangent plane", and its state per lane is the 64-bit set of the sectors seen.  It needs the centre's normal only:
// no partner-side record, no LDS, no neighbour list.  The set is an OR over the partners, so the answer is exact whatever the walk's
// order; the longest empty run and its start are found per lane once the walk is done.
#include "pcpx_boundary.h"
#include "pcpx_keep.h"

namespace pcpx {

namespace {

// T_k of the header, k = 1 .. 7
constexpr float tan_k(int k)
{
    constexpr float tans[7] = PCPX_BOUNDARY_TANS;
    return tans[k - 1];
}

// The sector 0 .. 63 of the direction (a, b), not both zero (the header's rule, the seven compares as three steps of a binary
// search: T_k x does not decrease with k).
__device__ __forceinline__ u32 sector_of(const float a, const float b)
{
    constexpr float T1 = tan_k(1), T2 = tan_k(2), T3 = tan_k(3), T4 = tan_k(4), T5 = tan_k(5), T6 = tan_k(6), T7 = tan_k(7);
    const float fa = __builtin_fabsf(a), fb = __builtin_fabsf(b);
    const bool swap = fb > fa;
    const float x = swap ? fb : fa, y = swap ? fa : fb;
    const bool ge4 = y >= T4 * x;
    const bool ge2 = y >= (ge4 ? T6 : T2) * x;
    const float t1 = ge4 ? (ge2 ? T7 : T5) : (ge2 ? T3 : T1);
    const bool ge1 = y >= t1 * x;
    const u32 sub = (ge4 ? 4u : 0u) + (ge2 ? 2u : 0u) + (ge1 ? 1u : 0u);
    const u32 q = swap ? 15u - sub : sub;
    return b < 0.f ? (a < 0.f ? 32u + q : 63u - q) : (a < 0.f ? 31u - q : q);
}

// bit p of the result = bit (p + k) mod 64 of x, k in 0 .. 63
__device__ __forceinline__ u64 rotated_down(const u64 x, const u32 k) { return (x >> k) | (x << ((64u - k) & 63u)); }

// The longest cyclic run of zero bits of `mask` and where its lowest instance starts.  R(k) = the positions from which k bits
// of ~mask are set; R(a + b) = R(a) & rotated_down(R(b), a).  Six doublings give R(1), R(2), .. R(32); the longest run's length is
// then put together from its binary digits, high to low -- 12 rotations, no loop over the bits.  A run of exactly that length is
// maximal, so the bit below its start is set.
__device__ __forceinline__ void longest_gap(const u64 mask, u32& gap, u32& start)
{
    gap = mask == 0ull ? 64u : 0u;
    start = 0u;
    if (mask == 0ull || mask == ~0ull) return;
    u64 runs[6];
    runs[0] = ~mask;
#pragma unroll
    for (int j = 0; j < 5; ++j) runs[j + 1] = runs[j] & rotated_down(runs[j], 1u << j);
    u64 at = ~0ull;  // R(0)
    u32 len = 0u;
#pragma unroll
    for (int j = 5; j >= 0; --j) {
        const u64 longer = at & rotated_down(runs[j], len);
        if (longer != 0ull) {
            at = longer;
            len += 1u << j;
        }
    }
    gap = len;
    start = static_cast<u32>(__builtin_ctzll(at));
}

// What the walk writes, by input row; any but keep may be null.
struct BoundaryOut {
    uint8_t* keep = nullptr;
    uint8_t* gap = nullptr;  // rows x 2: {G, start}
    u32* count = nullptr;
    u64* sectors = nullptr;
};

// One wave per group of 64 curve-consecutive positions, one lane per indexed point.  The lane gathers its normal by input row once
// and keeps u and v in six registers, the set in two and the count in one.  A lane without a frame walks for its count with
// u = v = 0; its set is cleared at the end.  The sector arithmetic is under the distance test's branch, by measurement: predicated
// for all eight points of every visited leaf it took 8.22 ms against 4.54 ms per 10 M points at ~42 neighbours, with the same
// bits (profiles/r24_boundary.json) -- most points of a visited leaf are in no lane's sphere.
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void k_boundary(TreeView t, u32 group_end, float radius, const float* __restrict__ normals,
                                                                  u32 gap_sectors, u32 at_least, BoundaryOut out)
{
    const u32 lane = threadIdx.x & 63u;
    const u32 g = virtual_block() * WAVES_PER_BLOCK + wave_in_block();
    if (g >= group_end) return;
    const u32 p = g * GROUP + lane;
    const bool valid = p < t.n;
    LaneQuery c{0.f, 0.f, 0.f, 0u};
    if (valid) c = lane_query<true>(t, QueryView{}, p);
    const float qx = c.x, qy = c.y, qz = c.z;
    const u32 row = c.row;
    float ux = 0.f, uy = 0.f, uz = 0.f, vx = 0.f, vy = 0.f, vz = 0.f;
    bool has_frame = false;
    if (valid) {
        const float nx = normals[3ull * row], ny = normals[3ull * row + 1], nz = normals[3ull * row + 2];
        const float ax = __builtin_fabsf(nx), ay = __builtin_fabsf(ny), az = __builtin_fabsf(nz);
        has_frame = __builtin_isfinite(nx) && __builtin_isfinite(ny) && __builtin_isfinite(nz) && !(nx == 0.f && ny == 0.f && nz == 0.f);
        if (has_frame) {
            if (ax <= ay && ax <= az) ux = 0.f, uy = -nz, uz = ny;
            else if (ay <= az) ux = -nz, uy = 0.f, uz = nx;
            else ux = -ny, uy = nx, uz = 0.f;
            vx = ny * uz - nz * uy;
            vy = nz * ux - nx * uz;
            vz = nx * uy - ny * ux;
        }
    }
    const float r2 = valid ? radius * radius : -1.f;  // sphere.hpp:34 radius * radius in float; -1: idle lane
    u32 cnt = 0, lo = 0, hi = 0;
    auto need = [&](const NodeBox& b) { return box_d2(b, qx, qy, qz) <= r2; };
    walk_needed_leaves<false>(t, need, [&](const u32, const Leaf* record, u64, u32) {
        const Leaf lf = load_const(record);
#pragma unroll
        for (int j = 0; j < LEAF; ++j) {
            const float dx = lf.x[j] - qx, dy = lf.y[j] - qy, dz = lf.z[j] - qz;
            if (sq3(dx, dy, dz) <= r2) {  // (a NaN padding point fails)
                cnt += 1u;
                const float a = (dx * ux + dy * uy) + dz * uz, b = (dx * vx + dy * vy) + dz * vz;
                if (!(a == 0.f && b == 0.f)) {
                    const u32 s = sector_of(a, b);
                    const u32 bit = 1u << (s & 31u);  // (by word: a 32-bit shift never reaches the upper one)
                    lo |= s < 32u ? bit : 0u;
                    hi |= s < 32u ? 0u : bit;
                }
            }
        }
    });
    if (!valid) return;
    const u64 mask = has_frame ? (static_cast<u64>(hi) << 32) | lo : 0ull;
    u32 gap = 255u, start = 255u;
    if (has_frame) longest_gap(mask, gap, start);
    out.keep[row] = has_frame && cnt >= at_least && gap >= gap_sectors ? 1 : 0;  // (no frame: 255 passes the last test alone)
    if (out.gap) {
        out.gap[2ull * row] = static_cast<uint8_t>(gap);
        out.gap[2ull * row + 1] = static_cast<uint8_t>(start);
    }
    if (out.count) out.count[row] = cnt;
    if (out.sectors) out.sectors[row] = mask;
}

int check_boundary(const char* what, const float* normals, float radius, u32 gap_sectors, u32 flags, const void* keep)
{
    if (flags & ~PCPX_BOUNDARY_ON_DEVICE) {
        set_error("%s: unknown flag bits 0x%x", what, flags);
        return PCPX_ERR_INVALID;
    }
    if (!(radius >= 0.f)) {  // (false for NaN)
        set_error("%s: the radius must be >= 0 (got %g)", what, static_cast<double>(radius));
        return PCPX_ERR_INVALID;
    }
    if (gap_sectors < 1u || gap_sectors > PCPX_BOUNDARY_SECTORS) {
        set_error("%s: gap_sectors must be 1 .. %u (got %u)", what, PCPX_BOUNDARY_SECTORS, gap_sectors);
        return PCPX_ERR_INVALID;
    }
    if (!normals) {
        set_error("%s: the normals array is NULL", what);
        return PCPX_ERR_INVALID;
    }
    if (!keep) {
        set_error("%s: the keep array is NULL", what);
        return PCPX_ERR_INVALID;
    }
    return PCPX_OK;
}

// Everything is enqueued on the handle's stream; the scratch (the scan's places and tile sums) is the handle's, one Carve ensured
// once before the first launch.  The rows of the points outside the voxel grid are filled before the walk, which writes every other.
int boundary_self(Index& ix, const float* d_normals, float radius, u32 gap_sectors, u32 min_neighbours, const BoundaryOut& o, u32* d_kept_rows,
                  u64* d_kept_count)
{
    int st;
    hipStream_t s = ix.stream;
    const u64 rows = ix.n_in, n = ix.n;
    if (rows == 0) {
        if (d_kept_count) PCPX_HIP(hipMemsetAsync(d_kept_count, 0, sizeof(u64), s));
        return PCPX_OK;
    }
    Carve c;
    const size_t place_at = c.take(rows * sizeof(u32)), sums_at = c.take((scan_tiles(rows) + 1ull) * sizeof(u32));
    if ((st = ensure_scratch(ix, c.bytes())) != PCPX_OK) return st;
    char* base = static_cast<char*>(ix.d_scratch);
    if (n != rows) {
        PCPX_HIP(hipMemsetAsync(o.keep, 0, rows * sizeof(uint8_t), s));
        if (o.gap) PCPX_HIP(hipMemsetAsync(o.gap, 0xFF, rows * 2 * sizeof(uint8_t), s));
        if (o.count) PCPX_HIP(hipMemsetAsync(o.count, 0, rows * sizeof(u32), s));
        if (o.sectors) PCPX_HIP(hipMemsetAsync(o.sectors, 0, rows * sizeof(u64), s));
    }
    if (n > 0) {
        const u64 groups = (n + GROUP - 1) / GROUP;
        k_boundary<<<grid_for_groups(groups), 64 * WAVES_PER_BLOCK, 0, s>>>(ix.view(), static_cast<u32>(groups), radius, d_normals, gap_sectors,
                                                                            min_neighbours > 1u ? min_neighbours : 1u, o);
        PCPX_HIP(hipGetLastError());
    }
    return count_and_compact_kept(o.keep, rows, reinterpret_cast<u32*>(base + place_at), reinterpret_cast<u32*>(base + sums_at), d_kept_rows,
                                  d_kept_count, s);
}

// One interval of the PCPX_K_RANGE family for the whole call: what the call launches through other modules books nothing of its own.
int booked_as_one_range_interval(Index& ix, const float* d_normals, float radius, u32 gap_sectors, u32 min_neighbours, const BoundaryOut& o,
                                 u32* d_kept_rows, u64* d_kept_count)
{
    ProfileScope prof(ix, PCPX_K_RANGE);
    const bool profiling = ix.profiling;
    ix.profiling = false;
    const int st = boundary_self(ix, d_normals, radius, gap_sectors, min_neighbours, o, d_kept_rows, d_kept_count);
    ix.profiling = profiling;
    return st;
}

}  // namespace

}  // namespace pcpx

using namespace pcpx;

extern "C" {

int pcpx_boundary_self(pcpx_index* h, const float* normals, float radius, uint32_t gap_sectors, uint32_t min_neighbours, uint32_t flags,
                       uint8_t* keep, uint32_t* opt_kept_rows, uint64_t* opt_kept_count, uint8_t* opt_gap, uint32_t* opt_count,
                       uint64_t* opt_sectors)
{
    static const char* what = "pcpx_boundary_self";
    if (flags & PCPX_BOUNDARY_ON_DEVICE) {
        return on_index(h, what, WHOLE_CLOUD, [&](Index* ix) -> int {
            if (const int st = check_boundary(what, normals, radius, gap_sectors, flags, keep)) return st;
            BoundaryOut o;
            o.keep = keep;
            o.gap = opt_gap;
            o.count = opt_count;
            o.sectors = opt_sectors;
            return booked_as_one_range_interval(*ix, normals, radius, gap_sectors, min_neighbours, o, opt_kept_rows, opt_kept_count);
        });
    }
    return on_index_host(h, what, WHOLE_CLOUD, [&](Index* ix, Staged& stage) -> int {
        int st;
        if ((st = check_boundary(what, normals, radius, gap_sectors, flags, keep)) != PCPX_OK) return st;
        if (opt_kept_count) *opt_kept_count = 0;
        const u64 rows = ix->n_in;
        if (rows == 0) return PCPX_OK;
        const float* dn = stage.upload(normals, rows * 3 * sizeof(float));
        BoundaryOut d;
        d.keep = stage.alloc<uint8_t>(rows * sizeof(uint8_t));
        d.gap = stage.alloc_for(opt_gap, rows * 2 * sizeof(uint8_t));
        d.count = stage.alloc_for(opt_count, rows * sizeof(u32));
        d.sectors = stage.alloc_for(opt_sectors, rows * sizeof(u64));
        u32* dr = stage.alloc_for(opt_kept_rows, rows * sizeof(u32));
        u64* dt = opt_kept_rows || opt_kept_count ? stage.alloc<u64>(sizeof(u64)) : nullptr;
        if ((st = stage.st) != PCPX_OK) return st;
        if ((st = booked_as_one_range_interval(*ix, dn, radius, gap_sectors, min_neighbours, d, dr, dt)) != PCPX_OK) return st;
        stage.download(keep, d.keep, rows * sizeof(uint8_t));
        stage.download_opt(opt_gap, d.gap, rows * 2 * sizeof(uint8_t));
        stage.download_opt(opt_count, d.count, rows * sizeof(u32));
        stage.download_opt(opt_sectors, d.sectors, rows * sizeof(u64));
        return download_kept(stage, dt, dr, opt_kept_count, opt_kept_rows);
    });
}

}  // extern "C"
