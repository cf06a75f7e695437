// pcpx_descriptors.hip -- the Fast Point Feature Histogram of the indexed cloud's points (include/pcpx_descriptors.h; DESIGN.md
// section 22).  The eighth and ninth forms of the leaf-direct sphere walk of pcpx_device.h:
//   k_spfh  a pair test against a partner whose coordinates and normal are scalars of two leaf records (k_segment_hook's shape);
//           the three bins of every pair go to 33 counters per lane in LDS;
//   k_fpfh  an accumulation over the sphere of a per-point record (k_range_moments' shape): the partner's 33-float SPFH record is
//           a scalar load, the lane's 33 sums are registers.
// A subset of rows is described by the same two kernels with the other lanes idle: k_fpfh_mark first walks the described points'
// spheres and marks the positions whose SPFH the second walk will read.
#include "pcpx_device.h"
#include "pcpx_stage.h"
#include "pcpx_descriptors.h"

namespace pcpx {

namespace {

constexpr u32 FP_BLOCK = 256;
constexpr int NB = PCPX_FPFH_BINS;   // bins per feature
constexpr int NF = PCPX_FPFH_SIZE;   // floats per descriptor
static_assert(NF == 3 * NB, "three features");

// The SPFH of one curve position: what k_spfh leaves for k_fpfh, 132 bytes per leaf slot.
struct Spfh {
    float v[NF];
};
static_assert(sizeof(Spfh) == 4 * NF, "SPFH record must be dense");

// One thread per leaf slot (npos = 8 nleaves of them): the point's normal from its input row into the leaf's normal record (zeros in
// a slot that holds no point: its coordinates are NaN and pass no distance test).  The subset form's words are preset here: nobody
// is described (k_fpfh_rows names those who are) and no SPFH is needed (k_fpfh_mark says which are).
__global__ __launch_bounds__(FP_BLOCK) void k_fpfh_prep(TreeView t, u32 npos, const float* __restrict__ normals, Normals8* __restrict__ nrec,
                                                        u32* __restrict__ opt_described, uint8_t* __restrict__ opt_needed)
{
    const u32 p = blockIdx.x * FP_BLOCK + threadIdx.x;
    if (p >= npos) return;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    if (p < t.n) {
        const u32 row = t.leaves[p / LEAF].id[p % LEAF];
        nx = normals[3ull * row], ny = normals[3ull * row + 1], nz = normals[3ull * row + 2];
    }
    Normals8& rec = nrec[p / LEAF];
    rec.x[p % LEAF] = nx, rec.y[p % LEAF] = ny, rec.z[p % LEAF] = nz;
    if (opt_described) opt_described[p] = INVALID_ID;
    if (opt_needed) opt_needed[p] = 0;
}

// Subset form, one thread per described row k: described[position of rows[k]] = k.  The rows are distinct, so no two threads write
// one word.  (A row that is >= n_in or outside the voxel grid keeps the zeros its output row was preset with.)
__global__ __launch_bounds__(FP_BLOCK) void k_fpfh_rows(const u32* __restrict__ rows, u32 m, u32 n_in, const u32* __restrict__ position_of,
                                                        u32* __restrict__ described)
{
    const u32 k = blockIdx.x * FP_BLOCK + threadIdx.x;
    if (k >= m) return;
    const u32 row = rows[k];
    if (row >= n_in) return;
    const u32 p = position_of[row];
    if (p != INVALID_ID) described[p] = k;
}

// Subset form: one lane per described point, the others idle (r2 = -1); a group with none returns after one load.  For every
// position that some lane has in its sphere, one lane stores needed = 1 (the eight positions of a leaf: lanes 0-7, one store).
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void k_fpfh_mark(TreeView t, u32 group_end, float radius, const u32* __restrict__ described,
                                                                   uint8_t* __restrict__ needed)
{
    const u32 lane = threadIdx.x & 63u;
    const u32 g = virtual_block() * WAVES_PER_BLOCK + wave_in_block();
    if (g >= group_end) return;
    const u32 p = g * GROUP + lane;
    const bool active = p < t.n && described[p] != INVALID_ID;
    if (!any_lane(active)) return;
    LaneQuery c{0.f, 0.f, 0.f, 0u};
    if (active) c = lane_query<true>(t, QueryView{}, p);
    const float qx = c.x, qy = c.y, qz = c.z;
    const float r2 = active ? radius * radius : -1.f;  // sphere.hpp:34 radius * radius in float; -1: idle lane
    auto need = [&](const NodeBox& b) { return box_d2(b, qx, qy, qz) <= r2; };
    walk_needed_leaves<false>(t, need, [&](const u32 leaf, const Leaf* record, u64, u32) {
        const Leaf lf = load_const(record);
        u32 inside = 0;  // bit j: some lane has point j of the leaf in its sphere
#pragma unroll
        for (int j = 0; j < LEAF; ++j) {
            const float dx = lf.x[j] - qx, dy = lf.y[j] - qy, dz = lf.z[j] - qz;
            if (any_lane(sq3(dx, dy, dz) <= r2)) inside |= 1u << j;  // (a NaN padding point fails)
        }
        if (lane < static_cast<u32>(LEAF) && ((inside >> lane) & 1u)) needed[leaf * LEAF + lane] = 1;
    });
}

// float32(cos, sin)(k pi / 11), k = 1, 3, 5, 7, 9 (pcpx_descriptors.h)
__device__ __forceinline__ u32 sector_steps(float x, float ay)
{
    constexpr float cs[5] = PCPX_FPFH_COS_INIT, sn[5] = PCPX_FPFH_SIN_INIT;
    u32 k = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) k += (cs[i] * ay - sn[i] * x >= 0.f) ? 1u : 0u;
    return k;
}
// trunc(min(max((f + 1) * 5.5, 0), 10)); f is not NaN
__device__ __forceinline__ u32 bin_of(float f)
{
    float u = (f + 1.f) * 5.5f;
    u = u < 0.f ? 0.f : u;
    u = u > 10.f ? 10.f : u;
    return static_cast<u32>(u);
}

// One wave per group of 64 curve-consecutive positions, one lane per point whose SPFH is wanted (every indexed point, or the marked
// ones).  The partner's point and normal are scalars of the two leaf records; only the lane's own point and normal are vector.  The 33
// counters of a lane are indexed by the bins, so they live in LDS: hist[bin][lane], the bank is the lane and every ds_add_u32 is
// conflict-free whatever the bins are.  The arithmetic of a pair is pcpx_descriptors.h's, line by line (contraction is off).
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void k_spfh(TreeView t, u32 group_end, float radius, const Normals8* __restrict__ nrec,
                                                              const uint8_t* __restrict__ opt_needed, Spfh* __restrict__ spfh_at,
                                                              float* __restrict__ opt_spfh_row, u32* __restrict__ opt_pairs_row)
{
    __shared__ u32 hist[WAVES_PER_BLOCK][NF][GROUP];
    const u32 lane = threadIdx.x & 63u;
    const u32 wave = wave_in_block();
    const u32 g = virtual_block() * WAVES_PER_BLOCK + wave;
    if (g >= group_end) return;
    const u32 p = g * GROUP + lane;
    bool active = p < t.n;
    if (opt_needed) active = active && opt_needed[p] != 0;
    if (!any_lane(active)) return;
    LaneQuery c{0.f, 0.f, 0.f, 0u};
    float nix = 0.f, niy = 0.f, niz = 0.f;
    if (active) {
        c = lane_query<true>(t, QueryView{}, p);
        const Normals8& own = nrec[p / LEAF];
        nix = own.x[p % LEAF], niy = own.y[p % LEAF], niz = own.z[p % LEAF];
    }
    const float qx = c.x, qy = c.y, qz = c.z;
    const float r2 = active ? radius * radius : -1.f;  // sphere.hpp:34 radius * radius in float; -1: idle lane
    u32(*h)[GROUP] = hist[wave];
#pragma unroll
    for (int b = 0; b < NF; ++b) h[b][lane] = 0;
    u32 pairs = 0;
    auto need = [&](const NodeBox& b) { return box_d2(b, qx, qy, qz) <= r2; };
    walk_needed_leaves<false>(t, need, [&](const u32 leaf, const Leaf* record, u64, u32) {
        const Leaf lf = load_const(record);
        const Normals8 ln = load_const(nrec + leaf);
#pragma unroll
        for (int j = 0; j < LEAF; ++j) {
            const float dx = lf.x[j] - qx, dy = lf.y[j] - qy, dz = lf.z[j] - qz;
            const float d2 = sq3(dx, dy, dz);
            if (!any_lane(d2 <= r2 && d2 > 0.f)) continue;  // (a NaN padding point fails; the lane's own point has d2 = 0)
            const float njx = ln.x[j], njy = ln.y[j], njz = ln.z[j];
            const float ai = nix * dx + niy * dy + niz * dz;
            const float aj = njx * dx + njy * dy + njz * dz;
            const bool swap = fabsf(ai) < fabsf(aj);
            const float ex = swap ? -dx : dx, ey = swap ? -dy : dy, ez = swap ? -dz : dz, a = swap ? -aj : ai;
            const float nsx = swap ? njx : nix, nsy = swap ? njy : niy, nsz = swap ? njz : niz;
            const float ntx = swap ? nix : njx, nty = swap ? niy : njy, ntz = swap ? niz : njz;
            const float f3 = __fdiv_rn(a, __fsqrt_rn(d2));
            const float vx = ey * nsz - ez * nsy, vy = ez * nsx - ex * nsz, vz = ex * nsy - ey * nsx;
            const float vv = vx * vx + vy * vy + vz * vz;
            const float vl = __fsqrt_rn(vv);
            const float f2 = __fdiv_rn(vx * ntx + vy * nty + vz * ntz, vl);
            const float wx = nsy * vz - nsz * vy, wy = nsz * vx - nsx * vz, wz = nsx * vy - nsy * vx;
            const float y = wx * ntx + wy * nty + wz * ntz;
            const float x = (nsx * ntx + nsy * nty + nsz * ntz) * vl;
            // (vv == 0 fails `vv > 0`, and so does a NaN vv; the four tests below are false for a NaN)
            if (d2 <= r2 && d2 > 0.f && vv > 0.f && f3 == f3 && f2 == f2 && x == x && y == y) {
                const u32 k = sector_steps(x, fabsf(y));
                const u32 b1 = y >= 0.f ? 5u + k : 5u - k;
                const u32 b2 = NB + bin_of(f2), b3 = 2 * NB + bin_of(f3);
                __hip_atomic_fetch_add(&h[b1][lane], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                __hip_atomic_fetch_add(&h[b2][lane], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                __hip_atomic_fetch_add(&h[b3][lane], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                pairs += 1u;
            }
        }
    });
    if (!active) return;
    const float fpairs = static_cast<float>(pairs);
    Spfh& mine = spfh_at[p];
    float* by_row = opt_spfh_row ? opt_spfh_row + static_cast<u64>(c.row) * NF : nullptr;
#pragma unroll
    for (int b = 0; b < NF; ++b) {
        const float v = pairs ? __fdiv_rn(100.f * static_cast<float>(h[b][lane]), fpairs) : 0.f;
        mine.v[b] = v;
        if (by_row) by_row[b] = v;
    }
    if (opt_pairs_row) opt_pairs_row[c.row] = pairs;
}

// One lane per described point (every indexed point, or those k_fpfh_rows named; the others idle with r2 = -1).  The partner's
// coordinates and its SPFH record are scalar loads -- the record only where some lane has the partner in its sphere -- and the
// lane's 33 sums are registers, each += spfh_j[b] * w with the lane's own w = 1 / d2, or 0 where the partner is outside its sphere
// or at distance 0: the records are finite and the sums never negative, so a term of +0 leaves every bit of a sum as it was, and a
// lane's sums do not depend on which other lanes are active.  No LDS, no atomics, nothing between workgroups.
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void k_fpfh(TreeView t, u32 group_end, float radius, const Spfh* __restrict__ spfh_at,
                                                              const u32* __restrict__ opt_described, float* __restrict__ fpfh)
{
    const u32 lane = threadIdx.x & 63u;
    const u32 g = virtual_block() * WAVES_PER_BLOCK + wave_in_block();
    if (g >= group_end) return;
    const u32 p = g * GROUP + lane;
    bool active = p < t.n;
    u32 out_row = INVALID_ID;
    if (opt_described) {
        if (active) out_row = opt_described[p];
        active = out_row != INVALID_ID;
    }
    if (!any_lane(active)) return;
    LaneQuery c{0.f, 0.f, 0.f, 0u};
    if (active) c = lane_query<true>(t, QueryView{}, p);
    if (!opt_described) out_row = c.row;
    const float qx = c.x, qy = c.y, qz = c.z;
    const float r2 = active ? radius * radius : -1.f;  // sphere.hpp:34 radius * radius in float; -1: idle lane
    float acc[NF];
#pragma unroll
    for (int b = 0; b < NF; ++b) acc[b] = 0.f;
    auto need = [&](const NodeBox& b) { return box_d2(b, qx, qy, qz) <= r2; };
    walk_needed_leaves<false>(t, need, [&](const u32 leaf, const Leaf* record, u64, u32) {
        const Leaf lf = load_const(record);
#pragma unroll
        for (int j = 0; j < LEAF; ++j) {
            const float dx = lf.x[j] - qx, dy = lf.y[j] - qy, dz = lf.z[j] - qz;
            const float d2 = sq3(dx, dy, dz);
            const bool in = d2 <= r2 && d2 > 0.f;  // (a NaN padding point fails)
            if (!any_lane(in)) continue;
            const Spfh rec = load_const(spfh_at + (static_cast<u64>(leaf) * LEAF + j));
            const float w = in ? __fdiv_rn(1.f, d2) : 0.f;
#pragma unroll
            for (int b = 0; b < NF; ++b) acc[b] += rec.v[b] * w;
        }
    });
    if (!active) return;
    float* out = fpfh + static_cast<u64>(out_row) * NF;
#pragma unroll
    for (int f = 0; f < 3; ++f) {
        float sum = 0.f;
#pragma unroll
        for (int b = 0; b < NB; ++b) sum += acc[f * NB + b];
        const float scale = sum > 0.f ? __fdiv_rn(100.f, sum) : 0.f;
#pragma unroll
        for (int b = 0; b < NB; ++b) out[f * NB + b] = acc[f * NB + b] * scale;
    }
}

int check_fpfh_args(const char* what, const void* normals, float radius, const void* rows, u64 m, u32 flags, const void* fpfh)
{
    if (const int st = check_radius(what, radius)) return st;
    if (flags != 0u) {
        set_error("%s: unknown flag bits 0x%x", what, flags);
        return PCPX_ERR_INVALID;
    }
    if (!normals) {
        set_error("%s: the normal array is NULL", what);
        return PCPX_ERR_INVALID;
    }
    if (!fpfh) {
        set_error("%s: the fpfh array is NULL", what);
        return PCPX_ERR_INVALID;
    }
    if (!rows && m != 0) {
        set_error("%s: the rows array is NULL with m = %llu", what, static_cast<unsigned long long>(m));
        return PCPX_ERR_INVALID;
    }
    if (m > 0xFFFFFFFFull) {
        set_error("%s: m = %llu distinct rows cannot be", what, static_cast<unsigned long long>(m));
        return PCPX_ERR_INVALID;
    }
    return PCPX_OK;
}

// Everything is enqueued on the handle's stream, no synchronisation.  Scratch of the handle: the SPFH records (one per leaf slot), the
// normal records, and for a subset the described words and needed bytes (one per leaf slot) and position_of (one word per input row).
// subset: d_rows[0 .. m) are described (m = 0: nobody), else every input row.
int fpfh_self(Index& ix, const float* d_normals, float radius, bool subset, const u32* d_rows, u64 m, float* d_fpfh, float* d_spfh, u32* d_pairs)
{
    int st;
    hipStream_t s = ix.stream;
    const u64 rows = ix.n_in, n = ix.n;
    const u64 out_rows = subset ? m : rows;
    // the rows that no walk writes: all of a subset's until their lanes have run, and those of the points outside the voxel grid
    if (out_rows && (subset || n != rows)) PCPX_HIP(hipMemsetAsync(d_fpfh, 0, out_rows * NF * sizeof(float), s));
    if (rows && (subset || n != rows)) {
        if (d_spfh) PCPX_HIP(hipMemsetAsync(d_spfh, 0, rows * NF * sizeof(float), s));
        if (d_pairs) PCPX_HIP(hipMemsetAsync(d_pairs, 0, rows * sizeof(u32), s));
    }
    if (n == 0 || out_rows == 0) return PCPX_OK;
    const u64 npos = static_cast<u64>(ix.nleaves) * LEAF;  // >= n
    Carve c;
    const size_t spfh_off = c.take(npos * sizeof(Spfh)), nrec_off = c.take(ix.nleaves * sizeof(Normals8));
    const size_t described_off = subset ? c.take(npos * sizeof(u32)) : 0, needed_off = subset ? c.take(npos) : 0,
                 pos_of_off = subset ? c.take(rows * sizeof(u32)) : 0;
    if ((st = ensure_scratch(ix, c.bytes())) != PCPX_OK) return st;
    char* base = static_cast<char*>(ix.d_scratch);
    Spfh* spfh_at = reinterpret_cast<Spfh*>(base + spfh_off);
    Normals8* nrec = reinterpret_cast<Normals8*>(base + nrec_off);
    u32* described = subset ? reinterpret_cast<u32*>(base + described_off) : nullptr;
    uint8_t* needed = subset ? reinterpret_cast<uint8_t*>(base + needed_off) : nullptr;
    u32* position_of = subset ? reinterpret_cast<u32*>(base + pos_of_off) : nullptr;
    const TreeView t = ix.view();
    const u32 groups = static_cast<u32>((n + GROUP - 1) / GROUP);
    const u32 grid = grid_for_groups(groups);
    k_fpfh_prep<<<blocks_of(npos, FP_BLOCK), FP_BLOCK, 0, s>>>(t, static_cast<u32>(npos), d_normals, nrec, described, needed);
    if (subset) {
        PCPX_HIP(hipMemsetAsync(position_of, 0xFF, rows * sizeof(u32), s));
        if ((st = launch_invert_perm(ix.d_perm, n, position_of, s)) != PCPX_OK) return st;
        k_fpfh_rows<<<blocks_of(m, FP_BLOCK), FP_BLOCK, 0, s>>>(d_rows, static_cast<u32>(m), static_cast<u32>(rows), position_of, described);
        k_fpfh_mark<<<grid, 64 * WAVES_PER_BLOCK, 0, s>>>(t, groups, radius, described, needed);
    }
    k_spfh<<<grid, 64 * WAVES_PER_BLOCK, 0, s>>>(t, groups, radius, nrec, needed, spfh_at, d_spfh, d_pairs);
    k_fpfh<<<grid, 64 * WAVES_PER_BLOCK, 0, s>>>(t, groups, radius, spfh_at, described, d_fpfh);
    PCPX_HIP(hipGetLastError());
    return PCPX_OK;
}

}  // namespace

}  // namespace pcpx

using namespace pcpx;

extern "C" {

int pcpx_fpfh_self_dev(pcpx_index* h, const float* d_normals, float radius, const uint32_t* d_opt_rows, uint64_t m, uint32_t flags,
                       float* d_fpfh, float* d_opt_spfh, uint32_t* d_opt_pairs)
{
    static const char* what = "pcpx_fpfh_self_dev";
    return on_index(h, what, WHOLE_CLOUD, [&](Index* ix) -> int {
        int st;
        if ((st = check_fpfh_args(what, d_normals, radius, d_opt_rows, m, flags, d_fpfh)) != PCPX_OK) return st;
        ProfileScope prof(*ix, PCPX_K_RANGE);
        return fpfh_self(*ix, d_normals, radius, d_opt_rows != nullptr, d_opt_rows, m, d_fpfh, d_opt_spfh, d_opt_pairs);
    });
}

int pcpx_fpfh_self(pcpx_index* h, const float* normals, float radius, const uint32_t* opt_rows, uint64_t m, uint32_t flags, float* fpfh,
                   float* opt_spfh, uint32_t* opt_pairs)
{
    static const char* what = "pcpx_fpfh_self";
    return on_index_host(h, what, WHOLE_CLOUD, [&](Index* ix, Staged& stage) -> int {
        int st;
        if ((st = check_fpfh_args(what, normals, radius, opt_rows, m, flags, fpfh)) != PCPX_OK) return st;
        const u64 rows = ix->n_in, out_rows = opt_rows ? m : rows;
        if (rows == 0) {  // (every entry of a subset is >= n_in)
            if (out_rows) std::memset(fpfh, 0, out_rows * NF * sizeof(float));
            return PCPX_OK;
        }
        const float* dn = stage.upload(normals, rows * 3 * sizeof(float));
        const u32* dr = stage.upload(opt_rows, m * sizeof(u32));  // (null for m = 0)
        float* df = stage.alloc<float>(out_rows * NF * sizeof(float));
        float* ds = stage.alloc_for(opt_spfh, rows * NF * sizeof(float));
        u32* dp = stage.alloc_for(opt_pairs, rows * sizeof(u32));
        if ((st = stage.st) != PCPX_OK) return st;
        {
            ProfileScope prof(*ix, PCPX_K_RANGE);
            if ((st = fpfh_self(*ix, dn, radius, opt_rows != nullptr, dr, m, df, ds, dp)) != PCPX_OK) return st;
        }
        if (out_rows) stage.download(fpfh, df, out_rows * NF * sizeof(float));
        stage.download_opt(opt_spfh, ds, rows * NF * sizeof(float));
        stage.download_opt(opt_pairs, dp, rows * sizeof(u32));
        return stage.wait();
    });
}

}  // extern "C"
