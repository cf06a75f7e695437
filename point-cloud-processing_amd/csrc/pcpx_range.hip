// pcpx_range.hip -- radius search kernels (sphere and axis-aligned box ranges) for gfx950: the same wave-uniform
// walk as the kNN kernel (pcpx_device.h), one lane = one range, count, CSR fill or moments (normal, centroid, mean distance).
#include "pcpx_device.h"
#include "pcpx_eig3.h"
#include "pcpx_scan.h"

namespace pcpx {

namespace {

// A leaf that at most this many lanes need is looked at eight needing lanes x eight points at a time (packed_leaf below), in
// the count and the list form (lane-per-range leaves in the list form until round 4).  <= 32: one 512-B row of LDS per wave.
constexpr u32 PACKED_LEAVES = 16;
static_assert(PACKED_LEAVES <= 32, "one row of LDS per wave");
// Wave priority by phase, as in k_knn (pcpx_query.hip): the dense leaf's 88 vector instructions run at a lower priority than the walk
// and the packed leaves (2.238 -> 2.212 ms per 10 M counts; the dense leaf raised instead: 2.25)
constexpr int PRIO_BASE = 1, PRIO_DENSE = 0;

// ------------------------------------------------------------------------------------------------
// sphere range: count / fill (include/pcp/octree/linked_octree_node.hpp:581-614 semantics:
// every point with d2 <= r*r, query included)
// ------------------------------------------------------------------------------------------------
// One group of 64 curve-consecutive queries, one per lane: the wave-uniform walk of pcpx_device.h, a leaf's 8 points
// broadcast from SGPRs, the count kept per lane (compare + add-with-carry: 2 VALU per candidate on top of the 8 of the
// distance -- an exec-masked form would not be shorter).  The kernel sits on both issue pipes, so what pays is what takes
// instructions off both: a last-level node looks at its own leaves (no push and pop), and a leaf that few lanes need is
// counted eight needing lanes x eight points at a time (count form: packed_leaf below; the fill form keeps the lane-per-range
// leaf).  10 M counts at r = 0.01: 2.56 ms (round 3 start) -> 2.40 (direct leaves + round 3's point-per-lane form) -> 2.21
// (round 4: the packed form instead; profiles/experiments/README.md).
//
// MOM (moments form): 1 = per lane the count n, S = sum d and Q = sum d d^T of d = p - q (q: the sphere's
// centre), then centroid q + S / n and the PCA normal of C = Q - S S^T / n (eig3_smallest, as k_knn and k_normals); 2 = also
// D = sum |d| for the mean distance D / n; 3 = the moments of 1 and the shape features of C: its three
// eigenvalues, the surface variation and the principal axis beside the normal, out of the one solve.  Lane-per-range leaves only
// (a packed leaf would need a cross-lane sum of ~11 values).
struct FeaturesOut {
    float* evals = nullptr;      // rows x 3, ascending
    float* curvature = nullptr;  // rows: max(l0, 0) / ((l0 + l1) + l2)
    float* normals = nullptr;    // rows x 3
    float* axes = nullptr;       // rows x 3
    u32* count = nullptr;        // rows
};
// what the features form writes for an empty neighbourhood (C = 0), and what its epilogue writes from C and n
__device__ __forceinline__ void write_features(const FeaturesOut& fo, const u64 row, const u32 cnt, float c00, float c10, float c20, float c11,
                                               float c21, float c22)
{
    if (fo.evals || fo.curvature || fo.normals || fo.axes) {
        float nrm[3], ev[3], ax[3];
        eig3_smallest<true>(c00, c10, c20, c11, c21, c22, nrm, ev, ax);
        const u64 r3 = 3ull * row;
        if (fo.evals) {
            fo.evals[r3] = ev[0];
            fo.evals[r3 + 1] = ev[1];
            fo.evals[r3 + 2] = ev[2];
        }
        if (fo.curvature) {
            const float sum = (ev[0] + ev[1]) + ev[2];
            float sv = sum > 0.f ? fmaxf(ev[0], 0.f) / sum : 0.f;  // (n = 1, copies of one point: C = 0)
            if (cnt == 0u) sv = __builtin_nanf("");
            fo.curvature[row] = sv;
        }
        if (fo.normals) {
            fo.normals[r3] = nrm[0];
            fo.normals[r3 + 1] = nrm[1];
            fo.normals[r3 + 2] = nrm[2];
        }
        if (fo.axes) {
            fo.axes[r3] = ax[0];
            fo.axes[r3 + 1] = ax[1];
            fo.axes[r3 + 2] = ax[2];
        }
    }
    if (fo.count) fo.count[row] = cnt;
}
struct MomentsOut {
    float* normals = nullptr;    // rows x 3
    float* centroids = nullptr;  // rows x 3
    float* mean_dist = nullptr;  // rows
    u32* count = nullptr;        // rows
};

// AT_LEAST (the outlier filters of pcpx_outliers.hip; count form only): the caller asks only whether the sphere holds `at_least`
// points.  A lane whose count has reached the bound stops needing nodes: its r^2 becomes the idle lane's -1, so it passes no further
// distance test, asks for no further box and publishes -1 in the packed leaves it was already booked for.  A lane that never
// reaches the bound has walked its whole sphere.  It writes keep = count >= at_least by input row and no count.
template <bool SELF, bool FILL, int MOM = 0, bool AT_LEAST = false>
__device__ __forceinline__ void range_group(const TreeView& t, const QueryView& qv, const u32 g, const float radius,
                                            const float* __restrict__ radii, u32* __restrict__ out_cnt,
                                            const u64* __restrict__ offsets, u32* __restrict__ out_idx, float4* __restrict__ pub,
                                            const u32 lane, const MomentsOut mo = MomentsOut{}, const FeaturesOut fo = FeaturesOut{},
                                            const u32 at_least = 0u, uint8_t* __restrict__ keep_out = nullptr)
{
    static_assert(MOM == 0 || !FILL, "the moments form lists nothing");
    static_assert(!AT_LEAST || (MOM == 0 && !FILL), "the at-least form is a count form");
    const u32 p = g * GROUP + lane;
    const u32 nq = SELF ? t.n : qv.nq;
    const bool valid = p < nq && (!SELF || p - qv.pos_lo < qv.pos_hi - qv.pos_lo);  // (self ranges: only the asked positions)
    LaneQuery q{0.f, 0.f, 0.f, 0u};
    if (valid) q = lane_query<SELF>(t, qv, p);
    const float qx = q.x, qy = q.y, qz = q.z;
    const u32 row = q.row;
    float r = radius;
    if (radii && valid) r = radii[row];
    float r2 = valid ? r * r : -1.f;  // sphere.hpp:34 radius * radius in float; -1: idle lane (only the at-least form writes it again)
    __builtin_amdgcn_s_setprio(PRIO_BASE);
    u32 cnt = 0;
    u64 wpos = (FILL && valid) ? offsets[row] : 0;
    auto need = [&](const NodeBox& b) { return box_d2(b, qx, qy, qz) <= r2; };
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, q00 = 0.f, q10 = 0.f, q11 = 0.f, q20 = 0.f, q21 = 0.f, q22 = 0.f, dsum = 0.f;  // (moments form)

    auto leaf_record_points = [&](const Leaf& lf) {
        if constexpr (MOM != 0) {
#pragma unroll
            for (int j = 0; j < LEAF; ++j) {
                const float dx = lf.x[j] - qx, dy = lf.y[j] - qy, dz = lf.z[j] - qz;
                const float d2 = sq3(dx, dy, dz);
                if (d2 <= r2) {  // (a NaN padding point fails)
                    cnt += 1u;
                    s0 += dx; s1 += dy; s2 += dz;
                    q00 += dx * dx; q10 += dy * dx; q11 += dy * dy;
                    q20 += dz * dx; q21 += dz * dy; q22 += dz * dz;
                    if (MOM == 2) dsum += sqrtf(d2);
                }
            }
            return;
        }
        if (!FILL) {
            __builtin_amdgcn_s_setprio(PRIO_DENSE);
            // count: the eight "inside" masks first (a scalar register pair each), then eight add-with-carry -- from
            // `cnt += in` hipcc pairs the points up as compare, select 0/1 under VCC, compare, add-with-carry, and the select
            // under a VCC that a compare has just written issues in 23 cycles on gfx950 (profiles/r03_valu_issue_rates.txt)
            u64 inside[LEAF];
#pragma unroll
            for (int j = 0; j < LEAF; ++j) {
                float dx = lf.x[j] - qx, dy = lf.y[j] - qy, dz = lf.z[j] - qz;
                inside[j] = __builtin_amdgcn_ballot_w64(sq3(dx, dy, dz) <= r2);
            }
            static_assert(LEAF == 8, "eight masks");
            u64 carry_out;  // (one statement: between two that pass a register on hipcc puts an s_nop)
            asm("v_addc_co_u32_e64 %0, %1, %0, 0, %2\n\tv_addc_co_u32_e64 %0, %1, %0, 0, %3\n\t"
                "v_addc_co_u32_e64 %0, %1, %0, 0, %4\n\tv_addc_co_u32_e64 %0, %1, %0, 0, %5\n\t"
                "v_addc_co_u32_e64 %0, %1, %0, 0, %6\n\tv_addc_co_u32_e64 %0, %1, %0, 0, %7\n\t"
                "v_addc_co_u32_e64 %0, %1, %0, 0, %8\n\tv_addc_co_u32_e64 %0, %1, %0, 0, %9"
                : "+v"(cnt), "=&s"(carry_out)
                : "s"(inside[0]), "s"(inside[1]), "s"(inside[2]), "s"(inside[3]), "s"(inside[4]), "s"(inside[5]), "s"(inside[6]),
                  "s"(inside[7]));
            __builtin_amdgcn_s_setprio(PRIO_BASE);
            if constexpr (AT_LEAST) {
                if (cnt >= at_least) r2 = -1.f;
            }
            return;
        }
#pragma unroll
        for (int j = 0; j < LEAF; ++j) {
            float dx = lf.x[j] - qx, dy = lf.y[j] - qy, dz = lf.z[j] - qz;
            bool in = sq3(dx, dy, dz) <= r2;
            if (in) out_idx[wpos + cnt] = lf.id[j];
            cnt += in ? 1u : 0u;
        }
    };
    // A leaf that at most PACKED_LEAVES lanes need is counted EIGHT NEEDING LANES x EIGHT POINTS at a time (k_knn's
    // packed_leaf, pcpx_query.hip): the needing lanes publish {centre, r^2} in LDS in the order of their rank among the needing
    // lanes, lane 8 i + j forms the distance from the i-th published centre to point j, and a needing lane adds the number of set
    // bits of its own byte of the step's ballot -- ~12 vector instructions per eight needing lanes (+ 8 per leaf) against 88 per
    // leaf in the lane-per-range form.  Same arithmetic (d = p - c, three roundings; sphere.hpp:27-35).  A slot that holds no
    // centre holds r^2 = -1 (k_range sets the row so, a needing lane sets its slot back): the lanes of a step beyond the leaf's
    // needing lanes count nothing, without a lane mask per step (the scalar unit is as loaded as the vector units here).
    // The list form (round 5) does the same: the needing lanes also publish where their list stands (offset + what they have so far),
    // and a lane whose point is inside writes the point's index at that place plus the number of set bits below its own in its
    // group's byte of the step's ballot -- the order of a list is the order of the lane-per-range form: walk order, then point
    // order inside a leaf.
    constexpr bool packed_leaves = MOM == 0;
    auto packed_leaf = [&](const Leaf* record, const u64 who, const u32 how_many) {
        u32 lane_here = lane;
        asm volatile("" : "+v"(lane_here));  // (or what depends on the lane alone is kept in registers for the whole walk)
        const u32 j = lane_here & 7u, i = lane_here >> 3;
        const float* rec = reinterpret_cast<const float*>(record);
        const float cx = rec[j], cy = rec[LEAF + j], cz = rec[2 * LEAF + j];
        u32 idj = 0;
        if (FILL) idj = reinterpret_cast<const u32*>(record)[3 * LEAF + j];
        u64* const pub_at = reinterpret_cast<u64*>(pub + 32);  // (list form: the row's second part)
        const u32 rank = __builtin_amdgcn_mbcnt_hi(static_cast<u32>(who >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<u32>(who), 0u));
        const bool mine = __builtin_amdgcn_inverse_ballot_w64(who);
        if (mine) {
            pub[rank] = make_float4(qx, qy, qz, r2);
            if (FILL) pub_at[rank] = wpos + cnt;
        }
        __builtin_amdgcn_wave_barrier();  // (one wave: its LDS operations complete in order; this only pins the compiler's order)
        const u32 my_byte = (rank & 7u) << 3;
        for (u32 s = 0; s < how_many; s += 8u) {
            const float4 q = pub[s + i];
            const float dx = cx - q.x, dy = cy - q.y, dz = cz - q.z;
            const bool in_here = sq3(dx, dy, dz) <= q.w;  // (a NaN padding point fails; so does every point against an empty slot)
            const u64 inside = __builtin_amdgcn_ballot_w64(in_here);
            if (FILL && in_here) {
                const u32 group_byte = static_cast<u32>(inside >> (lane_here & 56u)) & 0xFFu;  // the eight points against published range s + i
                out_idx[pub_at[s + i] + static_cast<u32>(__builtin_popcount(group_byte & ((1u << j) - 1u)))] = idj;
            }
            if (mine && rank - s < 8u) cnt += static_cast<u32>(__builtin_popcount(static_cast<u32>(inside >> my_byte) & 0xFFu));
        }
        __builtin_amdgcn_wave_barrier();
        if (mine) reinterpret_cast<float*>(pub + rank)[3] = -1.f;
        __builtin_amdgcn_wave_barrier();
        if constexpr (AT_LEAST) {
            if (cnt >= at_least) r2 = -1.f;
        }
    };
    walk_needed_leaves<packed_leaves>(t, need, [&](const u32, const Leaf* record, const u64 who, const u32 how_many) {
        if (packed_leaves && how_many <= PACKED_LEAVES) packed_leaf(record, who, how_many);
        else leaf_record_points(load_const(record));
    });
    if constexpr (MOM != 0) {
        if (!valid) return;
        // epilogue: C = Q - S (S / n); n = 0 (an empty sphere) gives C = 0 -- the reference's empty scatter matrix -- and NaN for
        // the centroid and the mean distance (0 / 0), as pcp::estimate_normal and average_distances_to_neighbors do
        const float fn = static_cast<float>(cnt);
        const float m0 = s0 / fn, m1 = s1 / fn, m2 = s2 / fn;
        if constexpr (MOM == 3) {
            const bool any = cnt != 0u;
            const float c00 = any ? q00 - s0 * m0 : 0.f, c10 = any ? q10 - s1 * m0 : 0.f, c11 = any ? q11 - s1 * m1 : 0.f;
            const float c20 = any ? q20 - s2 * m0 : 0.f, c21 = any ? q21 - s2 * m1 : 0.f, c22 = any ? q22 - s2 * m2 : 0.f;
            write_features(fo, row, cnt, c00, c10, c20, c11, c21, c22);
            return;
        }
        const u64 r3 = 3ull * row;
        if (mo.normals) {
            const bool any = cnt != 0u;
            const float c00 = any ? q00 - s0 * m0 : 0.f, c10 = any ? q10 - s1 * m0 : 0.f, c11 = any ? q11 - s1 * m1 : 0.f;
            const float c20 = any ? q20 - s2 * m0 : 0.f, c21 = any ? q21 - s2 * m1 : 0.f, c22 = any ? q22 - s2 * m2 : 0.f;
            float nrm[3], ev[3];
            eig3_smallest(c00, c10, c20, c11, c21, c22, nrm, ev);
            mo.normals[r3] = nrm[0];
            mo.normals[r3 + 1] = nrm[1];
            mo.normals[r3 + 2] = nrm[2];
        }
        if (mo.centroids) {
            mo.centroids[r3] = qx + m0;
            mo.centroids[r3 + 1] = qy + m1;
            mo.centroids[r3 + 2] = qz + m2;
        }
        if (MOM == 2 && mo.mean_dist) mo.mean_dist[row] = dsum / fn;
        if (mo.count) mo.count[row] = cnt;
    } else if constexpr (AT_LEAST) {
        if (valid) keep_out[row] = cnt >= at_least ? 1 : 0;
    } else {
        if (valid && !FILL) out_cnt[(SELF && qv.by_position) ? p + qv.pos_bias : row] = cnt;
    }
}

// One single-wave workgroup per group, XCD-aware block order (pcpx_device.h: virtual_block).  (Tried: a persistent grid
// pulling groups from the 8 work queues like k_knn -- 10 M counts at r = 0.01 went from 2.8 to 3.1 ms: these groups are
// short and even, the dispatcher is the better scheduler here.)
template <bool SELF, bool FILL>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void k_range(TreeView t, QueryView qv, u32 group_first, u32 group_end, float radius,
                                                               const float* __restrict__ radii, u32* __restrict__ out_cnt,
                                                               const u64* __restrict__ offsets, u32* __restrict__ out_idx)
{
    __shared__ float4 published[WAVES_PER_BLOCK][FILL ? 48 : 32];  // packed_leaf's row, one per wave (list form: + 32 list positions)
    const u32 lane = threadIdx.x & 63u;
    const u32 g = group_first + virtual_block() * WAVES_PER_BLOCK + wave_in_block();
    if (g >= group_end) return;
    if (lane < 32u) published[wave_in_block()][lane].w = -1.f;  // packed_leaf's invariant: a slot that holds no centre holds r^2 = -1
    range_group<SELF, FILL>(t, qv, g, radius, radii, out_cnt, offsets, out_idx, published[wave_in_block()], lane);
}

// k_range<true, false> with the one radius of the launch a float in device memory (the density filter of pcpx_outliers.hip, whose
// radius an earlier kernel on the stream has left there): one uniform scalar load per wave, then the same group walk, so the same
// bits.  A NaN radius gives r^2 = NaN: no box is needed, no point is inside, every count is 0.
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void k_range_radius_at(TreeView t, QueryView qv, u32 group_first, u32 group_end,
                                                                         const float* __restrict__ radius_at, u32* __restrict__ out_cnt)
{
    __shared__ float4 published[WAVES_PER_BLOCK][32];
    const u32 lane = threadIdx.x & 63u;
    const u32 g = group_first + virtual_block() * WAVES_PER_BLOCK + wave_in_block();
    if (g >= group_end) return;
    if (lane < 32u) published[wave_in_block()][lane].w = -1.f;
    const float radius = load_const(radius_at);
    range_group<true, false>(t, qv, g, radius, nullptr, out_cnt, nullptr, nullptr, published[wave_in_block()], lane);
}

// The at-least form of the self count walk: keep = the sphere holds at_least (>= 1) points, by input row.  The one radius of the
// launch is `radius`, or the float at radius_at when that is not null.
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void k_range_at_least(TreeView t, QueryView qv, u32 group_first, u32 group_end, float radius,
                                                                        const float* __restrict__ radius_at, u32 at_least,
                                                                        uint8_t* __restrict__ keep)
{
    __shared__ float4 published[WAVES_PER_BLOCK][32];
    const u32 lane = threadIdx.x & 63u;
    const u32 g = group_first + virtual_block() * WAVES_PER_BLOCK + wave_in_block();
    if (g >= group_end) return;
    if (lane < 32u) published[wave_in_block()][lane].w = -1.f;
    if (radius_at) radius = load_const(radius_at);
    range_group<true, false, 0, true>(t, qv, g, radius, nullptr, nullptr, nullptr, nullptr, published[wave_in_block()], lane, MomentsOut{},
                                      FeaturesOut{}, at_least, keep);
}

// The moments form: one lane per sphere as k_range, no LDS (lane-per-range leaves); outputs by input row (self) or query row (batch)
template <bool SELF, int MOM>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void k_range_moments(TreeView t, QueryView qv, u32 group_first, u32 group_end, float radius,
                                                                       const float* __restrict__ radii, MomentsOut mo)
{
    const u32 lane = threadIdx.x & 63u;
    const u32 g = group_first + virtual_block() * WAVES_PER_BLOCK + wave_in_block();
    if (g >= group_end) return;
    range_group<SELF, false, MOM>(t, qv, g, radius, radii, nullptr, nullptr, nullptr, nullptr, lane, mo);
}

// the empty-set values at the rows of the points that are not indexed (position_of = 0xFFFFFFFF: outside the voxel grid)
__global__ __launch_bounds__(256) void k_range_moments_empty_rows(const u32* __restrict__ pos_of, u64 n_rows, MomentsOut mo)
{
    const u64 i = blockIdx.x * static_cast<u64>(blockDim.x) + threadIdx.x;
    if (i >= n_rows || pos_of[i] != 0xFFFFFFFFu) return;
    const float nan = __builtin_nanf("");
    if (mo.normals) {
        float nrm[3], ev[3];
        eig3_smallest(0.f, 0.f, 0.f, 0.f, 0.f, 0.f, nrm, ev);  // (what the epilogue gives for n = 0)
        mo.normals[3 * i] = nrm[0];
        mo.normals[3 * i + 1] = nrm[1];
        mo.normals[3 * i + 2] = nrm[2];
    }
    if (mo.centroids) {
        mo.centroids[3 * i] = nan;
        mo.centroids[3 * i + 1] = nan;
        mo.centroids[3 * i + 2] = nan;
    }
    if (mo.mean_dist) mo.mean_dist[i] = nan;
    if (mo.count) mo.count[i] = 0u;
}

// The features form: the walk and the moments of k_range_moments<SELF, 1>, the epilogue's one solve giving the
// eigenvalues, the surface variation and the principal axis beside the normal
template <bool SELF>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void k_range_features(TreeView t, QueryView qv, u32 group_first, u32 group_end, float radius,
                                                                        const float* __restrict__ radii, FeaturesOut fo)
{
    const u32 lane = threadIdx.x & 63u;
    const u32 g = group_first + virtual_block() * WAVES_PER_BLOCK + wave_in_block();
    if (g >= group_end) return;
    range_group<SELF, false, 3>(t, qv, g, radius, radii, nullptr, nullptr, nullptr, nullptr, lane, MomentsOut{}, fo);
}

// the empty-set values at the rows of the points that are not indexed, as k_range_moments_empty_rows
__global__ __launch_bounds__(256) void k_range_features_empty_rows(const u32* __restrict__ pos_of, u64 n_rows, FeaturesOut fo)
{
    const u64 i = blockIdx.x * static_cast<u64>(blockDim.x) + threadIdx.x;
    if (i >= n_rows || pos_of[i] != 0xFFFFFFFFu) return;
    write_features(fo, i, 0u, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f);  // (what the epilogue gives for n = 0)
}

// AABB ranges: one wave per 64 boxes, no spatial coherence assumed (boxes are few in practice:
// test/octree/octree_range_search.cpp:80-118).  contains() is inclusive
// (axis_aligned_bounding_box.hpp:111-125); prune = box/box overlap (intersections.hpp:25-32).
template <bool FILL>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void k_range_aabb(TreeView t, const float* __restrict__ boxes6, u32 nb,
                                                    u32* __restrict__ out_cnt, const u64* __restrict__ offsets,
                                                    u32* __restrict__ out_idx)
{
    const u32 lane = threadIdx.x & 63u;
    const u32 g = blockIdx.x * WAVES_PER_BLOCK + wave_in_block();
    const u32 p = g * GROUP + lane;
    const bool valid = p < nb;
    // an idle lane gets an inverted box that contains and overlaps nothing
    float b0 = 1.f, b1 = 1.f, b2 = 1.f, b3 = -1.f, b4 = -1.f, b5 = -1.f;
    if (valid) {
        b0 = boxes6[6ull * p]; b1 = boxes6[6ull * p + 1]; b2 = boxes6[6ull * p + 2];
        b3 = boxes6[6ull * p + 3]; b4 = boxes6[6ull * p + 4]; b5 = boxes6[6ull * p + 5];
    }
    u32 cnt = 0;
    u64 wpos = (FILL && valid) ? offsets[p] : 0;
    auto need = [&](const NodeBox& n) {
        const float lx = n.lo(0), ly = n.lo(1), lz = n.lo(2), hx = n.hi(0), hy = n.hi(1), hz = n.hi(2);
        bool o = (hx >= b0) & (hy >= b1) & (hz >= b2) & (lx <= b3) & (ly <= b4) & (lz <= b5);
        return o & (n.poison == 0.f) & valid;
    };
    auto leaf_points = [&](const u32 leaf) {
        const Leaf lf = load_const(t.leaves + leaf);
#pragma unroll
        for (int j = 0; j < LEAF; ++j) {
            float x = lf.x[j], y = lf.y[j], z = lf.z[j];
            bool in = valid & (x >= b0) & (y >= b1) & (z >= b2) & (x <= b3) & (y <= b4) & (z <= b5);
            if (FILL) {
                if (in) out_idx[wpos + cnt] = lf.id[j];
            }
            cnt += in ? 1u : 0u;
        }
    };
    // The boxes of a wave need not lie near each other, so a leaf is needed by one or two of them as a rule: such a leaf is looked
    // at EIGHT NEEDING BOXES x EIGHT POINTS at a time, as in k_range (round 5; until then every visited leaf cost all 64 lanes its
    // eight containment tests).  The needing lanes publish their box -- and, list form, where their list stands -- by their rank
    // among the needing lanes; an unused slot holds an inverted box.
    __shared__ float4 pub_lo_s[WAVES_PER_BLOCK][32], pub_hi_s[WAVES_PER_BLOCK][32];
    __shared__ u64 pub_at_s[WAVES_PER_BLOCK][FILL ? 32 : 1];
    float4* const pub_lo = pub_lo_s[wave_in_block()];
    float4* const pub_hi = pub_hi_s[wave_in_block()];
    u64* const pub_at = pub_at_s[wave_in_block()];
    if (lane < 32u) {
        pub_lo[lane] = make_float4(1.f, 1.f, 1.f, 0.f);
        pub_hi[lane] = make_float4(-1.f, -1.f, -1.f, 0.f);
    }
    auto packed_leaf = [&](const Leaf* record, const u64 who, const u32 how_many) {
        const u32 j = lane & 7u, i = lane >> 3;
        const float* rec = reinterpret_cast<const float*>(record);
        const float x = rec[j], y = rec[LEAF + j], z = rec[2 * LEAF + j];
        u32 idj = 0;
        if (FILL) idj = reinterpret_cast<const u32*>(record)[3 * LEAF + j];
        const u32 rank = __builtin_amdgcn_mbcnt_hi(static_cast<u32>(who >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<u32>(who), 0u));
        const bool mine = __builtin_amdgcn_inverse_ballot_w64(who);
        if (mine) {
            pub_lo[rank] = make_float4(b0, b1, b2, 0.f);
            pub_hi[rank] = make_float4(b3, b4, b5, 0.f);
            if (FILL) pub_at[rank] = wpos + cnt;
        }
        __builtin_amdgcn_wave_barrier();  // (one wave: its LDS operations complete in order; this only pins the compiler's order)
        const u32 my_byte = (rank & 7u) << 3;
#pragma nounroll
        for (u32 s = 0; s < how_many; s += 8u) {
            const float4 lo = pub_lo[s + i], hi = pub_hi[s + i];
            const bool in_here = (x >= lo.x) & (y >= lo.y) & (z >= lo.z) & (x <= hi.x) & (y <= hi.y) & (z <= hi.z);  // (NaN padding fails)
            const u64 inside = __builtin_amdgcn_ballot_w64(in_here);
            if (FILL && in_here) {
                const u32 group_byte = static_cast<u32>(inside >> (lane & 56u)) & 0xFFu;
                out_idx[pub_at[s + i] + static_cast<u32>(__builtin_popcount(group_byte & ((1u << j) - 1u)))] = idj;
            }
            if (mine && rank - s < 8u) cnt += static_cast<u32>(__builtin_popcount(static_cast<u32>(inside >> my_byte) & 0xFFu));
        }
        __builtin_amdgcn_wave_barrier();
        if (mine) {
            pub_lo[rank] = make_float4(1.f, 1.f, 1.f, 0.f);
            pub_hi[rank] = make_float4(-1.f, -1.f, -1.f, 0.f);
        }
        __builtin_amdgcn_wave_barrier();
    };
    // the walk of walk_needed_leaves (pcpx_device.h) with a last-level node's needed children in a scalar loop
    WalkerT<true, true> wk;
    u32 nexp = 0;
    if (wk.start(t, need, nexp) && t.nleaves != 0u) leaf_points(0u);
    while (!wk.done()) {  // one pop per trip: a node is expanded; a last-level node looks at its needed leaves itself
        u32 loc;
        const int h = wk.pop(loc);
        if (h > 1) {
            wk.expand(t, h, loc, need);
        } else {  // (no leaf is ever popped)
            u32 needed = wk.leaves_of(t, loc, need);
            // (one copy of the leaf forms, the needed children in a loop: written out four times they cost the count kernel
            //  133 saved scalar registers)
#pragma nounroll
            while (needed != 0u) {
                u32 c;
                asm("s_ff1_i32_b32 %0, %1\n\ts_bitset0_b32 %1, %0" : "=&s"(c), "+s"(needed));
                u64 who;
                u32 how_many;
                asm("s_cmp_eq_u32 %[c], 2\n\ts_cselect_b64 %[w], %[n2], %[n3]\n\t"
                    "s_cmp_eq_u32 %[c], 1\n\ts_cselect_b64 %[w], %[n1], %[w]\n\t"
                    "s_cmp_eq_u32 %[c], 0\n\ts_cselect_b64 %[w], %[n0], %[w]\n\t"
                    "s_bcnt1_i32_b64 %[m], %[w]"
                    : [w] "=&s"(who), [m] "=s"(how_many)
                    : [c] "s"(c), [n0] "s"(wk.leaf_need[0]), [n1] "s"(wk.leaf_need[1]), [n2] "s"(wk.leaf_need[2]), [n3] "s"(wk.leaf_need[3])
                    : "scc");
                const u32 leaf = (loc << LOGW) + c;
                if (leaf < t.nleaves) {
                    if (how_many <= PACKED_LEAVES) packed_leaf(t.leaves + leaf, who, how_many);
                    else leaf_points(leaf);
                }
            }
        }
    }
    if (valid && !FILL) out_cnt[p] = cnt;
}

// ONE range, latency form (the reference's per-call shape: benchmark/spatial_data_structures_benchmark.cpp:169-213): a single
// wavefront sweeps the tree breadth first for the one range -- the (up to 64) nodes of level 3 by one lane each, then two
// levels per step (a node's 16 grandchildren are contiguous in the heap layout), the surviving nodes compacted by ballot +
// prefix count into a frontier in LDS, in ascending order: the leaves come out in curve order like the batch form's walk --,
// then one lane per point of the surviving leaves.  depth / 2 + 2 dependent round trips (the depth-first walk of the batch
// kernels: one per node and leaf on the way).  The range travels in the kernel arguments; the count and up to `cap` indices
// live in the handle's pinned stage (host memory the device writes in place), and the host polls the completion word: one
// launch, no copy, no stream synchronisation -- the count / scan / fill sequence of the batch form is two launches and two
// synchronisations (41 us per call for a range that holds a handful of points).  A frontier of more than RANGE_FRONTIER nodes
// reports cap + 1 matches: the caller takes the batch form then, as for more than cap matches.
constexpr u32 RANGE_FRONTIER = 2048;
template <bool AABB>
__global__ __launch_bounds__(64) void k_range_one(TreeView t, float a0, float a1, float a2, float a3, float a4, float a5, u32 cap,
                                                  u32* __restrict__ out_idx, u32* __restrict__ out_cnt, u32* __restrict__ done_flag,
                                                  u32 epoch)
{
    __shared__ u32 front[2][RANGE_FRONTIER];
    const u32 lane = threadIdx.x;
    const float r2 = a3 * a3;  // sphere.hpp:34 radius * radius in float
    auto need = [&](const NodeBox& b) -> bool {
        const float lx = b.lo(0), ly = b.lo(1), lz = b.lo(2), hx = b.hi(0), hy = b.hi(1), hz = b.hi(2);
        if (AABB) return (hx >= a0) & (hy >= a1) & (hz >= a2) & (lx <= a3) & (ly <= a4) & (lz <= a5) & (b.poison == 0.f);
        return box_d2(b, a0, a1, a2) <= r2;  // (NaN for a padding node)
    };
    auto level_base = [](int d) { return d == 0 ? 0u : (0x55555555u >> (32 - 2 * d)); };
    // real nodes of tree level l (the ones the build writes: the children of a real node need not be real)
    auto nreal = [&](int l) { return (t.nleaves + (1u << (2 * (t.depth - l))) - 1u) >> (2 * (t.depth - l)); };
    u32 cnt = 0, m = 0;
    bool overflow = false;
    int cur = 0;
    if (t.nleaves > 0) {
        const int l0 = t.depth < 3 ? t.depth : 3;
        bool keep = false;
        if (lane < (1u << (2 * l0)) && lane < nreal(l0)) keep = need(t.nodes[level_base(l0) + lane]);
        const u64 mask = __builtin_amdgcn_ballot_w64(keep);
        const u32 below = __builtin_amdgcn_mbcnt_hi(static_cast<u32>(mask >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<u32>(mask), 0u));
        if (keep) front[0][below] = lane;
        m = static_cast<u32>(__builtin_popcountll(mask));
        __syncthreads();
        for (int d = l0; d < t.depth && m > 0;) {
            const int s = t.depth - d >= 2 ? 2 : 1;
            const u32 fan = 1u << (2 * s);
            u32 next = 0;
            for (u32 c0 = 0; c0 < fan * m; c0 += 64u) {
                const u32 c = c0 + lane;
                bool k2 = false;
                u32 node = 0;
                if (c < fan * m) {
                    node = front[cur][c >> (2 * s)] * fan + (c & (fan - 1u));
                    if (node < nreal(d + s)) k2 = need(t.nodes[level_base(d + s) + node]);
                }
                const u64 mk = __builtin_amdgcn_ballot_w64(k2);
                const u32 bl = __builtin_amdgcn_mbcnt_hi(static_cast<u32>(mk >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<u32>(mk), 0u));
                if (k2 && next + bl < RANGE_FRONTIER) front[cur ^ 1][next + bl] = node;
                next += static_cast<u32>(__builtin_popcountll(mk));
            }
            if (next > RANGE_FRONTIER) {
                overflow = true;
                next = RANGE_FRONTIER;
            }
            d += s;
            m = next;
            cur ^= 1;
            __syncthreads();
        }
        // the points of the surviving leaves, one per lane, in leaf (= curve) order
        for (u32 c0 = 0; c0 < static_cast<u32>(LEAF) * m && !overflow; c0 += 64u) {
            const u32 c = c0 + lane;
            bool in = false;
            u32 id = 0;
            if (c < static_cast<u32>(LEAF) * m) {
                const u32 leaf = front[cur][c / LEAF];
                if (leaf < t.nleaves) {
                    const Leaf& lf = t.leaves[leaf];
                    const u32 sl = c & 7u;
                    const float x = lf.x[sl], y = lf.y[sl], z = lf.z[sl];  // (NaN padding fails every comparison below)
                    id = lf.id[sl];
                    if (AABB) {
                        in = (x >= a0) & (y >= a1) & (z >= a2) & (x <= a3) & (y <= a4) & (z <= a5);
                    } else {
                        const float dx = x - a0, dy = y - a1, dz = z - a2;
                        in = sq3(dx, dy, dz) <= r2;
                    }
                }
            }
            const u64 mk = __builtin_amdgcn_ballot_w64(in);
            const u32 at = cnt + __builtin_amdgcn_mbcnt_hi(static_cast<u32>(mk >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<u32>(mk), 0u));
            if (in && at < cap) out_idx[at] = id;
            cnt += static_cast<u32>(__builtin_popcountll(mk));
        }
    }
    if (overflow) cnt = cap + 1u;
    if (lane == 0) *out_cnt = cnt;
    __threadfence_system();  // the row and the count are visible to the host before the completion word
    if (lane == 0) __hip_atomic_store(done_flag, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace

// range: on the host -- sphere {x, y, z, r} or box {min x, y, z, max x, y, z}: it travels in the kernel arguments
int launch_range_one(Index& ix, bool aabb, const float* range, u32 cap, u32* out_idx, u32* out_cnt, u32* done_flag, u32 epoch)
{
    ProfileScope prof(ix, PCPX_K_RANGE);
    if (aabb) k_range_one<true><<<1, 64, 0, ix.stream>>>(ix.view(), range[0], range[1], range[2], range[3], range[4], range[5], cap, out_idx, out_cnt, done_flag, epoch);
    else k_range_one<false><<<1, 64, 0, ix.stream>>>(ix.view(), range[0], range[1], range[2], range[3], 0.f, 0.f, cap, out_idx, out_cnt, done_flag, epoch);
    return check_hip(hipGetLastError(), "k_range_one launch", __FILE__, __LINE__);
}

int launch_range_count(Index& ix, const QueryView& qv, bool self, u64 group_first, u64 group_count, float radius,
                       const float* d_radii, u32* d_out_cnt)
{
    if (group_count == 0) return PCPX_OK;
    u32 grid = grid_for_groups(group_count);
    u32 gf = static_cast<u32>(group_first), ge = static_cast<u32>(group_first + group_count);
    ProfileScope prof(ix, PCPX_K_RANGE);
    if (self)
        k_range<true, false><<<grid, 64 * WAVES_PER_BLOCK, 0, ix.stream>>>(ix.view(), qv, gf, ge, radius, d_radii, d_out_cnt, nullptr, nullptr);
    else
        k_range<false, false><<<grid, 64 * WAVES_PER_BLOCK, 0, ix.stream>>>(ix.view(), qv, gf, ge, radius, d_radii, d_out_cnt, nullptr, nullptr);
    return check_hip(hipGetLastError(), "k_range launch", __FILE__, __LINE__);
}

int launch_range_count_self_radius_at(Index& ix, const QueryView& qv, u64 group_first, u64 group_count, const float* d_radius, u32* d_out_cnt)
{
    if (group_count == 0) return PCPX_OK;
    ProfileScope prof(ix, PCPX_K_RANGE);
    k_range_radius_at<<<grid_for_groups(group_count), 64 * WAVES_PER_BLOCK, 0, ix.stream>>>(
        ix.view(), qv, static_cast<u32>(group_first), static_cast<u32>(group_first + group_count), d_radius, d_out_cnt);
    return check_hip(hipGetLastError(), "k_range_radius_at launch", __FILE__, __LINE__);
}

int launch_range_at_least_self(Index& ix, const QueryView& qv, u64 group_first, u64 group_count, float radius, const float* d_radius, u32 at_least,
                               uint8_t* d_keep)
{
    if (group_count == 0) return PCPX_OK;
    ProfileScope prof(ix, PCPX_K_RANGE);
    k_range_at_least<<<grid_for_groups(group_count), 64 * WAVES_PER_BLOCK, 0, ix.stream>>>(
        ix.view(), qv, static_cast<u32>(group_first), static_cast<u32>(group_first + group_count), radius, d_radius, at_least, d_keep);
    return check_hip(hipGetLastError(), "k_range_at_least launch", __FILE__, __LINE__);
}

int launch_range_fill(Index& ix, const QueryView& qv, float radius, const float* d_radii, const u64* d_offsets,
                      u32* d_out_idx)
{
    u64 groups = (static_cast<u64>(qv.nq) + GROUP - 1) / GROUP;
    if (groups == 0) return PCPX_OK;
    ProfileScope prof(ix, PCPX_K_RANGE);
    k_range<false, true><<<grid_for_groups(groups), 64 * WAVES_PER_BLOCK, 0, ix.stream>>>(ix.view(), qv, 0u, static_cast<u32>(groups), radius,
                                                                           d_radii, nullptr, d_offsets, d_out_idx);
    return check_hip(hipGetLastError(), "k_range fill launch", __FILE__, __LINE__);
}

// ---- lists of every indexed point's range, device resident: counts by input row -> offsets (exclusive scan, 64-bit) -> fill ----
// d_offsets: n_rows + 1 entries (rows = input indices; a point that is not indexed has an empty list); d_total: one u64 (device).
// d_cnt: n_rows counts (scratch of the caller); d_tile_sum: ceil(n_rows / 1024) + 1 u64 (scratch).
int launch_range_offsets(Index& ix, const u32* d_cnt, u64 n_rows, u64* d_tile_sum, u64* d_offsets)
{
    return exclusive_scan<u64>(ArrayRows<u32>{d_cnt}, n_rows, d_tile_sum, d_offsets, d_offsets + n_rows, ix.stream);  // 32-bit counts, 64-bit offsets
}
int launch_range_fill_self(Index& ix, u64 group_first, u64 group_count, float radius, const u64* d_offsets, u32* d_out_idx)
{
    if (group_count == 0) return PCPX_OK;
    QueryView qv{nullptr, nullptr, nullptr, nullptr, nullptr, static_cast<u32>(ix.n)};
    ProfileScope prof(ix, PCPX_K_RANGE);
    k_range<true, true><<<grid_for_groups(group_count), 64 * WAVES_PER_BLOCK, 0, ix.stream>>>(ix.view(), qv, static_cast<u32>(group_first),
                                                                                 static_cast<u32>(group_first + group_count), radius, nullptr, nullptr,
                                                                                 d_offsets, d_out_idx);
    return check_hip(hipGetLastError(), "k_range self fill launch", __FILE__, __LINE__);
}

// The moments form over query groups [group_first, group_first + group_count) of qv (self: the index's own points, qv.pos_lo /
// pos_hi the asked positions).  Any output may be null; the mean distance's sum is only formed when it is asked for.
int launch_range_moments(Index& ix, const QueryView& qv, bool self, u64 group_first, u64 group_count, float radius, const float* d_radii,
                         float* d_normals, float* d_centroids, float* d_mean_dist, u32* d_count)
{
    if (group_count == 0) return PCPX_OK;
    const u32 grid = grid_for_groups(group_count);
    const u32 gf = static_cast<u32>(group_first), ge = static_cast<u32>(group_first + group_count);
    MomentsOut mo;
    mo.normals = d_normals;
    mo.centroids = d_centroids;
    mo.mean_dist = d_mean_dist;
    mo.count = d_count;
    const dim3 block(64 * WAVES_PER_BLOCK);
    ProfileScope prof(ix, PCPX_K_RANGE);
    if (self) {
        if (d_mean_dist) k_range_moments<true, 2><<<grid, block, 0, ix.stream>>>(ix.view(), qv, gf, ge, radius, d_radii, mo);
        else k_range_moments<true, 1><<<grid, block, 0, ix.stream>>>(ix.view(), qv, gf, ge, radius, d_radii, mo);
    } else {
        if (d_mean_dist) k_range_moments<false, 2><<<grid, block, 0, ix.stream>>>(ix.view(), qv, gf, ge, radius, d_radii, mo);
        else k_range_moments<false, 1><<<grid, block, 0, ix.stream>>>(ix.view(), qv, gf, ge, radius, d_radii, mo);
    }
    return check_hip(hipGetLastError(), "k_range_moments launch", __FILE__, __LINE__);
}

int launch_range_moments_empty_rows(Index& ix, const u32* d_pos_of, u64 n_rows, float* d_normals, float* d_centroids, float* d_mean_dist,
                                    u32* d_count)
{
    if (n_rows == 0) return PCPX_OK;
    MomentsOut mo;
    mo.normals = d_normals;
    mo.centroids = d_centroids;
    mo.mean_dist = d_mean_dist;
    mo.count = d_count;
    k_range_moments_empty_rows<<<static_cast<u32>((n_rows + 255) / 256), 256, 0, ix.stream>>>(d_pos_of, n_rows, mo);
    return check_hip(hipGetLastError(), "k_range_moments_empty_rows launch", __FILE__, __LINE__);
}

// The features form, as launch_range_moments / launch_range_moments_empty_rows
static FeaturesOut features_out(float* d_evals, float* d_curvature, float* d_normals, float* d_axes, u32* d_count)
{
    FeaturesOut fo;
    fo.evals = d_evals;
    fo.curvature = d_curvature;
    fo.normals = d_normals;
    fo.axes = d_axes;
    fo.count = d_count;
    return fo;
}

int launch_range_features(Index& ix, const QueryView& qv, bool self, u64 group_first, u64 group_count, float radius, const float* d_radii,
                          float* d_evals, float* d_curvature, float* d_normals, float* d_axes, u32* d_count)
{
    if (group_count == 0) return PCPX_OK;
    const u32 grid = grid_for_groups(group_count);
    const u32 gf = static_cast<u32>(group_first), ge = static_cast<u32>(group_first + group_count);
    const FeaturesOut fo = features_out(d_evals, d_curvature, d_normals, d_axes, d_count);
    const dim3 block(64 * WAVES_PER_BLOCK);
    ProfileScope prof(ix, PCPX_K_RANGE);
    if (self) k_range_features<true><<<grid, block, 0, ix.stream>>>(ix.view(), qv, gf, ge, radius, d_radii, fo);
    else k_range_features<false><<<grid, block, 0, ix.stream>>>(ix.view(), qv, gf, ge, radius, d_radii, fo);
    return check_hip(hipGetLastError(), "k_range_features launch", __FILE__, __LINE__);
}

int launch_range_features_empty_rows(Index& ix, const u32* d_pos_of, u64 n_rows, float* d_evals, float* d_curvature, float* d_normals,
                                     float* d_axes, u32* d_count)
{
    if (n_rows == 0) return PCPX_OK;
    const FeaturesOut fo = features_out(d_evals, d_curvature, d_normals, d_axes, d_count);
    k_range_features_empty_rows<<<static_cast<u32>((n_rows + 255) / 256), 256, 0, ix.stream>>>(d_pos_of, n_rows, fo);
    return check_hip(hipGetLastError(), "k_range_features_empty_rows launch", __FILE__, __LINE__);
}

int launch_aabb_count(Index& ix, const float* d_boxes6, u64 nb, u32* d_out_cnt)
{
    if (nb == 0) return PCPX_OK;
    u32 grid = static_cast<u32>((nb + 64 * WAVES_PER_BLOCK - 1) / (64 * WAVES_PER_BLOCK));
    ProfileScope prof(ix, PCPX_K_RANGE);
    k_range_aabb<false><<<grid, 64 * WAVES_PER_BLOCK, 0, ix.stream>>>(ix.view(), d_boxes6, static_cast<u32>(nb), d_out_cnt, nullptr, nullptr);
    return check_hip(hipGetLastError(), "k_range_aabb launch", __FILE__, __LINE__);
}

int launch_aabb_fill(Index& ix, const float* d_boxes6, u64 nb, const u64* d_offsets, u32* d_out_idx)
{
    if (nb == 0) return PCPX_OK;
    u32 grid = static_cast<u32>((nb + 64 * WAVES_PER_BLOCK - 1) / (64 * WAVES_PER_BLOCK));
    ProfileScope prof(ix, PCPX_K_RANGE);
    k_range_aabb<true><<<grid, 64 * WAVES_PER_BLOCK, 0, ix.stream>>>(ix.view(), d_boxes6, static_cast<u32>(nb), nullptr, d_offsets, d_out_idx);
    return check_hip(hipGetLastError(), "k_range_aabb fill launch", __FILE__, __LINE__);
}

}  // namespace pcpx
