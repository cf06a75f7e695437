// pcpx_cluster.hip -- radius-connected components and DBSCAN of the indexed cloud (include/pcpx_cluster.h):
// the leaf-direct sphere walk of pcpx_device.h (one lane per self sphere, lane-per-range leaves) feeds every in-range pair to the
// union-find of pcpx_unionfind.h over CURVE POSITIONS and writes no neighbour list, a second walk gives the border points their
// label, and the passes after it turn roots into labels by input row.
#include "pcpx_labels.h"
#include "pcpx_cluster.h"

namespace pcpx {

namespace {

static_assert(NOT_CORE == PCPX_CLUSTER_NOISE, "a non-core position's parent word is the noise label");

// The passes from roots to labels by input row (k_cluster_flatten, k_cluster_label, k_cluster_rows, k_cluster_compact) are
// pcpx_labels.h's, shared with pcpx_segment.hip.

// One thread per leaf slot (npos = 8 nleaves of them): the core flag into the parent word, the outputs that are known by now by
// input row, and aux[p] = NOT_CORE for the representatives' atomicMin.  count_at: the sphere counts BY POSITION (null: min_pts = 1,
// every indexed point is core and no count was taken).
__global__ __launch_bounds__(CL_BLOCK) void k_cluster_init(TreeView t, u32 npos, const u32* count_at, u32 min_pts, u32* __restrict__ parent,
                                                           u32* aux, uint8_t* __restrict__ core_row, u32* __restrict__ count_row)
{
    const u32 p = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (p >= npos) return;
    bool core = false;
    if (p < t.n) {
        const u32 c = count_at ? count_at[p] : 1u;
        core = c >= min_pts;
        const u32 row = t.leaves[p / LEAF].id[p % LEAF];
        if (core_row) core_row[row] = core ? 1 : 0;
        if (count_row && count_at) count_row[row] = c;
    }
    parent[p] = core ? p : NOT_CORE;
    aux[p] = NOT_CORE;  // (count_at may be aux: read above by this thread only)
}

// The hook launch: one wave per group of 64 curve-consecutive positions, one lane per core point.  Of every in-range pair only the
// side that comes LATER in curve order takes it (the partner's position is the scalar leaf number times 8 plus j: one compare), so
// each pair is united once.  A lane keeps its root so far in a register and skips a partner whose parent word already shows it.
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void k_cluster_hook(TreeView t, u32 group_end, float radius, u32* parent)
{
    const u32 lane = threadIdx.x & 63u;
    const u32 g = virtual_block() * WAVES_PER_BLOCK + wave_in_block();
    if (g >= group_end) return;
    const u32 p = g * GROUP + lane;
    LaneQuery c{0.f, 0.f, 0.f, 0u};
    u32 mine = NOT_CORE;
    if (p < t.n) {
        c = lane_query<true>(t, QueryView{}, p);
        mine = uf_load(parent + p);
    }
    const float qx = c.x, qy = c.y, qz = c.z;
    const float r2 = mine != NOT_CORE ? radius * radius : -1.f;  // sphere.hpp:34 radius * radius in float; -1: idle lane
    if (!any_lane(mine != NOT_CORE)) return;
    auto need = [&](const NodeBox& b) { return box_d2(b, qx, qy, qz) <= r2; };
    // only partners EARLIER in curve order than the group's own end: about half of a full walk
    walk_needed_leaves<false, true>(t, need, [&](const u32 leaf, const Leaf* record, u64, u32) {
        const Leaf lf = load_const(record);
#pragma unroll
        for (int j = 0; j < LEAF; ++j) {
            const float dx = lf.x[j] - qx, dy = lf.y[j] - qy, dz = lf.z[j] - qz;
            const u32 q = leaf * LEAF + j;
            if (sq3(dx, dy, dz) <= r2 && q < p) {  // (a NaN padding point fails: q < t.n here)
                const u32 seen = uf_load(parent + q);
                if (seen != NOT_CORE && seen != mine) mine = uf_unite(parent, mine, q);
            }
        }
    }, (g + 1u) * (GROUP / LEAF));
}

// The border pass: the same walk with the core lanes idle; a non-core lane takes the smallest label among the core points in its
// sphere (NOT_CORE, the largest word, where there is none: noise).  label_at is not written in this launch, so a leaf's eight labels
// are one scalar load beside its record.  A group with no non-core lane ends at once.  final_at[p]: the label of position p.
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void k_cluster_border(TreeView t, u32 group_end, float radius, const u32* __restrict__ label_at,
                                                                        u32* __restrict__ final_at)
{
    const u32 lane = threadIdx.x & 63u;
    const u32 g = virtual_block() * WAVES_PER_BLOCK + wave_in_block();
    if (g >= group_end) return;
    const u32 p = g * GROUP + lane;
    const bool valid = p < t.n;
    LaneQuery c{0.f, 0.f, 0.f, 0u};
    u32 best = NOT_CORE;
    if (valid) {
        c = lane_query<true>(t, QueryView{}, p);
        best = label_at[p];
    }
    const float qx = c.x, qy = c.y, qz = c.z;
    const bool border = valid && best == NOT_CORE;
    const float r2 = border ? radius * radius : -1.f;
    if (any_lane(border)) {
        auto need = [&](const NodeBox& b) { return box_d2(b, qx, qy, qz) <= r2; };
        walk_needed_leaves<false>(t, need, [&](const u32 leaf, const Leaf* record, u64, u32) {
            const Leaf lf = load_const(record);
            const Labels8 lb = load_const(reinterpret_cast<const Labels8*>(label_at + static_cast<u64>(leaf) * LEAF));
#pragma unroll
            for (int j = 0; j < LEAF; ++j) {
                const float dx = lf.x[j] - qx, dy = lf.y[j] - qy, dz = lf.z[j] - qz;
                if (sq3(dx, dy, dz) <= r2) best = min(best, lb.v[j]);  // (an idle lane: r2 = -1, its own label stays)
            }
        });
    }
    if (valid) final_at[p] = best;
}


int check_cluster_args(const char* what, float radius, u32 min_pts, u32 flags, const void* labels)
{
    if (const int st = check_radius(what, radius)) return st;
    if (min_pts == 0) {
        set_error("%s: min_pts must be >= 1", what);
        return PCPX_ERR_INVALID;
    }
    if (flags & ~PCPX_CLUSTER_COMPACT) {
        set_error("%s: unknown flag bits 0x%x", what, flags & ~PCPX_CLUSTER_COMPACT);
        return PCPX_ERR_INVALID;
    }
    if (!labels) {
        set_error("%s: the label array is NULL", what);
        return PCPX_ERR_INVALID;
    }
    return PCPX_OK;
}

}  // namespace

// Everything on the handle's stream, no synchronisation.  Scratch of the handle: parent (one word per leaf slot, and room for one per
// input row: the compact form's ranks), aux (one word per leaf slot: counts by position, then representatives by root, then final
// labels by position) and the scan's tile sums.
int cluster_self(Index& ix, float radius, u32 min_pts, u32 flags, u32* d_labels, uint8_t* d_core, u32* d_count, u64* d_cluster_count)
{
    int st;
    hipStream_t s = ix.stream;
    const u64 rows = ix.n_in, n = ix.n;
    if (rows == 0) {
        if (d_cluster_count) PCPX_HIP(hipMemsetAsync(d_cluster_count, 0, sizeof(u64), s));
        return PCPX_OK;
    }
    const u64 npos = static_cast<u64>(ix.nleaves) * LEAF;  // >= n
    const u32 ntiles = scan_tiles(rows);
    Carve c;
    const size_t parent_at = c.take((npos > rows ? npos : rows) * sizeof(u32)), aux_at = c.take((npos ? npos : 1) * sizeof(u32)),
                 sums_at = c.take((ntiles + 1ull) * sizeof(u32));
    if ((st = ensure_scratch(ix, c.bytes())) != PCPX_OK) return st;
    char* base = static_cast<char*>(ix.d_scratch);
    u32* parent = reinterpret_cast<u32*>(base + parent_at);
    u32* aux = reinterpret_cast<u32*>(base + aux_at);
    u32* sums = reinterpret_cast<u32*>(base + sums_at);
    if (n != rows) {  // the rows of the points outside the voxel grid: noise, not core, count 0
        PCPX_HIP(hipMemsetAsync(d_labels, 0xFF, rows * sizeof(u32), s));
        if (d_core) PCPX_HIP(hipMemsetAsync(d_core, 0, rows * sizeof(uint8_t), s));
        if (d_count) PCPX_HIP(hipMemsetAsync(d_count, 0, rows * sizeof(u32), s));
    }
    if (n > 0) {
        const TreeView t = ix.view();
        const u64 groups = (n + GROUP - 1) / GROUP;
        const bool counted = min_pts > 1;
        QueryView qv = self_view(ix);
        if (counted) {  // the core test's counts, by position (one contiguous store per group); k_cluster_init takes them to the rows
            qv.by_position = 1;
            if ((st = launch_range_count(ix, qv, true, 0, groups, radius, nullptr, aux)) != PCPX_OK) return st;
        } else if (d_count) {  // min_pts = 1 needs no count: only the caller wants it
            if ((st = launch_range_count(ix, qv, true, 0, groups, radius, nullptr, d_count)) != PCPX_OK) return st;
        }
        ProfileScope prof(ix, PCPX_K_RANGE);
        k_cluster_init<<<blocks_of(npos, CL_BLOCK), CL_BLOCK, 0, s>>>(t, static_cast<u32>(npos), counted ? aux : nullptr, min_pts, parent, aux, d_core,
                                                                    d_count);
        const u32 grid = grid_for_groups(groups);
        k_cluster_hook<<<grid, 64 * WAVES_PER_BLOCK, 0, s>>>(t, static_cast<u32>(groups), radius, parent);
        k_cluster_flatten<<<blocks_of(n, CL_BLOCK), CL_BLOCK, 0, s>>>(t, parent, aux);
        k_cluster_label<<<blocks_of(n, CL_BLOCK), CL_BLOCK, 0, s>>>(static_cast<u32>(n), parent, aux);
        const u32* final_at = parent;
        if (counted) {  // (min_pts = 1: no indexed point is non-core)
            k_cluster_border<<<grid, 64 * WAVES_PER_BLOCK, 0, s>>>(t, static_cast<u32>(groups), radius, parent, aux);
            final_at = aux;
        }
        k_cluster_rows<<<blocks_of(n, CL_BLOCK), CL_BLOCK, 0, s>>>(t, final_at, d_labels);
        PCPX_HIP(hipGetLastError());
    }
    // (parent is free by now: the ranks, rank[i] = representatives among rows [0, i))
    return count_and_compact_labels(d_labels, rows, (flags & PCPX_CLUSTER_COMPACT) != 0, parent, sums, d_cluster_count, s);
}

}  // namespace pcpx

using namespace pcpx;

extern "C" {

int pcpx_cluster_self_dev(pcpx_index* h, float radius, uint32_t min_pts, uint32_t flags, uint32_t* d_labels, uint8_t* d_opt_core,
                          uint32_t* d_opt_count, uint64_t* d_opt_cluster_count)
{
    static const char* what = "pcpx_cluster_self_dev";
    return on_index(h, what, WHOLE_CLOUD, [&](Index* ix) -> int {
        int st;
        if ((st = check_cluster_args(what, radius, min_pts, flags, d_labels)) != PCPX_OK) return st;
        return cluster_self(*ix, radius, min_pts, flags, d_labels, d_opt_core, d_opt_count, d_opt_cluster_count);
    });
}

int pcpx_cluster_self(pcpx_index* h, float radius, uint32_t min_pts, uint32_t flags, uint32_t* labels, uint8_t* opt_core,
                      uint32_t* opt_count, uint64_t* opt_cluster_count)
{
    static const char* what = "pcpx_cluster_self";
    return on_index_host(h, what, WHOLE_CLOUD, [&](Index* ix, Staged& stage) -> int {
        int st;
        if ((st = check_cluster_args(what, radius, min_pts, flags, labels)) != PCPX_OK) return st;
        if (opt_cluster_count) *opt_cluster_count = 0;
        const u64 rows = ix->n_in;
        if (rows == 0) return PCPX_OK;
        u32* dl = stage.alloc<u32>(rows * sizeof(u32));
        uint8_t* dc = stage.alloc_for(opt_core, rows * sizeof(uint8_t));
        u32* dk = stage.alloc_for(opt_count, rows * sizeof(u32));
        u64* dt = stage.alloc_for(opt_cluster_count, sizeof(u64));
        if ((st = stage.st) != PCPX_OK || (st = cluster_self(*ix, radius, min_pts, flags, dl, dc, dk, dt)) != PCPX_OK) return st;
        stage.download(labels, dl, rows * sizeof(u32));
        stage.download_opt(opt_core, dc, rows * sizeof(uint8_t));
        stage.download_opt(opt_count, dk, rows * sizeof(u32));
        stage.download_opt(opt_cluster_count, dt, sizeof(u64));
        return stage.wait();
    });
}

}  // extern "C"
