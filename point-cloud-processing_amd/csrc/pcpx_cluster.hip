// pcpx_cluster.hip -- radius-connected components and DBSCAN of the indexed cloud (include/pcpx_cluster.h):
// a fourth form of the sphere walk of pcpx_range.hip (one lane per self sphere, lane-per-range leaves) that feeds every in-range
// pair to a union-find over CURVE POSITIONS and writes no neighbour list, a second walk that gives the border points their label,
// and the passes that turn roots into labels by input row.
#include "pcpx_device.h"
#include "pcpx_cluster.h"

namespace pcpx {

namespace {

constexpr u32 NOT_CORE = 0xFFFFFFFFu;  // parent word of a position that holds no core point (= PCPX_CLUSTER_NOISE as a label)
static_assert(NOT_CORE == PCPX_CLUSTER_NOISE, "a non-core position's parent word is the noise label");
constexpr u32 CL_BLOCK = 256;

// ---- the union-find: the ECL-CC scheme of pcpx_isosurface.hip, restated over curve positions ------------
// parent[v] <= v always, a root is its own parent, a hook links the larger of two roots under the smaller with a CAS: every root is
// the smallest position of its tree, and the final root of a component is its smallest core position whatever order the hooks ran
// in.  Only core positions are vertices; the word of any other position holds NOT_CORE and is never followed.
//
// Coherence: the parent words are written by other workgroups, on other XCDs, within the hook launch, so every access to them
// there is an agent-scope atomic (relaxed: no other data is handed over through them).  Any value parent[x] ever held is an
// ancestor of x and stays one: a stale or overwritten halving store only lengthens a later walk, and two positions that show the
// same ancestor are in one tree.  A CAS succeeds only on a word that still holds its own index (a root).
// Progress: no lane waits for another.  A climb ends because parents strictly decrease; a failed CAS means another lane hooked
// that root meanwhile -- there are fewer than n hooks in all -- and the retry climbs from what the CAS returned.
__device__ __forceinline__ u32 uf_load(const u32* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ u32 uf_root(u32* parent, u32 x)
{
    u32 cur = uf_load(parent + x);
    if (cur != x) {
        u32 prev = x, next;
        while (cur > (next = uf_load(parent + cur))) {
            __hip_atomic_store(parent + prev, next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // path halving
            prev = cur;
            cur = next;
        }
    }
    return cur;
}

// joins the trees of two core positions; `a` = a known ancestor of the first (the lane's own root so far), returns the joined root
__device__ __forceinline__ u32 uf_unite(u32* parent, u32 a, u32 q)
{
    a = uf_root(parent, a);
    u32 r = uf_root(parent, q);
    while (a != r) {
        u32 lo = a < r ? a : r, hi = a < r ? r : a;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &hi, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            return lo;
        a = uf_root(parent, hi);  // hi now holds the parent it was given meanwhile
        r = uf_root(parent, lo);
    }
    return a;
}

// ---- the sphere walk of range_group (pcpx_range.hip), lane-per-range leaves, with the leaf's number handed to the caller --------
// leaf_fn(leaf, record) is called, in curve order, for every leaf below `leaf_end` whose box some lane's sphere reaches.  The walk is
// depth first in curve order, so the first node that starts at or beyond leaf_end ends it: the hook form only looks at partners
// EARLIER in curve order than its own group, about half of a full walk.
template <class LeafFn>
__device__ __forceinline__ void sphere_walk(const TreeView& t, const float qx, const float qy, const float qz, const float r2,
                                            const u32 leaf_end, LeafFn&& leaf_fn)
{
    auto need = [&](const NodeBox& b) { return box_d2(b, qx, qy, qz) <= r2; };
    WalkerT<true, false> wk;
    u32 nexp = 0;
    if (wk.start(t, need, nexp))  // the root is the only unit
        for (u32 leaf = 0; leaf < static_cast<u32>(UNIT_LEAVES) && leaf < t.nleaves && leaf < leaf_end; ++leaf)
            leaf_fn(leaf, load_const(t.leaves + leaf));
    while (!wk.done()) {  // one pop per trip; a last-level node looks at its needed leaves itself (no tree has depth 1: no leaf is popped)
        u32 loc;
        const int h = wk.pop(loc);
        if ((static_cast<u64>(loc) << (LOGW * h)) * UNIT_LEAVES >= leaf_end) break;  // this node and all that are pending lie later
        if (h > 1) {
            wk.expand(t, h, loc, need);
        } else {
            const u32 needed = wk.leaves_of(t, loc, need);
            const Leaf* records = t.leaves + (loc << LOGW) * UNIT_LEAVES;
#pragma unroll
            for (int c = 0; c < W; ++c) {
                if ((needed >> c) & 1u) {
#pragma unroll
                    for (int r = 0; r < UNIT_LEAVES; ++r) {
                        const u32 leaf = ((loc << LOGW) + c) * UNIT_LEAVES + r;
                        if (leaf >= t.nleaves || leaf >= leaf_end) break;
                        leaf_fn(leaf, load_const(records + c * UNIT_LEAVES + r));
                    }
                }
            }
        }
    }
}

struct Labels8 {
    u32 v[LEAF];
};

// the point of curve position p (p < t.n)
__device__ __forceinline__ void point_at(const TreeView& t, u32 p, float& x, float& y, float& z)
{
    const Leaf& lf = t.leaves[p / LEAF];
    x = lf.x[p % LEAF];
    y = lf.y[p % LEAF];
    z = lf.z[p % LEAF];
}

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
    float qx = 0.f, qy = 0.f, qz = 0.f;
    u32 mine = NOT_CORE;
    if (p < t.n) {
        point_at(t, p, qx, qy, qz);
        mine = uf_load(parent + p);
    }
    const float r2 = mine != NOT_CORE ? radius * radius : -1.f;  // sphere.hpp:34 radius * radius in float; -1: idle lane
    if (!any_lane(mine != NOT_CORE)) return;
    sphere_walk(t, qx, qy, qz, r2, (g + 1u) * (GROUP / LEAF), [&](const u32 leaf, const Leaf& lf) {
#pragma unroll
        for (int j = 0; j < LEAF; ++j) {
            const float dx = lf.x[j] - qx, dy = lf.y[j] - qy, dz = lf.z[j] - qz;
            const u32 q = leaf * LEAF + j;
            if (sq3(dx, dy, dz) <= r2 && q < p) {  // (a NaN padding point fails: q < t.n here)
                const u32 seen = uf_load(parent + q);
                if (seen != NOT_CORE && seen != mine) mine = uf_unite(parent, mine, q);
            }
        }
    });
}

// parent[p] = the root of p, in a launch after the hooks: the roots are fixed.  The climb here only READS (no path halving): a
// halving store is a read of parent[x] followed later by a store of an ancestor over it, and one that straddled thread x's own
// store of its root would put a lower ancestor back.  With reads only, the one store to parent[p] in this launch is its root, and
// a climb that passes through p sees either the old ancestor or the root: both lead to the same root.  (The hooks' halving has
// left the paths short.)
// The representative of a root = the smallest input index among its core points: an atomicMin per point on the root's word of aux
// would serialise a 10 M-point component on one address (measured: 113 ms of a 119 ms call), so a wave first folds the lanes that
// share the first active lane's root into one atomic, twice, and a lane that is left only issues its atomic if the word it reads
// is still larger than its index (the word only decreases: a stale read costs an atomic that changes nothing, never a lost one).
__global__ __launch_bounds__(CL_BLOCK) void k_cluster_flatten(TreeView t, u32* parent, u32* aux)
{
    const u32 p = blockIdx.x * CL_BLOCK + threadIdx.x;
    u32 r = p < t.n ? uf_load(parent + p) : NOT_CORE;
    u32 id = NOT_CORE;
    if (r != NOT_CORE) {
        for (u32 up; r > (up = uf_load(parent + r));) r = up;
        __hip_atomic_store(parent + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        id = t.leaves[p / LEAF].id[p % LEAF];
    }
    bool todo = r != NOT_CORE;
    for (int fold = 0; fold < 2; ++fold) {
        const u64 left = __builtin_amdgcn_ballot_w64(todo);
        if (left == 0ull) return;
        const int leader = __builtin_ctzll(left);
        const u32 r0 = static_cast<u32>(__builtin_amdgcn_readlane(static_cast<int>(r), leader));
        const bool same = todo && r == r0;
        u32 m = same ? id : NOT_CORE;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = min(m, static_cast<u32>(__shfl_xor(static_cast<int>(m), off)));
        if ((threadIdx.x & 63u) == static_cast<u32>(leader) && uf_load(aux + r0) > m) atomicMin(aux + r0, m);
        todo = todo && !same;
    }
    if (todo && uf_load(aux + r) > id) atomicMin(aux + r, id);
}

// parent[p] = the label of core position p (its root's representative).  In place: a thread reads its own parent word only.
__global__ __launch_bounds__(CL_BLOCK) void k_cluster_label(u32 n, u32* __restrict__ parent, const u32* __restrict__ aux)
{
    const u32 p = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (p >= n) return;
    const u32 r = parent[p];
    if (r != NOT_CORE) parent[p] = aux[r];
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
    float qx = 0.f, qy = 0.f, qz = 0.f;
    u32 best = NOT_CORE;
    if (valid) {
        point_at(t, p, qx, qy, qz);
        best = label_at[p];
    }
    const bool border = valid && best == NOT_CORE;
    const float r2 = border ? radius * radius : -1.f;
    if (any_lane(border)) {
        sphere_walk(t, qx, qy, qz, r2, t.nleaves, [&](const u32 leaf, const Leaf& lf) {
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

// labels by input row (the rows of points outside the grid were set to noise before)
__global__ __launch_bounds__(CL_BLOCK) void k_cluster_rows(TreeView t, const u32* __restrict__ final_at, u32* __restrict__ labels)
{
    const u32 p = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (p >= t.n) return;
    labels[t.leaves[p / LEAF].id[p % LEAF]] = final_at[p];
}

// ---- the number of clusters and the compact ids: row i is a representative iff labels[i] == i; exclusive scan of that flag ------
constexpr u32 CL_TILE = 1024;
__global__ __launch_bounds__(256) void k_cluster_tile_sums(const u32* __restrict__ labels, u32 n, u32* __restrict__ tile_sum)
{
    __shared__ u32 w[4];
    const u32 base = blockIdx.x * CL_TILE;
    u32 v = 0;
#pragma unroll
    for (u32 j = 0; j < CL_TILE / 256; ++j) {
        const u32 i = base + j * 256 + threadIdx.x;
        v += (i < n && labels[i] == i) ? 1u : 0u;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63u) == 0) w[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = w[0] + w[1] + w[2] + w[3];
}
// one block: tile sums -> their exclusive scan in place, and the total
__global__ __launch_bounds__(1024) void k_cluster_scan_sums(u32* __restrict__ tile_sum, u32 ntiles, u64* __restrict__ total_out)
{
    __shared__ u32 wsum[16];
    __shared__ u32 carry_s;
    const u32 t = threadIdx.x, lane = t & 63u, w = t >> 6;
    if (t == 0) carry_s = 0;
    __syncthreads();
    for (u32 base = 0; base < ntiles; base += 1024) {
        const u32 i = base + t;
        const u32 v = i < ntiles ? tile_sum[i] : 0u;
        u32 incl = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const u32 up = __shfl_up(incl, off);
            if (lane >= static_cast<u32>(off)) incl += up;
        }
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        u32 before = carry_s, total = 0;
        for (u32 j = 0; j < 16; ++j) {
            before += j < w ? wsum[j] : 0u;
            total += wsum[j];
        }
        if (i < ntiles) tile_sum[i] = before + incl - v;
        __syncthreads();
        if (t == 0) carry_s += total;
        __syncthreads();
    }
    if (t == 0 && total_out) *total_out = carry_s;
}
// rank[i] = representatives among rows [0, i)
__global__ __launch_bounds__(256) void k_cluster_ranks(const u32* __restrict__ labels, u32 n, const u32* __restrict__ tile_base, u32* __restrict__ rank)
{
    __shared__ u32 w[4];
    const u32 base = blockIdx.x * CL_TILE + threadIdx.x * (CL_TILE / 256);
    u32 c[CL_TILE / 256], s = 0;
#pragma unroll
    for (u32 j = 0; j < CL_TILE / 256; ++j) {
        c[j] = (base + j < n && labels[base + j] == base + j) ? 1u : 0u;
        s += c[j];
    }
    const u32 lane = threadIdx.x & 63u;
    u32 incl = s;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const u32 up = __shfl_up(incl, off);
        if (lane >= static_cast<u32>(off)) incl += up;
    }
    if (lane == 63) w[threadIdx.x >> 6] = incl;
    __syncthreads();
    u32 before = 0;
    for (u32 j = 0; j < (threadIdx.x >> 6); ++j) before += w[j];
    u32 at = tile_base[blockIdx.x] + before + incl - s;
#pragma unroll
    for (u32 j = 0; j < CL_TILE / 256; ++j) {
        if (base + j < n) rank[base + j] = at;
        at += c[j];
    }
}
// labels[i] = rank of its representative (in place: a thread reads and writes its own row of labels)
__global__ __launch_bounds__(CL_BLOCK) void k_cluster_compact(u32* __restrict__ labels, u32 n, const u32* __restrict__ rank)
{
    const u32 i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= n) return;
    const u32 l = labels[i];
    if (l != NOT_CORE) labels[i] = rank[l];
}

inline u32 blocks_of(u64 n, u32 per) { return static_cast<u32>((n + per - 1) / per); }

int check_cluster_args(const char* what, float radius, u32 min_pts, u32 flags, const void* labels)
{
    if (!(radius >= 0.f)) {  // (false for NaN)
        set_error("%s: the radius must be >= 0 (got %g)", what, static_cast<double>(radius));
        return PCPX_ERR_INVALID;
    }
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
    const u32 ntiles = blocks_of(rows, CL_TILE);
    auto padded = [](u64 words) { return (words * sizeof(u32) + 255) / 256 * 256; };
    const size_t parent_bytes = padded(npos > rows ? npos : rows), aux_bytes = padded(npos ? npos : 1), sums_bytes = padded(ntiles + 1);
    if ((st = ensure_scratch(ix, parent_bytes + aux_bytes + sums_bytes)) != PCPX_OK) return st;
    u32* parent = static_cast<u32*>(ix.d_scratch);
    u32* aux = reinterpret_cast<u32*>(static_cast<char*>(ix.d_scratch) + parent_bytes);
    u32* sums = reinterpret_cast<u32*>(static_cast<char*>(ix.d_scratch) + parent_bytes + aux_bytes);
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
    const bool compact = (flags & PCPX_CLUSTER_COMPACT) != 0;
    if (compact || d_cluster_count) {
        const u32 n32 = static_cast<u32>(rows);
        k_cluster_tile_sums<<<ntiles, 256, 0, s>>>(d_labels, n32, sums);
        k_cluster_scan_sums<<<1, 1024, 0, s>>>(sums, ntiles, d_cluster_count);
        if (compact) {
            u32* rank = parent;  // (free by now)
            k_cluster_ranks<<<ntiles, 256, 0, s>>>(d_labels, n32, sums, rank);
            k_cluster_compact<<<blocks_of(rows, CL_BLOCK), CL_BLOCK, 0, s>>>(d_labels, n32, rank);
        }
        PCPX_HIP(hipGetLastError());
    }
    return PCPX_OK;
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
    return on_index(h, what, WHOLE_CLOUD, [&](Index* ix) -> int {
        int st;
        if ((st = check_cluster_args(what, radius, min_pts, flags, labels)) != PCPX_OK) return st;
        if (opt_cluster_count) *opt_cluster_count = 0;
        const u64 rows = ix->n_in;
        if (rows == 0) return PCPX_OK;
        DevBuf dl(ix->pool), dc(ix->pool), dk(ix->pool), dt(ix->pool);
        if ((st = dl.alloc(rows * sizeof(u32))) != PCPX_OK) return st;
        if (opt_core && (st = dc.alloc(rows * sizeof(uint8_t))) != PCPX_OK) return st;
        if (opt_count && (st = dk.alloc(rows * sizeof(u32))) != PCPX_OK) return st;
        if (opt_cluster_count && (st = dt.alloc(sizeof(u64))) != PCPX_OK) return st;
        if ((st = cluster_self(*ix, radius, min_pts, flags, dl.as<u32>(), dc.as<uint8_t>(), dk.as<u32>(), dt.as<u64>())) != PCPX_OK) return st;
        PCPX_HIP(hipMemcpyAsync(labels, dl.p, rows * sizeof(u32), hipMemcpyDeviceToHost, ix->stream));
        if (opt_core) PCPX_HIP(hipMemcpyAsync(opt_core, dc.p, rows * sizeof(uint8_t), hipMemcpyDeviceToHost, ix->stream));
        if (opt_count) PCPX_HIP(hipMemcpyAsync(opt_count, dk.p, rows * sizeof(u32), hipMemcpyDeviceToHost, ix->stream));
        if (opt_cluster_count) PCPX_HIP(hipMemcpyAsync(opt_cluster_count, dt.p, sizeof(u64), hipMemcpyDeviceToHost, ix->stream));
        PCPX_HIP(hipStreamSynchronize(ix->stream));
        return PCPX_OK;
    });
}

}  // extern "C"
