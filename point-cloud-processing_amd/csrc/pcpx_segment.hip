// pcpx_segment.hip -- smooth-surface segmentation of the indexed cloud (include/pcpx_segment.h): the
// order-independent form of normal-constrained region growing.  A fifth form of the leaf-direct sphere walk of pcpx_device.h: its
// pair test is "within r AND the normals agree", and it reads the neighbours' normals leaf by leaf the way it reads their
// coordinates.  Every passing pair goes to the union-find of pcpx_unionfind.h over CURVE POSITIONS, a second walk gives the
// non-smooth points their label, the passes of pcpx_labels.h turn roots into labels by input row, and a size filter drops the
// small segments.
#include "pcpx_labels.h"
#include "pcpx_segment.h"

namespace pcpx {

namespace {

static_assert(NOT_CORE == PCPX_SEGMENT_NOISE, "a non-smooth position's parent word is the noise label");

// t = (ax bx + ay by) + az bz, every product and both sums rounded (no FMA: pcpx_device.h turns contraction off); |t| >= min_cos,
// or t >= min_cos where the normals' signs matter.  A NaN t fails either test.  Symmetric: every product commutes exactly.
template <bool ORIENTED>
__device__ __forceinline__ bool compatible(float ax, float ay, float az, float bx, float by, float bz, float min_cos)
{
    const float t = ax * bx + ay * by + az * bz;
    return ORIENTED ? t >= min_cos : fabsf(t) >= min_cos;
}

// One thread per leaf slot (npos = 8 nleaves of them): the point's normal from its input row into the leaf's normal record (zeros in
// a slot that holds no point: its coordinates are NaN and pass no distance test), the smooth flag into the parent word and by
// input row, and aux[p] = NOT_CORE for the representatives' atomicMin.  curvature: by input row, or null (every indexed point is
// smooth).
__global__ __launch_bounds__(CL_BLOCK) void k_segment_prep(TreeView t, u32 npos, const float* __restrict__ normals,
                                                           const float* __restrict__ curvature, float max_curvature,
                                                           Normals8* __restrict__ nrec, u32* __restrict__ parent, u32* __restrict__ aux,
                                                           uint8_t* __restrict__ smooth_row)
{
    const u32 p = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (p >= npos) return;
    bool smooth = false;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    if (p < t.n) {
        const u32 row = t.leaves[p / LEAF].id[p % LEAF];
        nx = normals[3ull * row], ny = normals[3ull * row + 1], nz = normals[3ull * row + 2];
        smooth = curvature ? curvature[row] <= max_curvature : true;  // (false for a NaN curvature)
        if (smooth_row) smooth_row[row] = smooth ? 1 : 0;
    }
    Normals8& rec = nrec[p / LEAF];
    rec.x[p % LEAF] = nx, rec.y[p % LEAF] = ny, rec.z[p % LEAF] = nz;
    parent[p] = smooth ? p : NOT_CORE;
    aux[p] = NOT_CORE;
}

// The hook launch, k_cluster_hook's half walk: one wave per group of 64 curve-consecutive positions, one lane per smooth point, its
// own normal in three registers.  Of every near and compatible pair only the side that comes LATER in curve order takes it, so each
// pair is united once and the walk ends at the group's own leaves.  A leaf's normal record is one scalar load beside its
// coordinate record; the distance test, the order test and the dot test come before the partner's parent word is read.
template <bool ORIENTED>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void k_segment_hook(TreeView t, u32 group_end, float radius, float min_cos,
                                                                      const Normals8* __restrict__ nrec, u32* parent)
{
    const u32 lane = threadIdx.x & 63u;
    const u32 g = virtual_block() * WAVES_PER_BLOCK + wave_in_block();
    if (g >= group_end) return;
    const u32 p = g * GROUP + lane;
    LaneQuery c{0.f, 0.f, 0.f, 0u};
    float nx = 0.f, ny = 0.f, nz = 0.f;
    u32 mine = NOT_CORE;
    if (p < t.n) {
        c = lane_query<true>(t, QueryView{}, p);
        const Normals8& own = nrec[p / LEAF];
        nx = own.x[p % LEAF], ny = own.y[p % LEAF], nz = own.z[p % LEAF];
        mine = uf_load(parent + p);
    }
    const float qx = c.x, qy = c.y, qz = c.z;
    const float r2 = mine != NOT_CORE ? radius * radius : -1.f;  // sphere.hpp:34 radius * radius in float; -1: idle lane
    if (!any_lane(mine != NOT_CORE)) return;
    auto need = [&](const NodeBox& b) { return box_d2(b, qx, qy, qz) <= r2; };
    walk_needed_leaves<false, true>(t, need, [&](const u32 leaf, const Leaf* record, u64, u32) {
        const Leaf lf = load_const(record);
        const Normals8 ln = load_const(nrec + leaf);
#pragma unroll
        for (int j = 0; j < LEAF; ++j) {
            const float dx = lf.x[j] - qx, dy = lf.y[j] - qy, dz = lf.z[j] - qz;
            const u32 q = leaf * LEAF + j;
            if (sq3(dx, dy, dz) <= r2 && q < p && compatible<ORIENTED>(nx, ny, nz, ln.x[j], ln.y[j], ln.z[j], min_cos)) {
                const u32 seen = uf_load(parent + q);  // (a NaN padding point fails the distance test: q < t.n here)
                if (seen != NOT_CORE && seen != mine) mine = uf_unite(parent, mine, q);
            }
        }
    }, (g + 1u) * (GROUP / LEAF));
}

// The border pass (only with a curvature array), k_cluster_border's full walk with the smooth lanes idle: a non-smooth lane takes the
// smallest label among the smooth points that are in its sphere and compatible with it (NOT_CORE, the largest word, where there is
// none: noise).  label_at is not written in this launch, so a leaf's eight labels are one scalar load beside its two records; a
// non-smooth partner's word is NOT_CORE and never wins the minimum.  final_at[p]: the label of position p.
template <bool ORIENTED>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void k_segment_border(TreeView t, u32 group_end, float radius, float min_cos,
                                                                        const Normals8* __restrict__ nrec, const u32* __restrict__ label_at,
                                                                        u32* __restrict__ final_at)
{
    const u32 lane = threadIdx.x & 63u;
    const u32 g = virtual_block() * WAVES_PER_BLOCK + wave_in_block();
    if (g >= group_end) return;
    const u32 p = g * GROUP + lane;
    const bool valid = p < t.n;
    LaneQuery c{0.f, 0.f, 0.f, 0u};
    float nx = 0.f, ny = 0.f, nz = 0.f;
    u32 best = NOT_CORE;
    if (valid) {
        c = lane_query<true>(t, QueryView{}, p);
        const Normals8& own = nrec[p / LEAF];
        nx = own.x[p % LEAF], ny = own.y[p % LEAF], nz = own.z[p % LEAF];
        best = label_at[p];
    }
    const float qx = c.x, qy = c.y, qz = c.z;
    const bool border = valid && best == NOT_CORE;
    const float r2 = border ? radius * radius : -1.f;
    if (any_lane(border)) {
        auto need = [&](const NodeBox& b) { return box_d2(b, qx, qy, qz) <= r2; };
        walk_needed_leaves<false>(t, need, [&](const u32 leaf, const Leaf* record, u64, u32) {
            const Leaf lf = load_const(record);
            const Normals8 ln = load_const(nrec + leaf);
            const Labels8 lb = load_const(reinterpret_cast<const Labels8*>(label_at + static_cast<u64>(leaf) * LEAF));
#pragma unroll
            for (int j = 0; j < LEAF; ++j) {
                const float dx = lf.x[j] - qx, dy = lf.y[j] - qy, dz = lf.z[j] - qz;
                if (sq3(dx, dy, dz) <= r2 && compatible<ORIENTED>(nx, ny, nz, ln.x[j], ln.y[j], ln.z[j], min_cos))
                    best = min(best, lb.v[j]);  // (an idle lane: r2 = -1, its own label stays)
            }
        });
    }
    if (valid) final_at[p] = best;
}

// ---- the size filter: rows per label, then the rows of the small segments to noise -------------------------------------------------
// size[l] += the rows that carry label l (a label is an input row: size has one word per row, zeroed before).  One atomic per row
// would serialise a cloud that is one segment on one address, so a wave folds the lanes that share its first active lane's label
// into one atomic, twice, as k_cluster_flatten does for the representatives.
__global__ __launch_bounds__(CL_BLOCK) void k_segment_sizes(const u32* __restrict__ labels, u32 rows, u32* size)
{
    const u32 i = blockIdx.x * CL_BLOCK + threadIdx.x;
    const u32 l = i < rows ? labels[i] : NOT_CORE;
    bool todo = l != NOT_CORE;
    for (int fold = 0; fold < 2; ++fold) {
        const u64 left = __builtin_amdgcn_ballot_w64(todo);
        if (left == 0ull) return;
        const int leader = __builtin_ctzll(left);
        const u32 l0 = static_cast<u32>(__builtin_amdgcn_readlane(static_cast<int>(l), leader));
        const bool same = todo && l == l0;
        const u32 together = static_cast<u32>(__builtin_popcountll(__builtin_amdgcn_ballot_w64(same)));
        if ((threadIdx.x & 63u) == static_cast<u32>(leader)) atomicAdd(size + l0, together);
        todo = todo && !same;
    }
    if (todo) atomicAdd(size + l, 1u);
}
// (in place: a thread reads and writes its own row of labels; nothing writes size in this launch)
__global__ __launch_bounds__(CL_BLOCK) void k_segment_drop_small(u32* __restrict__ labels, u32 rows, const u32* __restrict__ size, u32 min_size)
{
    const u32 i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= rows) return;
    const u32 l = labels[i];
    if (l != NOT_CORE && size[l] < min_size) labels[i] = NOT_CORE;
}

constexpr u32 SEGMENT_FLAGS = PCPX_SEGMENT_COMPACT | PCPX_SEGMENT_ORIENTED;

int check_segment_args(const char* what, const void* normals, const void* curvature, float radius, float min_cos, float max_curvature,
                       u32 flags, const void* labels)
{
    if (const int st = check_radius(what, radius)) return st;
    if (min_cos != min_cos) {
        set_error("%s: min_cos is NaN", what);
        return PCPX_ERR_INVALID;
    }
    if (curvature && max_curvature != max_curvature) {
        set_error("%s: max_curvature is NaN", what);
        return PCPX_ERR_INVALID;
    }
    if (flags & ~SEGMENT_FLAGS) {
        set_error("%s: unknown flag bits 0x%x", what, flags & ~SEGMENT_FLAGS);
        return PCPX_ERR_INVALID;
    }
    if (!normals) {
        set_error("%s: the normal array is NULL", what);
        return PCPX_ERR_INVALID;
    }
    if (!labels) {
        set_error("%s: the label array is NULL", what);
        return PCPX_ERR_INVALID;
    }
    return PCPX_OK;
}

template <bool ORIENTED>
void launch_segment_walks(const TreeView& t, u64 groups, float radius, float min_cos, const Normals8* nrec, u32* parent, u32* aux, bool border,
                          hipStream_t s)
{
    const u32 grid = grid_for_groups(groups), n = t.n;
    k_segment_hook<ORIENTED><<<grid, 64 * WAVES_PER_BLOCK, 0, s>>>(t, static_cast<u32>(groups), radius, min_cos, nrec, parent);
    k_cluster_flatten<<<blocks_of(n, CL_BLOCK), CL_BLOCK, 0, s>>>(t, parent, aux);
    k_cluster_label<<<blocks_of(n, CL_BLOCK), CL_BLOCK, 0, s>>>(n, parent, aux);
    if (border) k_segment_border<ORIENTED><<<grid, 64 * WAVES_PER_BLOCK, 0, s>>>(t, static_cast<u32>(groups), radius, min_cos, nrec, parent, aux);
}

}  // namespace

// Everything on the handle's stream, no synchronisation.  Scratch of the handle: parent (one word per leaf slot, and room for one per
// input row: the compact form's ranks), aux (as many: representatives by root, then final labels by position, then the sizes by
// label), the scan's tile sums and the normal records.
int segment_self(Index& ix, const float* d_normals, const float* d_curvature, float radius, float min_cos, float max_curvature, u32 min_size,
                 u32 flags, u32* d_labels, uint8_t* d_smooth, u64* d_segment_count)
{
    int st;
    hipStream_t s = ix.stream;
    const u64 rows = ix.n_in, n = ix.n;
    if (rows == 0) {
        if (d_segment_count) PCPX_HIP(hipMemsetAsync(d_segment_count, 0, sizeof(u64), s));
        return PCPX_OK;
    }
    const u64 npos = static_cast<u64>(ix.nleaves) * LEAF;  // >= n
    const u32 ntiles = scan_tiles(rows);
    Carve c;
    const u64 words = npos > rows ? npos : rows;
    const size_t parent_at = c.take(words * sizeof(u32)), aux_at = c.take(words * sizeof(u32)), sums_at = c.take((ntiles + 1ull) * sizeof(u32)),
                 nrec_at = c.take((ix.nleaves ? ix.nleaves : 1u) * sizeof(Normals8));
    if ((st = ensure_scratch(ix, c.bytes())) != PCPX_OK) return st;
    char* base = static_cast<char*>(ix.d_scratch);
    u32* parent = reinterpret_cast<u32*>(base + parent_at);
    u32* aux = reinterpret_cast<u32*>(base + aux_at);
    u32* sums = reinterpret_cast<u32*>(base + sums_at);
    Normals8* nrec = reinterpret_cast<Normals8*>(base + nrec_at);
    if (n != rows) {  // the rows of the points outside the voxel grid: noise, not smooth
        PCPX_HIP(hipMemsetAsync(d_labels, 0xFF, rows * sizeof(u32), s));
        if (d_smooth) PCPX_HIP(hipMemsetAsync(d_smooth, 0, rows * sizeof(uint8_t), s));
    }
    ProfileScope prof(ix, PCPX_K_RANGE);
    if (n > 0) {
        const TreeView t = ix.view();
        const u64 groups = (n + GROUP - 1) / GROUP;
        const bool border = d_curvature != nullptr;  // (without a curvature array no indexed point is non-smooth)
        k_segment_prep<<<blocks_of(npos, CL_BLOCK), CL_BLOCK, 0, s>>>(t, static_cast<u32>(npos), d_normals, d_curvature, max_curvature, nrec, parent,
                                                                    aux, d_smooth);
        if (flags & PCPX_SEGMENT_ORIENTED) launch_segment_walks<true>(t, groups, radius, min_cos, nrec, parent, aux, border, s);
        else launch_segment_walks<false>(t, groups, radius, min_cos, nrec, parent, aux, border, s);
        k_cluster_rows<<<blocks_of(n, CL_BLOCK), CL_BLOCK, 0, s>>>(t, border ? aux : parent, d_labels);
        PCPX_HIP(hipGetLastError());
    }
    if (min_size > 1) {  // (parent and aux are free by now)
        PCPX_HIP(hipMemsetAsync(aux, 0, rows * sizeof(u32), s));
        k_segment_sizes<<<blocks_of(rows, CL_BLOCK), CL_BLOCK, 0, s>>>(d_labels, static_cast<u32>(rows), aux);
        k_segment_drop_small<<<blocks_of(rows, CL_BLOCK), CL_BLOCK, 0, s>>>(d_labels, static_cast<u32>(rows), aux, min_size);
        PCPX_HIP(hipGetLastError());
    }
    // a dropped segment's representative row is noise now: row i is a surviving representative iff labels[i] == i
    return count_and_compact_labels(d_labels, rows, (flags & PCPX_SEGMENT_COMPACT) != 0, parent, sums, d_segment_count, s);
}

}  // namespace pcpx

using namespace pcpx;

extern "C" {

int pcpx_segment_self_dev(pcpx_index* h, const float* d_normals, const float* d_opt_curvature, float radius, float min_cos,
                          float max_curvature, uint32_t min_size, uint32_t flags, uint32_t* d_labels, uint8_t* d_opt_smooth,
                          uint64_t* d_opt_segment_count)
{
    static const char* what = "pcpx_segment_self_dev";
    return on_index(h, what, WHOLE_CLOUD, [&](Index* ix) -> int {
        int st;
        if ((st = check_segment_args(what, d_normals, d_opt_curvature, radius, min_cos, max_curvature, flags, d_labels)) != PCPX_OK) return st;
        return segment_self(*ix, d_normals, d_opt_curvature, radius, min_cos, max_curvature, min_size, flags, d_labels, d_opt_smooth,
                            d_opt_segment_count);
    });
}

int pcpx_segment_self(pcpx_index* h, const float* normals, const float* opt_curvature, float radius, float min_cos, float max_curvature,
                      uint32_t min_size, uint32_t flags, uint32_t* labels, uint8_t* opt_smooth, uint64_t* opt_segment_count)
{
    static const char* what = "pcpx_segment_self";
    return on_index_host(h, what, WHOLE_CLOUD, [&](Index* ix, Staged& stage) -> int {
        int st;
        if ((st = check_segment_args(what, normals, opt_curvature, radius, min_cos, max_curvature, flags, labels)) != PCPX_OK) return st;
        if (opt_segment_count) *opt_segment_count = 0;
        const u64 rows = ix->n_in;
        if (rows == 0) return PCPX_OK;
        const float* dn = stage.upload(normals, rows * 3 * sizeof(float));
        const float* dk = stage.upload(opt_curvature, rows * sizeof(float));
        u32* dl = stage.alloc<u32>(rows * sizeof(u32));
        uint8_t* ds = stage.alloc_for(opt_smooth, rows * sizeof(uint8_t));
        u64* dt = stage.alloc_for(opt_segment_count, sizeof(u64));
        if ((st = stage.st) != PCPX_OK ||
            (st = segment_self(*ix, dn, dk, radius, min_cos, max_curvature, min_size, flags, dl, ds, dt)) != PCPX_OK)
            return st;
        stage.download(labels, dl, rows * sizeof(u32));
        stage.download_opt(opt_smooth, ds, rows * sizeof(uint8_t));
        stage.download_opt(opt_segment_count, dt, sizeof(u64));
        return stage.wait();
    });
}

}  // extern "C"
