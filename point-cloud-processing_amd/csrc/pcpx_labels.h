// pcpx_labels.h -- from union-find roots over curve positions to labels by input row: the passes that clustering (pcpx_cluster.hip;
// DESIGN.md section 17) and smooth-surface segmentation (pcpx_segment.hip; section 19) run after their hook launch, and the
// compaction of the labels to 0 ... C-1.  Included by .hip translation units only.
#ifndef PCPX_LABELS_H
#define PCPX_LABELS_H

#include "pcpx_device.h"
#include "pcpx_scan.h"
#include "pcpx_stage.h"
#include "pcpx_unionfind.h"

namespace pcpx {
namespace {

constexpr u32 NOT_CORE = 0xFFFFFFFFu;  // parent word of a position that holds no core point (= the noise label)
constexpr u32 CL_BLOCK = 256;

// The union-find (pcpx_unionfind.h) runs over curve positions: only core positions are vertices; the word of any other position
// holds NOT_CORE and is never followed.  The final root of a component is its smallest core position.

struct Labels8 {
    u32 v[LEAF];
};

// parent[p] = the root of p, in a launch after the hooks, by the read-only climb (uf_find, pcpx_unionfind.h).
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
        r = uf_find(parent, r);
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

// labels by input row (the rows of points outside the grid were set to noise before)
__global__ __launch_bounds__(CL_BLOCK) void k_cluster_rows(TreeView t, const u32* __restrict__ final_at, u32* __restrict__ labels)
{
    const u32 p = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (p >= t.n) return;
    labels[t.leaves[p / LEAF].id[p % LEAF]] = final_at[p];
}

// ---- the number of clusters and the compact ids: row i is a representative iff labels[i] == i; exclusive scan of that flag ------
struct IsRepresentative {
    const u32* labels;
    __device__ u32 operator()(u32 i) const { return labels[i] == i ? 1u : 0u; }
};
// labels[i] = rank of its representative (in place: a thread reads and writes its own row of labels)
__global__ __launch_bounds__(CL_BLOCK) void k_cluster_compact(u32* __restrict__ labels, u32 n, const u32* __restrict__ rank)
{
    const u32 i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= n) return;
    const u32 l = labels[i];
    if (l != NOT_CORE) labels[i] = rank[l];
}

// The tail of a labelling call: the count of representatives among `rows` label rows into *d_count (may be null) and, compact, the
// labels renumbered 0 ... C-1 in the order of the representatives.  rank: `rows` words (used only when compact); sums: the scan's
// tile sums.  On stream s, no synchronisation.
inline int count_and_compact_labels(u32* d_labels, u64 rows, bool compact, u32* rank, u32* sums, u64* d_count, hipStream_t s)
{
    if (!compact && !d_count) return PCPX_OK;
    int st;
    if ((st = exclusive_scan(IsRepresentative{d_labels}, rows, sums, compact ? rank : nullptr, d_count, s)) != PCPX_OK) return st;
    if (compact) k_cluster_compact<<<blocks_of(rows, CL_BLOCK), CL_BLOCK, 0, s>>>(d_labels, static_cast<u32>(rows), rank);
    PCPX_HIP(hipGetLastError());
    return PCPX_OK;
}

}  // namespace
}  // namespace pcpx

#endif
