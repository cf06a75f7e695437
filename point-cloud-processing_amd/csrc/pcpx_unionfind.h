// pcpx_unionfind.h -- the lock-free union-find of the connected-component passes, in the style of ECL-CC: the active cubes of the
// hint-seeded surface (pcpx_isosurface.hip) and the core points of the clustering (pcpx_cluster.hip; section 17).
// parent[v] <= v always, a root is its own parent, a hook links the larger of two roots under the smaller with a CAS: every root is
// the smallest vertex of its tree, and the final root of a component is its smallest vertex whatever order the hooks ran in.
//
// Coherence: the parent words are written by other workgroups, on other XCDs, within the hook launch, so every access to them
// there is an agent-scope atomic (relaxed: no other data is handed over through them).  Any value parent[x] ever held is an
// ancestor of x and stays one: a stale or overwritten halving store only lengthens a later walk, and two vertices that show the
// same ancestor are in one tree.  A CAS succeeds only on a word that still holds its own index (a root).
// Progress: no lane waits for another.  A climb ends because parents strictly decrease; a failed CAS means another lane hooked
// that root meanwhile -- there are fewer than n hooks in all -- and the retry climbs from what the CAS returned.
//
// Flattening (parent[x] = the root of x, in a launch after the hooks: the roots are fixed) climbs with uf_find, which only READS.
// A halving store is a read of parent[x] followed later by a store of an ancestor over it, and one that straddled thread x's own
// store of its root would put a non-root back.  With reads only, the one store to parent[x] in that launch is its root, and a
// climb that passes through x sees either the old ancestor or the root: both lead to the same root.  (The hooks' halving has left
// the paths short.)
#ifndef PCPX_UNIONFIND_H
#define PCPX_UNIONFIND_H

#include "pcpx_internal.h"

namespace pcpx {
namespace {

__device__ __forceinline__ u32 uf_load(const u32* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root above x, a vertex or a known ancestor of one; stores nothing
__device__ __forceinline__ u32 uf_find(const u32* parent, u32 x)
{
    for (u32 up; x > (up = uf_load(parent + x));) x = up;
    return x;
}

// the root of x, with path halving
__device__ __forceinline__ u32 uf_root(u32* parent, u32 x)
{
    u32 cur = uf_load(parent + x);
    if (cur != x) {
        u32 prev = x, next;
        while (cur > (next = uf_load(parent + cur))) {
            __hip_atomic_store(parent + prev, next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            prev = cur;
            cur = next;
        }
    }
    return cur;
}

// joins the trees of two vertices; `a` may be a known ancestor of the first (a lane's own root so far); returns the joined root
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

}  // namespace
}  // namespace pcpx

#endif
