"""A numpy restatement of the clustering contract of include/pcpx_cluster.h, from an edge list and the sphere
counts.  numpy only: no GPU, no package import, no scipy.

    brute_edges(pts, r)                  -> (src, dst, counts): every ordered pair with d2 <= r*r in float32 (the pair (i, i) included)
    edges_from_lists(offsets, indices)   -> (src, dst, counts) of CSR neighbour lists (Index.range_sphere)
    components(n, src, dst)              -> the smallest vertex index of every vertex's connected component
    cluster(n, src, dst, counts, min_pts, compact) -> (labels, core, clusters)

The contract: i ~ j iff j is in i's sphere; core iff count >= min_pts; a cluster is a connected component of the core points under
~, labelled with its smallest core index; a non-core point with a core point in its sphere takes the smallest label among those;
everything else is NOISE.  The compact form renumbers the labels 0 ... C-1 in the order of the representatives."""
import numpy as np

NOISE = np.uint32(0xFFFFFFFF)
F = np.float32


def brute_edges(pts, r, block=256):
    """Every ordered pair (i, j) with (dx*dx + dy*dy) + dz*dz <= r*r, d = p_j - p_i, all in float32 (three roundings, no fused
    multiply-add: the arithmetic of pcpx_range_count_*).  Brute force over a slab: the points are ordered along the cloud's longest
    axis and a block of rows is tested against every point whose coordinate lies within r (and a margin far above any rounding) of
    the block's, which is a superset of what can pass the float32 test."""
    pts = np.ascontiguousarray(pts, F).reshape(-1, 3)
    n = len(pts)
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.uint32)
    axis = int(np.argmax(np.ptp(pts.astype(np.float64), 0)))
    order = np.argsort(pts[:, axis], kind="stable")
    s = pts[order]
    key = s[:, axis].astype(np.float64)
    reach = float(r) * (1 + 1e-3) + 8 * float(np.spacing(F(np.abs(key).max() + float(r))))
    r2 = F(r) * F(r)
    src, dst = [], []
    for b0 in range(0, n, block):
        b1 = min(n, b0 + block)
        lo = int(np.searchsorted(key, key[b0] - reach, "left"))
        hi = int(np.searchsorted(key, key[b1 - 1] + reach, "right"))
        d = s[None, lo:hi, :] - s[b0:b1, None, :]
        d2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
        i, j = np.nonzero(d2 <= r2)
        src.append(order[b0 + i])
        dst.append(order[lo + j])
    src = np.concatenate(src).astype(np.int64)
    dst = np.concatenate(dst).astype(np.int64)
    return src, dst, np.bincount(src, minlength=n).astype(np.uint32)


def edges_from_lists(offsets, indices):
    """(src, dst, counts) of CSR lists: row i's entries are the points in i's sphere."""
    off = np.asarray(offsets).astype(np.int64)
    counts = np.diff(off)
    src = np.repeat(np.arange(len(counts), dtype=np.int64), counts)
    return src, np.asarray(indices).astype(np.int64), counts.astype(np.uint32)


def components(n, src, dst, want_rounds=False):
    """label[v] = the smallest vertex of v's connected component.  Hook on roots plus pointer jumping until stable: a round hooks
    the larger of every edge's two roots under the smaller (the minimum over the edges that ask), then jumps every pointer to its
    root.  parent[v] <= v throughout and labels only decrease, so the fixed point is the component's minimum."""
    parent = np.arange(n, dtype=np.int64)
    src = np.asarray(src, np.int64)
    dst = np.asarray(dst, np.int64)
    rounds = 0
    while True:
        rounds += 1
        a, b = parent[src], parent[dst]  # (roots: the pointers were jumped to the end)
        differ = a != b
        if not differ.any():
            break
        np.minimum.at(parent, np.maximum(a[differ], b[differ]), np.minimum(a[differ], b[differ]))
        while True:
            nxt = parent[parent]
            if np.array_equal(nxt, parent):
                break
            parent = nxt
    return (parent, rounds) if want_rounds else parent


def cluster(n, src, dst, counts, min_pts, compact=True, symmetric=False):
    """(labels uint32 (n,), core bool (n,), number of clusters) by the contract above.  The edge list may hold (i, i) pairs;
    symmetric=True says it already holds both directions of every pair (neighbour lists do), else the other direction is added."""
    src = np.asarray(src, np.int64)
    dst = np.asarray(dst, np.int64)
    if not symmetric:
        src, dst = np.concatenate([src, dst]), np.concatenate([dst, src])
    core = np.asarray(counts) >= min_pts
    both = core[src] & core[dst]
    comp = components(n, src[both], dst[both])
    labels = np.full(n, int(NOISE), np.int64)
    labels[core] = comp[core]
    # border: the smallest label among the core points in a non-core point's sphere
    take = ~core[src] & core[dst]
    border = np.full(n, int(NOISE), np.int64)
    np.minimum.at(border, src[take], comp[dst[take]])
    labels[~core] = border[~core]
    reps = np.unique(labels[core])
    if compact:
        out = np.full(n, int(NOISE), np.int64)
        kept = labels != int(NOISE)
        out[kept] = np.searchsorted(reps, labels[kept])
        labels = out
    return labels.astype(np.uint32), core, len(reps)
