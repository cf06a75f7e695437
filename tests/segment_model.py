"""A numpy restatement of the segmentation contract of include/pcpx_segment.h, from an edge list, the normals
and the curvatures.  numpy only: no GPU, no package import, no scipy.

    dots(normals, src, dst)          -> t = (nx_i nx_j + ny_i ny_j) + nz_i nz_j per pair, every product and both sums rounded to float32
    compatible(t, min_cos, oriented) -> |t| >= min_cos, or t >= min_cos; False for a NaN t
    segment(n, src, dst, normals, min_cos, ...)     -> (labels, smooth, segments) over a symmetric edge list
    segment_cloud(pts, normals, radius, min_cos, ...) -> the same for a cloud, by float32 brute force; `inside` = the indexed rows

The contract: i and j are near iff j is in i's sphere; compatible iff their dot product passes the threshold; a point is smooth iff
it is indexed and its curvature (if any is given) is <= max_curvature; a segment is a connected component of the smooth points under
"near and compatible", labelled with its smallest smooth index; a non-smooth indexed point takes the smallest label among the
compatible smooth points in its sphere; then every row of a segment that fewer than min_size rows carry becomes NOISE; the compact form
renumbers the surviving labels 0 ... S-1 in the order of the representatives."""
import numpy as np

from cluster_model import brute_edges, components

NOISE = np.uint32(0xFFFFFFFF)
F = np.float32


def dots(normals, src, dst):
    a = np.ascontiguousarray(normals, F).reshape(-1, 3)[src]
    b = np.ascontiguousarray(normals, F).reshape(-1, 3)[dst]
    with np.errstate(invalid="ignore", over="ignore"):
        return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def compatible(t, min_cos, oriented=False):
    with np.errstate(invalid="ignore"):
        return (t if oriented else np.abs(t)) >= F(min_cos)  # (a comparison with NaN is False)


def segment(n, src, dst, normals, min_cos, curvature=None, max_curvature=np.inf, min_size=1, oriented=False, compact=True):
    """(labels uint32 (n,), smooth bool (n,), number of segments).  (src, dst): every ordered near pair, both directions of each
    (the pairs (i, i) may be among them: a point is compatible with itself or not, and either way nothing follows)."""
    src = np.asarray(src, np.int64)
    dst = np.asarray(dst, np.int64)
    if curvature is None:
        smooth = np.ones(n, bool)
    else:
        with np.errstate(invalid="ignore"):
            smooth = np.ascontiguousarray(curvature, F).reshape(-1) <= F(max_curvature)
    ok = compatible(dots(normals, src, dst), min_cos, oriented)
    grow = ok & smooth[src] & smooth[dst]
    comp = components(n, src[grow], dst[grow])
    labels = np.full(n, int(NOISE), np.int64)
    labels[smooth] = comp[smooth]
    take = ok & ~smooth[src] & smooth[dst]
    border = np.full(n, int(NOISE), np.int64)
    np.minimum.at(border, src[take], comp[dst[take]])
    labels[~smooth] = border[~smooth]
    if min_size > 1:
        live = labels != int(NOISE)
        sizes = np.bincount(labels[live], minlength=max(n, 1))
        small = np.zeros(n, bool)
        small[live] = sizes[labels[live]] < min_size
        labels[small] = int(NOISE)
    reps = np.unique(labels[labels != int(NOISE)])
    if compact:
        out = np.full(n, int(NOISE), np.int64)
        kept = labels != int(NOISE)
        out[kept] = np.searchsorted(reps, labels[kept])
        labels = out
    return labels.astype(np.uint32), smooth, len(reps)


def segment_cloud(pts, normals, radius, min_cos, curvature=None, inside=None, edges=None, **kw):
    """segment() of a cloud by input row.  inside: bool per row, the rows the index holds (None: all); the others are NOISE and not
    smooth.  edges: brute_edges(pts[inside], radius) if the caller has it already."""
    pts = np.ascontiguousarray(pts, F).reshape(-1, 3)
    n = len(pts)
    rows = np.arange(n) if inside is None else np.nonzero(inside)[0]
    if edges is None:
        edges = brute_edges(pts[rows], radius)
    nrm = np.ascontiguousarray(normals, F).reshape(-1, 3)[rows]
    curv = None if curvature is None else np.ascontiguousarray(curvature, F).reshape(-1)[rows]
    compact = kw.get("compact", True)
    lab, smooth, count = segment(len(rows), edges[0], edges[1], nrm, min_cos, curvature=curv, **kw)
    if not compact:
        live = lab != NOISE
        lab = lab.copy()
        lab[live] = rows[lab[live]]  # representatives are input rows
    full = np.full(n, NOISE, np.uint32)
    full[rows] = lab
    fsmooth = np.zeros(n, bool)
    fsmooth[rows] = smooth
    return full, fsmooth, count
