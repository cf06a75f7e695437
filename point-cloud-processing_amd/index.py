"""Host-side mirror (Python) of the reference's spatial containers and normal estimation, in batched
form, over the C ABI of libpcpx.so.  The C++17 drop-in headers live in include/pcp/; this module
exists so that tests and bench.py can drive the same entry points from Python.

Names follow the reference: LinkedOctree ~ pcp::basic_linked_octree_t
(include/pcp/octree/linked_octree.hpp:40-41), LinkedKdTree ~ pcp::basic_linked_kdtree_t
(include/pcp/kdtree/linked_kdtree.hpp:64-65), estimate_normals ~ pcp::algorithm::estimate_normals
(include/pcp/algorithm/estimate_normals.hpp:58-65).  Elements are indices into the input array.
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import BuildParams, PcpxError, check  # noqa: F401

INVALID = np.uint32(0xFFFFFFFF)


def _f32(a, cols=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if cols is not None:
        a = a.reshape(-1, cols)
    return a


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def device_count():
    n = C.c_int(0)
    check(_capi.load().pcpx_device_count(C.byref(n)))
    return n.value


def bounding_box(xyz, device=0):
    """pcp::bounding_box (include/pcp/common/axis_aligned_bounding_box.hpp:214-251) on the GPU."""
    xyz = _f32(xyz, 3)
    out = np.zeros(6, np.float32)
    check(_capi.load().pcpx_bounding_box(_vp(xyz), len(xyz), device, out.ctypes.data_as(_capi.f32p)))
    return out


def shard_range(n, rank, world):
    a, b = C.c_uint64(0), C.c_uint64(0)
    check(_capi.load().pcpx_shard_range(n, rank, world, C.byref(a), C.byref(b)))
    return a.value, b.value


def shard_cuts_by_cost(n, world, group_stride, events):
    """pcpx_shard_cuts_by_cost: world + 1 curve positions (multiples of 64) that cut the order into shards of equal estimated WORK;
    events = the table of Index.knn_group_costs (nsamples x 4, uint32)."""
    ev = np.ascontiguousarray(events, dtype=np.uint32).reshape(-1, 4)
    out = (C.c_uint64 * (world + 1))()
    check(_capi.load().pcpx_shard_cuts_by_cost(n, world, group_stride, _vp(ev) if len(ev) else None, len(ev), out))
    return [int(v) for v in out]


def estimate_normal(points, device=0):
    """pcp::estimate_normal (include/pcp/common/normals/normal_estimation.hpp:32-78)."""
    pts = _f32(points, 3)
    out = np.zeros(3, np.float32)
    check(_capi.load().pcpx_estimate_normal(_vp(pts), len(pts), device, out.ctypes.data_as(_capi.f32p)))
    return out


def estimate_normals_batch(points, offsets, device=0):
    """pcpx_estimate_normals_batch: estimate_normal of every neighbourhood r = points[offsets[r] : offsets[r + 1]] in one launch
    (nrows + 1 offsets; they must not decrease, and need not start at 0).  Returns nrows x 3 float32."""
    pts = _f32(points, 3)
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    nrows = max(len(off) - 1, 0)
    out = np.zeros((nrows, 3), np.float32)
    check(_capi.load().pcpx_estimate_normals_batch(_vp(pts) if len(pts) else None, _vp(off) if len(off) else None, nrows, device,
                                                   _vp(out) if nrows else None))
    return out


class Index:
    """Owns a pcpx_index handle: the device-resident curve-sorted implicit AABB tree."""

    def __init__(self, xyz, voxel_grid=None, device=0, coarse_order=False, shard=None, k_hint=0):
        self._lib = _capi.load()
        self._h = C.c_void_p(None)
        self.device = device
        xyz = _f32(xyz, 3)
        self.n_in = len(xyz)
        p = self._params(voxel_grid, coarse_order, shard, k_hint)
        check(self._lib.pcpx_index_create(_vp(xyz), len(xyz), p, device, C.byref(self._h)))

    @staticmethod
    def _params(voxel_grid, coarse_order=False, shard=None, k_hint=0, borrow=False, shard_range=None):
        """pcpx_build_params: voxel_grid = the explicit grid (PCPX_BUILD_USE_GRID); coarse_order = PCPX_BUILD_COARSE_ORDER (an index that
        is rebuilt after a query pass or two: one radix pass fewer on a uniform cloud, same results); shard = (rank, world):
        PCPX_BUILD_SHARD, the rank-local index of the multi-GPU path (k_hint sizes its halo; borrow = PCPX_BUILD_BORROW_CLOUD)."""
        if shard_range is not None and shard is None:
            shard = (0, 1)
        if voxel_grid is None and not coarse_order and shard is None:
            return None
        p = BuildParams()
        p.struct_size = C.sizeof(BuildParams)
        p.flags = (_capi.PCPX_BUILD_USE_GRID if voxel_grid is not None else 0) | (_capi.PCPX_BUILD_COARSE_ORDER if coarse_order else 0)
        if shard is not None:
            p.flags |= _capi.PCPX_BUILD_SHARD | (_capi.PCPX_BUILD_BORROW_CLOUD if borrow else 0)
            p.shard_rank, p.shard_world = int(shard[0]), int(shard[1])
            p.shard_k_hint = int(k_hint)
            if shard_range is not None:  # PCPX_BUILD_SHARD_RANGE: explicit curve positions (first, count), e.g. a cut by work
                p.flags |= _capi.PCPX_BUILD_SHARD_RANGE
                p.shard_first, p.shard_count = int(shard_range[0]), int(shard_range[1])
        if voxel_grid is None:
            return C.pointer(p)
        g = np.asarray(voxel_grid, np.float32).reshape(6)
        for a in range(3):
            p.grid_min[a] = float(g[a])
            p.grid_max[a] = float(g[3 + a])
        return C.pointer(p)

    def rebuild(self, xyz, voxel_grid=None, coarse_order=False, shard=None, k_hint=0):
        xyz = _f32(xyz, 3)
        check(self._lib.pcpx_index_rebuild(self._h, _vp(xyz), len(xyz), self._params(voxel_grid, coarse_order, shard, k_hint)))
        self.n_in = len(xyz)

    def shard_info(self):
        """A rank-local index described (pcpx_index_shard_info)."""
        out = (C.c_uint64 * 8)()
        check(self._lib.pcpx_index_shard_info(self._h, out))
        names = ["local_points", "core_first", "core_count", "shard_first", "shard_count", "halo_cells", "last_failed", "enlargements"]
        return {k: int(out[i]) for i, k in enumerate(names)}

    def close(self):
        if self._h:
            self._lib.pcpx_index_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- container queries ----
    def size(self):
        n = C.c_uint64(0)
        check(self._lib.pcpx_index_size(self._h, C.byref(n)))
        return n.value

    def empty(self):
        return self.size() == 0

    def bbox(self):
        out = np.zeros(6, np.float32)
        check(self._lib.pcpx_index_bbox(self._h, out.ctypes.data_as(_capi.f32p)))
        return out

    # ---- kNN ----
    def knn_self(self, k, eps=1e-5, want_d2=False):
        idx = np.empty((self.n_in, k), np.uint32)
        cnt = np.empty(self.n_in, np.uint32)
        d2 = np.empty((self.n_in, k), np.float32) if want_d2 else None
        check(self._lib.pcpx_knn_self(self._h, k, eps, _vp(idx), _vp(cnt), _vp(d2)))
        return (idx, cnt, d2) if want_d2 else (idx, cnt)

    def knn(self, queries, k, eps=1e-5, want_d2=False):
        q = _f32(queries, 3)
        idx = np.empty((len(q), k), np.uint32)
        cnt = np.empty(len(q), np.uint32)
        d2 = np.empty((len(q), k), np.float32) if want_d2 else None
        check(self._lib.pcpx_knn_batch(self._h, _vp(q), len(q), k, eps, _vp(idx), _vp(cnt), _vp(d2)))
        return (idx, cnt, d2) if want_d2 else (idx, cnt)

    # ---- radius search ----
    def range_count_self(self, radius):
        cnt = np.empty(self.n_in, np.uint32)
        check(self._lib.pcpx_range_count_self(self._h, radius, _vp(cnt)))
        return cnt

    def range_count(self, queries, radius):
        q = _f32(queries, 3)
        cnt = np.empty(len(q), np.uint32)
        check(self._lib.pcpx_range_count_batch(self._h, _vp(q), len(q), radius, _vp(cnt)))
        return cnt

    def range_sphere(self, centers, radius):
        """CSR (offsets, indices) of the points inside each sphere; radius scalar or per-sphere."""
        q = _f32(centers, 3)
        radii = None
        r = 0.0
        if np.ndim(radius) == 0:
            r = float(radius)
        else:
            radii = _f32(radius).reshape(-1)
            assert len(radii) == len(q)
        off = np.zeros(len(q) + 1, np.uint64)
        st = self._lib.pcpx_range_sphere_batch(self._h, _vp(q), _vp(radii), r, len(q), _vp(off), None, 0)
        if st == _capi.PCPX_OK:
            return off, np.empty(0, np.uint32)
        if st != _capi.PCPX_ERR_CAPACITY:
            check(st)
        out = np.empty(int(off[-1]), np.uint32)
        check(self._lib.pcpx_range_sphere_batch(self._h, _vp(q), _vp(radii), r, len(q), _vp(off), _vp(out), len(out)))
        return off, out

    def range_aabb(self, boxes):
        b = _f32(boxes, 6)
        off = np.zeros(len(b) + 1, np.uint64)
        st = self._lib.pcpx_range_aabb_batch(self._h, _vp(b), len(b), _vp(off), None, 0)
        if st == _capi.PCPX_OK:
            return off, np.empty(0, np.uint32)
        if st != _capi.PCPX_ERR_CAPACITY:
            check(st)
        out = np.empty(int(off[-1]), np.uint32)
        check(self._lib.pcpx_range_aabb_batch(self._h, _vp(b), len(b), _vp(off), _vp(out), len(out)))
        return off, out

    # ---- fixed-radius neighbourhoods (include/pcpx_radius.h) ----
    @staticmethod
    def _moments_outputs(rows, normals, centroids, mean_dist, counts):
        if not (normals or centroids or mean_dist or counts):
            raise ValueError("ask for at least one of normals, centroids, mean_dist, counts")
        return (np.empty((rows, 3), np.float32) if normals else None, np.empty((rows, 3), np.float32) if centroids else None,
                np.empty(rows, np.float32) if mean_dist else None, np.empty(rows, np.uint32) if counts else None)

    @staticmethod
    def _moments_result(outs):
        got = tuple(o for o in outs if o is not None)
        return got[0] if len(got) == 1 else got

    def range_neighbourhoods_self(self, radius, normals=True, centroids=False, mean_dist=False, counts=False):
        """Per indexed point, over every point within `radius` (itself included): the PCA normal (n x 3), the centroid (n x 3), the
        mean distance (n) and the count (n), in input order -- what estimate_normals, estimate_tangent_planes and
        average_distances_to_neighbors give with a range_search(sphere) map.  Returns the asked outputs in that order (one array
        alone when one is asked).  An empty neighbourhood (a point outside the voxel grid): normal (0, 0, 1), NaN centroid and
        mean distance, count 0."""
        outs = self._moments_outputs(self.n_in, normals, centroids, mean_dist, counts)
        check(self._lib.pcpx_range_neighbourhoods_self(self._h, float(radius), *(_vp(o) for o in outs)))
        return self._moments_result(outs)

    def range_neighbourhoods(self, queries, radius, normals=True, centroids=False, mean_dist=False, counts=False):
        """The same for arbitrary spheres: centres `queries` (m x 3), `radius` a scalar or one radius per sphere."""
        q = _f32(queries, 3)
        radii = None
        r = 0.0
        if np.ndim(radius) == 0:
            r = float(radius)
        else:
            radii = _f32(radius).reshape(-1)
            if len(radii) != len(q):
                raise ValueError("one radius per sphere")
        outs = self._moments_outputs(len(q), normals, centroids, mean_dist, counts)
        check(self._lib.pcpx_range_neighbourhoods_batch(self._h, _vp(q), _vp(radii), r, len(q), *(_vp(o) for o in outs)))
        return self._moments_result(outs)

    def range_neighbourhoods_self_dev(self, radius, d_normals=None, d_centroids=None, d_mean_dist=None, d_counts=None, first=0,
                                      count=_capi.UINT64_MAX):
        """Device form (pointers to device arrays by input row; any may be None, not all), enqueued on the index's stream: the rows of
        the curve positions [first, first + count) -- plus, when that is the whole order, the rows of points outside the grid."""
        check(self._lib.pcpx_range_neighbourhoods_self_dev(self._h, float(radius), first, count,
                                                           *(C.c_void_p(d) if d else None for d in (d_normals, d_centroids, d_mean_dist, d_counts))))

    # ---- local shape features (include/pcpx_features.h) ----
    @staticmethod
    def _features_outputs(rows, evals, curvature, normals, axes, counts):
        if not (evals or curvature or normals or axes or counts):
            raise ValueError("ask for at least one of evals, curvature, normals, axes, counts")
        return (np.empty((rows, 3), np.float32) if evals else None, np.empty(rows, np.float32) if curvature else None,
                np.empty((rows, 3), np.float32) if normals else None, np.empty((rows, 3), np.float32) if axes else None,
                np.empty(rows, np.uint32) if counts else None)

    def shape_features_self(self, radius, evals=True, curvature=True, normals=False, axes=False, counts=False):
        """Per indexed point, over every point within `radius` (itself included, the neighbourhood of range_neighbourhoods_self):
        the three eigenvalues of the centred scatter matrix (n x 3, ascending, not divided by the count), the surface variation
        max(l0, 0) / (l0 + l1 + l2) (n; the `curvature` that Index.segment gates on), the PCA normal (n x 3, bit for bit that of
        range_neighbourhoods_self), the principal axis (n x 3: the largest eigenvalue's eigenvector) and the count (n), in input
        order.  Returns the asked outputs in that order (one array alone when one is asked).  An empty neighbourhood (a point
        outside the voxel grid): eigenvalues 0, curvature NaN, normal and axis (0, 0, 1), count 0."""
        outs = self._features_outputs(self.n_in, evals, curvature, normals, axes, counts)
        check(self._lib.pcpx_shape_features_self(self._h, float(radius), *(_vp(o) for o in outs)))
        return self._moments_result(outs)

    def shape_features(self, queries, radius, evals=True, curvature=True, normals=False, axes=False, counts=False):
        """The same for arbitrary spheres: centres `queries` (m x 3), `radius` a scalar or one radius per sphere."""
        q = _f32(queries, 3)
        radii = None
        r = 0.0
        if np.ndim(radius) == 0:
            r = float(radius)
        else:
            radii = _f32(radius).reshape(-1)
            if len(radii) != len(q):
                raise ValueError("one radius per sphere")
        outs = self._features_outputs(len(q), evals, curvature, normals, axes, counts)
        check(self._lib.pcpx_shape_features_batch(self._h, _vp(q), _vp(radii), r, len(q), *(_vp(o) for o in outs)))
        return self._moments_result(outs)

    def shape_features_self_dev(self, radius, d_evals=None, d_curvature=None, d_normals=None, d_axes=None, d_counts=None, first=0,
                                count=_capi.UINT64_MAX):
        """Device form (pointers to device arrays by input row; any may be None, not all), enqueued on the index's stream: the rows of
        the curve positions [first, first + count) -- plus, when that is the whole order, the rows of points outside the grid."""
        check(self._lib.pcpx_shape_features_self_dev(self._h, float(radius), first, count,
                                                     *(C.c_void_p(d) if d else None for d in (d_evals, d_curvature, d_normals, d_axes, d_counts))))

    # ---- moving least squares projection (include/pcpx_mls.h) ----
    @staticmethod
    def _mls_outputs(rows, points, displacements, normals, curvatures, counts, fit):
        if not (points or displacements or normals or curvatures or counts or fit):
            raise ValueError("ask for at least one of points, displacements, normals, curvatures, counts, fit")
        f3 = lambda want: np.empty((rows, 3), np.float32) if want else None
        return (f3(points), f3(displacements), f3(normals), np.empty((rows, 2), np.float32) if curvatures else None,
                np.empty(rows, np.uint32) if counts else None, np.empty(rows, np.uint32) if fit else None)

    @staticmethod
    def _mls_h(radius, gauss_h):
        return float(np.float32(radius) / np.float32(2)) if gauss_h is None else float(gauss_h)

    def mls_project_self(self, radius, gauss_h=None, order=2, points=True, displacements=False, normals=True, curvatures=False,
                         counts=False, fit=False):
        """Moving least squares projection of every indexed point, over every point within `radius` (itself included, the sphere of
        range_neighbourhoods_self) with the weight exp(-d^2 / gauss_h^2): order 1 projects onto the weighted PCA plane, order 2 onto
        a quadric fitted over that plane.  Outputs in input order: the projected points (n x 3), the displacements added to them
        (n x 3; far from the origin they keep what float32 points round away), the surface normals (n x 3), the mean and Gaussian
        curvature (n x 2; NaN unless fit = 2), the count (n) and the fit (n: 0 unchanged -- fewer than 3 points --, 1 plane,
        2 quadric).  Returns the asked outputs in that order (one array alone when one is asked).
        gauss_h defaults to radius / 2: the weight at the sphere's rim is then e^-4 (a radius of 0 needs a width of its own).  (PCL's
        default, h = r, leaves a jump of e^-1 at the rim: a point that crosses it changes the fit at once.)"""
        outs = self._mls_outputs(self.n_in, points, displacements, normals, curvatures, counts, fit)
        check(self._lib.pcpx_mls_project_self(self._h, float(radius), self._mls_h(radius, gauss_h), int(order), *(_vp(o) for o in outs)))
        return self._moments_result(outs)

    def mls_project(self, queries, radius, gauss_h=None, order=2, radii=None, points=True, displacements=False, normals=True,
                    curvatures=False, counts=False, fit=False):
        """The same for arbitrary sphere centres `queries` (m x 3): each is projected onto the surface of the indexed cloud.  radii: one
        radius per sphere; sphere i then uses the width gauss_h * radii[i] / radius, so `radius` (> 0) is the radius that gauss_h
        belongs to."""
        q = _f32(queries, 3)
        if radii is not None:
            radii = _f32(radii).reshape(-1)
            if len(radii) != len(q):
                raise ValueError("one radius per sphere")
        outs = self._mls_outputs(len(q), points, displacements, normals, curvatures, counts, fit)
        check(self._lib.pcpx_mls_project_batch(self._h, _vp(q), _vp(radii), float(radius), self._mls_h(radius, gauss_h), int(order), len(q),
                                               *(_vp(o) for o in outs)))
        return self._moments_result(outs)

    def mls_project_self_dev(self, radius, gauss_h=None, order=2, d_points=None, d_displacements=None, d_normals=None, d_curvatures=None,
                             d_counts=None, d_fit=None, first=0, count=_capi.UINT64_MAX):
        """Device form (pointers to device arrays by input row; any may be None, not all), enqueued on the index's stream: the rows of
        the curve positions [first, first + count) -- plus, when that is the whole order, the rows of points that are not indexed.
        d_points is a cloud like any other: it goes straight into Index.from_device."""
        check(self._lib.pcpx_mls_project_self_dev(self._h, float(radius), self._mls_h(radius, gauss_h), int(order), first, count,
                                                  *(C.c_void_p(d) if d else None
                                                    for d in (d_points, d_displacements, d_normals, d_curvatures, d_counts, d_fit))))

    # ---- clustering (include/pcpx_cluster.h) ----
    def cluster(self, radius, min_pts=1, compact=True, want_core=False, want_counts=False):
        """Radius-connected components (min_pts = 1) or DBSCAN of the indexed cloud: two points are joined iff one is in the other's
        sphere (the rule of range_count_self), a point is core iff its sphere holds >= min_pts points (itself included), clusters are
        the connected components of the core points, a non-core point with a core neighbour joins the smallest-labelled one's
        cluster, every other point (and every point outside the voxel grid) is noise: label 0xFFFFFFFF.  compact: labels
        0 ... C-1 ordered by representative, else the representative itself (the cluster's smallest core input index).
        Returns (labels uint32 (n_in,), number of clusters[, core bool (n_in,)][, counts uint32 (n_in,)])."""
        labels = np.empty(self.n_in, np.uint32)
        core = np.empty(self.n_in, np.uint8) if want_core else None
        counts = np.empty(self.n_in, np.uint32) if want_counts else None
        nclusters = C.c_uint64(0)
        check(self._lib.pcpx_cluster_self(self._h, float(radius), int(min_pts), _capi.PCPX_CLUSTER_COMPACT if compact else 0, _vp(labels),
                                          _vp(core), _vp(counts), C.byref(nclusters)))
        out = (labels, int(nclusters.value))
        if want_core:
            out += (core.astype(bool),)
        if want_counts:
            out += (counts,)
        return out

    def cluster_dev(self, radius, d_labels, min_pts=1, compact=True, d_core=None, d_counts=None, d_cluster_count=None):
        """Device form (pointers to device arrays by input row: labels uint32, core uint8, counts uint32; d_cluster_count one
        uint64), enqueued on the index's stream."""
        check(self._lib.pcpx_cluster_self_dev(self._h, float(radius), int(min_pts), _capi.PCPX_CLUSTER_COMPACT if compact else 0,
                                              C.c_void_p(d_labels) if d_labels else None,
                                              *(C.c_void_p(d) if d else None for d in (d_core, d_counts, d_cluster_count))))

    # ---- smooth-surface segmentation (include/pcpx_segment.h) ----
    @staticmethod
    def _segment_threshold(max_angle, min_cos):
        """min_cos as the C ABI takes it: given, or float32(cos(float64(max_angle))) of an angle in radians; exactly one of the two"""
        if (max_angle is None) == (min_cos is None):
            raise ValueError("give exactly one of max_angle and min_cos")
        return float(np.float32(np.cos(np.float64(max_angle)))) if min_cos is None else float(min_cos)

    @staticmethod
    def _segment_flags(oriented, compact):
        return (_capi.PCPX_SEGMENT_COMPACT if compact else 0) | (_capi.PCPX_SEGMENT_ORIENTED if oriented else 0)

    def segment(self, normals, radius, max_angle=None, min_cos=None, curvature=None, max_curvature=float("inf"), min_size=1, oriented=False,
                compact=True, want_smooth=False):
        """Smooth surface patches of the indexed cloud (normal-constrained region growing in its order-independent form): two points
        are joined iff one is in the other's sphere (the rule of range_count_self) and their normals agree, |n_i . n_j| >= min_cos
        in float32 (oriented: n_i . n_j >= min_cos); `normals` (n_in x 3) are used as given.  Segments are the connected
        components of the smooth points -- all indexed points, or with `curvature` (n_in) those with curvature <= max_curvature;
        a non-smooth point joins the smallest-labelled compatible smooth point in its sphere; segments of fewer than min_size rows,
        unreached points and points outside the voxel grid are noise: label 0xFFFFFFFF.  max_angle (radians) is converted as
        float32(cos(float64(max_angle))).  compact: labels 0 ... S-1 ordered by representative, else the representative itself
        (the segment's smallest smooth input index).
        Returns (labels uint32 (n_in,), number of segments[, smooth bool (n_in,)])."""
        threshold = self._segment_threshold(max_angle, min_cos)
        nrm = _f32(normals, 3)
        if len(nrm) != self.n_in:
            raise ValueError("one normal per input point")
        curv = None
        if curvature is not None:
            curv = _f32(curvature).reshape(-1)
            if len(curv) != self.n_in:
                raise ValueError("one curvature per input point")
        labels = np.empty(self.n_in, np.uint32)
        smooth = np.empty(self.n_in, np.uint8) if want_smooth else None
        nsegments = C.c_uint64(0)
        check(self._lib.pcpx_segment_self(self._h, _vp(nrm), _vp(curv), float(radius), threshold, float(max_curvature), int(min_size),
                                          self._segment_flags(oriented, compact), _vp(labels), _vp(smooth), C.byref(nsegments)))
        out = (labels, int(nsegments.value))
        if want_smooth:
            out += (smooth.astype(bool),)
        return out

    def segment_dev(self, d_normals, radius, d_labels, max_angle=None, min_cos=None, d_curvature=None, max_curvature=float("inf"), min_size=1,
                    oriented=False, compact=True, d_smooth=None, d_segment_count=None):
        """Device form (pointers to device arrays by input row: normals float32 x 3, curvature float32, labels uint32, smooth uint8;
        d_segment_count one uint64), enqueued on the index's stream."""
        check(self._lib.pcpx_segment_self_dev(self._h, *(C.c_void_p(d) if d else None for d in (d_normals, d_curvature)), float(radius),
                                              self._segment_threshold(max_angle, min_cos), float(max_curvature), int(min_size),
                                              self._segment_flags(oriented, compact),
                                              *(C.c_void_p(d) if d else None for d in (d_labels, d_smooth, d_segment_count))))

    # ---- Poisson-disk subsampling (include/pcpx_subsample.h) ----
    def subsample(self, radius, seed=0, want_keep=False, want_owner=False, want_rounds=False):
        """The subsample in which no two points are within `radius` of each other and every dropped indexed point has a kept point
        within `radius`: the kept set of the greedy loop that visits the points in ascending fmix32(input index ^ seed) and keeps a
        point iff no kept point is in its sphere (the rule of range_count_self).  A point outside the voxel grid is dropped;
        radius 0 keeps one point of every set of exact duplicates.  Returns the kept input indices, ascending (uint32)[, the keep
        mask bool (n_in,)][, owners uint32 (n_in,): the kept point in the row's sphere of smallest (d2, index), the row itself if it
        is kept, 0xFFFFFFFF outside the grid][, the round launches issued]."""
        keep = np.empty(self.n_in, np.uint8)
        owner = np.empty(self.n_in, np.uint32) if want_owner else None
        kept = np.empty(self.n_in, np.uint32)
        count = C.c_uint64(0)
        rounds = C.c_uint32(0)
        check(self._lib.pcpx_subsample_self(self._h, float(radius), int(seed) & 0xFFFFFFFF, 0, _vp(keep), _vp(owner), _vp(kept), C.byref(count),
                                            C.byref(rounds)))
        out = (kept[:int(count.value)].copy(),)
        if want_keep:
            out += (keep.astype(bool),)
        if want_owner:
            out += (owner,)
        if want_rounds:
            out += (int(rounds.value),)
        return out[0] if len(out) == 1 else out

    def subsample_dev(self, radius, d_keep, seed=0, d_owner=None, d_kept_rows=None, d_kept_count=None):
        """Device form (pointers to device arrays: keep uint8 and owner uint32 by input row, kept_rows uint32 with room for n_in
        entries, d_kept_count one uint64).  Synchronises the index's stream between rounds; what follows the last round is only
        enqueued.  Returns the round launches issued."""
        rounds = C.c_uint32(0)
        check(self._lib.pcpx_subsample_self_dev(self._h, float(radius), int(seed) & 0xFFFFFFFF, 0, C.c_void_p(d_keep) if d_keep else None,
                                                *(C.c_void_p(d) if d else None for d in (d_owner, d_kept_rows, d_kept_count)), C.byref(rounds)))
        return int(rounds.value)

    # ---- keypoints (include/pcpx_keypoints.h) ----
    @staticmethod
    def _dptr(d):
        """a device array as the C ABI takes it: None, an address, or anything with data_ptr() (a torch tensor)"""
        if d is None:
            return None
        addr = d.data_ptr() if hasattr(d, "data_ptr") else int(d)
        return C.c_void_p(addr) if addr else None

    def _kept_result(self, kept, count, keep, want_keep, extra=None):
        out = (kept[:int(count.value)].copy(),)
        if want_keep:
            out += (keep.astype(bool),)
        if extra is not None:
            out += (extra,)
        return out[0] if len(out) == 1 else out

    def local_maxima(self, score, radius, min_score=float("-inf"), min_neighbours=1, want_keep=False):
        """Sphere-wise non-maximum suppression: the points that are the maxima of `score` (n_in, float32) over `radius`.  A point is
        kept iff it is indexed, its score is not NaN and >= min_score, no other indexed point j in its sphere (the rule of
        range_count_self) beats it -- score_j > score_i, or score_j == score_i and j < i -- and its sphere holds at least
        min_neighbours points, itself included.  No two kept points are within `radius`; a dropped point need not have a kept one
        nearby (subsample promises that, this does not).  Minima: negate the score.
        Returns the kept input indices, ascending (uint32)[, the keep mask bool (n_in,)]."""
        s = _f32(score).reshape(-1)
        if len(s) != self.n_in:
            raise ValueError("one score per input point")
        keep = np.empty(self.n_in, np.uint8)
        kept = np.empty(self.n_in, np.uint32)
        count = C.c_uint64(0)
        check(self._lib.pcpx_local_maxima_self(self._h, _vp(s), float(radius), float(min_score), int(min_neighbours), 0, _vp(keep), _vp(kept),
                                               C.byref(count)))
        return self._kept_result(kept, count, keep, want_keep)

    def local_maxima_dev(self, d_score, radius, d_keep, min_score=float("-inf"), min_neighbours=1, d_kept_rows=None, d_kept_count=None):
        """Device form (torch tensors or pointers to device arrays: score float32 and keep uint8 by input row, kept_rows uint32 with
        room for n_in entries, d_kept_count one uint64), enqueued on the index's stream with no synchronisation: a curvature or
        saliency that shape_features_self_dev or iss_keypoints_dev left on the device goes straight in."""
        check(self._lib.pcpx_local_maxima_self_dev(self._h, self._dptr(d_score), float(radius), float(min_score), int(min_neighbours), 0,
                                                   *(self._dptr(d) for d in (d_keep, d_kept_rows, d_kept_count))))

    def iss_keypoints(self, salient_radius, non_max_radius, gamma21=0.975, gamma32=0.975, min_neighbours=5, want_saliency=False,
                      want_keep=False):
        """ISS keypoints (Zhong 2009) of the indexed cloud: with l0 <= l1 <= l2 and count of shape_features_self(salient_radius), the
        saliency of a point is l0 / count where l1 < gamma21 l2 and l0 < gamma32 l1 and NaN elsewhere (and outside the voxel grid);
        the keypoints are local_maxima(saliency, non_max_radius, min_neighbours=min_neighbours).
        Returns the kept input indices, ascending (uint32)[, the keep mask bool (n_in,)][, the saliency float32 (n_in,)]."""
        keep = np.empty(self.n_in, np.uint8)
        kept = np.empty(self.n_in, np.uint32)
        saliency = np.empty(self.n_in, np.float32) if want_saliency else None
        count = C.c_uint64(0)
        check(self._lib.pcpx_iss_keypoints_self(self._h, float(salient_radius), float(non_max_radius), float(gamma21), float(gamma32),
                                                int(min_neighbours), 0, _vp(keep), _vp(kept), C.byref(count), _vp(saliency)))
        return self._kept_result(kept, count, keep, want_keep, saliency)

    def iss_keypoints_dev(self, salient_radius, non_max_radius, d_keep, gamma21=0.975, gamma32=0.975, min_neighbours=5, d_kept_rows=None,
                          d_kept_count=None, d_saliency=None):
        """Device form (as local_maxima_dev; d_saliency float32 by input row), enqueued on the index's stream with no synchronisation."""
        check(self._lib.pcpx_iss_keypoints_self_dev(self._h, float(salient_radius), float(non_max_radius), float(gamma21), float(gamma32),
                                                    int(min_neighbours), 0, *(self._dptr(d) for d in (d_keep, d_kept_rows, d_kept_count, d_saliency))))

    # ---- outlier removal (include/pcpx_outliers.h) ----
    def _outlier_result(self, kept, count, keep, want_keep, *extras):
        out = (kept[:int(count.value)].copy(),)
        if want_keep:
            out += (keep.astype(bool),)
        out += tuple(e for e in extras if e is not None)
        return out[0] if len(out) == 1 else out

    def resolution(self, k=15, eps=1e-5, want_mean_dist=False):
        """The cloud's resolution: mean and sample standard deviation (float64, one fixed summation order: every bit depends on the
        cloud alone) of the mean distance to the k nearest neighbours over the usable rows -- indexed, with a finite mean distance.
        Returns (mean, std, usable)[, the mean distances float32 (n_in,), NaN outside the voxel grid]."""
        stats = np.empty(4, np.float64)
        d = np.empty(self.n_in, np.float32) if want_mean_dist else None
        check(self._lib.pcpx_outliers_resolution_self(self._h, int(k), float(eps), 0, _vp(d), _vp(stats)))
        out = (float(stats[0]), float(stats[1]), int(stats[3]))
        return out + (d,) if want_mean_dist else out

    def resolution_dev(self, d_stats, k=15, eps=1e-5, d_mean_dist=None):
        """Device form (d_stats: 4 float64 {mean, std, NaN, usable}; d_mean_dist float32 by input row), enqueued on the index's stream
        with no synchronisation."""
        check(self._lib.pcpx_outliers_resolution_self(self._h, int(k), float(eps), _capi.PCPX_OUTLIERS_ON_DEVICE, self._dptr(d_mean_dist),
                                                      self._dptr(d_stats)))

    def statistical_outliers(self, k=15, std_ratio=2.0, eps=1e-5, want_keep=False, want_mean_dist=False, want_stats=False):
        """Statistical outlier removal: keeps the usable rows whose mean distance d to their k nearest neighbours is
        <= float32(mean + std_ratio * std), mean and std as resolution(k) gives them.
        Returns the kept input indices, ascending (uint32)[, the keep mask bool (n_in,)][, d float32 (n_in,)][, stats float64 (4,):
        mean, std, the cut, the usable rows]."""
        keep = np.empty(self.n_in, np.uint8)
        kept = np.empty(self.n_in, np.uint32)
        d = np.empty(self.n_in, np.float32) if want_mean_dist else None
        stats = np.empty(4, np.float64) if want_stats else None
        count = C.c_uint64(0)
        check(self._lib.pcpx_outliers_statistical_self(self._h, int(k), float(eps), float(std_ratio), 0, _vp(keep), _vp(kept), C.byref(count),
                                                       _vp(d), _vp(stats)))
        return self._outlier_result(kept, count, keep, want_keep, d, stats)

    def statistical_outliers_dev(self, d_keep, k=15, std_ratio=2.0, eps=1e-5, d_kept_rows=None, d_kept_count=None, d_mean_dist=None,
                                 d_stats=None):
        """Device form (torch tensors or pointers to device arrays: keep uint8 by input row, kept_rows uint32 with room for n_in
        entries, d_kept_count one uint64, d_mean_dist float32 by input row, d_stats 4 float64), enqueued on the index's stream with
        no synchronisation."""
        check(self._lib.pcpx_outliers_statistical_self(self._h, int(k), float(eps), float(std_ratio), _capi.PCPX_OUTLIERS_ON_DEVICE,
                                                       *(self._dptr(d) for d in (d_keep, d_kept_rows, d_kept_count, d_mean_dist, d_stats))))

    def radius_outliers(self, radius, min_neighbours=5, want_keep=False, want_counts=False):
        """Radius outlier removal: keeps the indexed points whose sphere (the rule of range_count_self, the point itself included)
        holds at least max(min_neighbours, 1) points.  Without the counts the walk stops a point at the bound.
        Returns the kept input indices, ascending (uint32)[, the keep mask bool (n_in,)][, the counts uint32 (n_in,)]."""
        keep = np.empty(self.n_in, np.uint8)
        kept = np.empty(self.n_in, np.uint32)
        cnt = np.empty(self.n_in, np.uint32) if want_counts else None
        count = C.c_uint64(0)
        check(self._lib.pcpx_outliers_radius_self(self._h, float(radius), int(min_neighbours), 0, _vp(keep), _vp(kept), C.byref(count), _vp(cnt)))
        return self._outlier_result(kept, count, keep, want_keep, cnt)

    def radius_outliers_dev(self, radius, d_keep, min_neighbours=5, d_kept_rows=None, d_kept_count=None, d_count=None):
        """Device form (as statistical_outliers_dev; d_count uint32 by input row), enqueued on the index's stream."""
        check(self._lib.pcpx_outliers_radius_self(self._h, float(radius), int(min_neighbours), _capi.PCPX_OUTLIERS_ON_DEVICE,
                                                  *(self._dptr(d) for d in (d_keep, d_kept_rows, d_kept_count, d_count))))

    def density_outliers(self, k=15, radius_scale=1.0, min_neighbours=5, eps=1e-5, want_keep=False, want_counts=False, want_stats=False):
        """The reference's filter_point_cloud_noise_by_density in one call: radius_outliers at float32(radius_scale * mean) with the
        mean of resolution(k); the radius stays on the device.
        Returns the kept input indices, ascending (uint32)[, the keep mask][, the counts][, stats float64 (4,): mean, std, the radius,
        the usable rows]."""
        keep = np.empty(self.n_in, np.uint8)
        kept = np.empty(self.n_in, np.uint32)
        cnt = np.empty(self.n_in, np.uint32) if want_counts else None
        stats = np.empty(4, np.float64) if want_stats else None
        count = C.c_uint64(0)
        check(self._lib.pcpx_outliers_density_self(self._h, int(k), float(eps), float(radius_scale), int(min_neighbours), 0, _vp(keep), _vp(kept),
                                                   C.byref(count), _vp(cnt), _vp(stats)))
        return self._outlier_result(kept, count, keep, want_keep, cnt, stats)

    def density_outliers_dev(self, d_keep, k=15, radius_scale=1.0, min_neighbours=5, eps=1e-5, d_kept_rows=None, d_kept_count=None, d_count=None,
                             d_stats=None):
        """Device form (as radius_outliers_dev; d_stats 4 float64), enqueued on the index's stream."""
        check(self._lib.pcpx_outliers_density_self(self._h, int(k), float(eps), float(radius_scale), int(min_neighbours),
                                                   _capi.PCPX_OUTLIERS_ON_DEVICE,
                                                   *(self._dptr(d) for d in (d_keep, d_kept_rows, d_kept_count, d_count, d_stats))))

    # ---- boundary points (include/pcpx_boundary.h) ----
    def boundary(self, normals, radius, gap_sectors=16, min_neighbours=1, want_keep=False, want_gap=False, want_counts=False,
                 want_sectors=False):
        """Boundary points by the angle criterion (PCL's BoundaryEstimation): the rim of an open surface, the edges of its holes.  The
        directions from a point to the points of its sphere (the rule of range_count_self) are projected into the plane of its normal
        (`normals`: n_in x 3, float32, used as given) and sorted into 64 sectors of 5.625 degrees; G is the longest cyclic run of
        empty sectors.  A point is kept iff it is indexed, its normal is finite and not zero, its sphere holds at least
        max(min_neighbours, 1) points and G >= gap_sectors (1 .. 64; 16: an empty angle of 90 degrees or more).  Exact: every bit
        depends on the cloud and the normals alone (include/pcpx_boundary.h).
        Returns the kept input indices, ascending (uint32)[, the keep mask bool (n_in,)][, uint8 (n_in, 2): G and the sector the gap
        starts at, 255 255 where there is no frame][, the counts uint32 (n_in,)][, the sector masks uint64 (n_in,)]."""
        nrm = _f32(normals, 3)
        if len(nrm) != self.n_in:
            raise ValueError("one normal per input point")
        keep = np.empty(self.n_in, np.uint8)
        kept = np.empty(self.n_in, np.uint32)
        gap =np.empty((self.n_in, 2), np.uint8) if want_gap else None
        cnt = np.empty(self.n_in, np.uint32) if want_counts else None
        sectors = np.empty(self.n_in, np.uint64) if want_sectors else None
        count = C.c_uint64(0)
        check(self._lib.pcpx_boundary_self(self._h, _vp(nrm), float(radius), int(gap_sectors), int(min_neighbours), 0, _vp(keep), _vp(kept),
                                           C.byref(count), _vp(gap), _vp(cnt), _vp(sectors)))
        return self._outlier_result(kept, count, keep, want_keep, gap, cnt, sectors)

    def boundary_dev(self, d_normals, radius, d_keep, gap_sectors=16, min_neighbours=1, d_kept_rows=None, d_kept_count=None, d_gap=None,
                     d_count=None, d_sectors=None):
        """Device form (torch tensors or pointers to device arrays: normals float32 n_in x 3 and keep uint8 by input row, kept_rows
        uint32 with room for n_in entries, d_kept_count one uint64, d_gap uint8 n_in x 2, d_count uint32 and d_sectors uint64 by
        input row), enqueued on the index's stream with no synchronisation: the normals that range_neighbourhoods_self_dev left on the
        device go straight in, and the kept rows straight on into Index.from_device and cluster."""
        check(self._lib.pcpx_boundary_self(self._h, self._dptr(d_normals), float(radius), int(gap_sectors), int(min_neighbours),
                                           _capi.PCPX_BOUNDARY_ON_DEVICE,
                                           *(self._dptr(d) for d in (d_keep, d_kept_rows, d_kept_count, d_gap, d_count, d_sectors))))

    # ---- farthest point sampling (include/pcpx_fps.h) ----
    @staticmethod
    def _fps_params(flags, start, stop_radius):
        return _capi.FpsParams(flags, _capi.PCPX_FPS_START_LOWEST if start is None else int(start), float(stop_radius), 0)

    def farthest_points(self, m, start=None, stop_radius=0.0, want_d2=False, want_min_d2=False, want_owner=False, want_evaluations=False):
        """Farthest point sampling: up to `m` indexed points, each the one farthest (squared distance by the rule of
        range_count_self; among equals the lowest input index) from the samples before it, from `start` on (an input row; None: the
        lowest indexed row; a row outside the voxel grid selects nothing).  The selection ends early when no point is farther than
        `stop_radius` from the samples -- with 0, when every point coincides with a sample.  Exact: every bit depends on the cloud
        and the arguments alone (include/pcpx_fps.h).
        Returns the selected input indices in selection order (uint32, count of them)[, float32 (count,): each sample's squared
        distance to the samples before it, the first +inf][, float32 (n_in,): every row's squared distance to its nearest sample,
        +inf outside the grid][, uint32 (n_in,): the ordinal of the earliest nearest sample, 0xFFFFFFFF outside the grid][, the
        number of squared distances formed: a diagnostic]."""
        m = int(m)
        most = min(m, self.n_in)
        rows = np.empty(max(most, 1), np.uint32)  # (never NULL: m > 0 on an empty cloud is a valid call)
        d2 = np.empty(most, np.float32) if want_d2 else None
        min_d2 = np.empty(self.n_in, np.float32) if want_min_d2 else None
        owner = np.empty(self.n_in, np.uint32) if want_owner else None
        count, evaluations = C.c_uint64(0), C.c_uint64(0)
        params = self._fps_params(0, start, stop_radius)
        # (the library writes [0, count), count <= min(m, indexed points): arrays of min(m, n_in) entries hold them)
        check(self._lib.pcpx_farthest_points_self(self._h, m, C.byref(params), _vp(rows),
                                                  C.addressof(count), _vp(d2), _vp(min_d2), _vp(owner),
                                                  C.addressof(evaluations) if want_evaluations else None))
        k = int(count.value)
        out = (rows[:k].copy(),)
        if want_d2:
            out += (d2[:k].copy(),)
        if want_min_d2:
            out += (min_d2,)
        if want_owner:
            out += (owner,)
        if want_evaluations:
            out += (int(evaluations.value),)
        return out[0] if len(out) == 1 else out

    def farthest_points_dev(self, m, d_rows, d_count, start=None, stop_radius=0.0, d_d2=None, d_min_d2=None, d_owner=None, d_evaluations=None):
        """Device form (torch tensors or pointers to device arrays: d_rows uint32 and d_d2 float32 with room for m entries, of which
        [0, count) are written; d_count and d_evaluations one uint64 each; d_min_d2 float32 and d_owner uint32 by input row),
        enqueued on the index's stream: min(m, indexed points) launches and a few more, no read-back and no synchronisation between
        samples -- the stop rule is applied on the device.  The rows go straight on into a gather for a torch model or into
        Index.from_device."""
        params = self._fps_params(_capi.PCPX_FPS_ON_DEVICE, start, stop_radius)
        check(self._lib.pcpx_farthest_points_self(self._h, int(m), C.byref(params),
                                                  *(self._dptr(d) for d in (d_rows, d_count, d_d2, d_min_d2, d_owner, d_evaluations))))

    # ---- descriptors (include/pcpx_descriptors.h) ----
    def fpfh(self, normals, radius, rows=None, want_spfh=False):
        """Fast Point Feature Histograms (Rusu et al. 2009) over `radius` from `normals` (n_in x 3, float32, used as given): 33 floats
        per described point -- three blocks of 11 bins (the angle of the target's normal about the source's, the v component of the
        target's normal, the source's normal along the line), each scaled to sum 100 -- the 1 / d^2-weighted sum of the neighbours'
        simplified histograms.  rows: distinct input indices to describe (default: every input row); a row outside the voxel grid or
        >= n_in gets zeros.
        Returns fpfh float32 (m, 33)[, spfh float32 (n_in, 33), pairs uint32 (n_in,): by input row, and with `rows` zero except at
        the points that some described row's sphere holds]."""
        nrm = _f32(normals).reshape(-1)
        if len(nrm) != 3 * self.n_in:
            raise ValueError("one normal per input point")
        sel = None if rows is None else np.ascontiguousarray(rows, np.uint32).reshape(-1)
        m = self.n_in if sel is None else len(sel)
        out = np.empty((m, 33), np.float32)
        spfh = np.empty((self.n_in, 33), np.float32) if want_spfh else None
        pairs = np.empty(self.n_in, np.uint32) if want_spfh else None
        held = sel if sel is None or len(sel) else np.zeros(1, np.uint32)  # (an empty selection still passes an address: NULL means every row)
        check(self._lib.pcpx_fpfh_self(self._h, _vp(nrm), float(radius), _vp(held), 0 if sel is None else m, 0, _vp(out), _vp(spfh), _vp(pairs)))
        return (out, spfh, pairs) if want_spfh else out

    def fpfh_dev(self, d_normals, radius, d_fpfh, d_rows=None, m=0, d_spfh=None, d_pairs=None):
        """Device form (torch tensors or pointers to device arrays: normals float32 (n_in, 3); rows uint32, m of them -- the kept rows
        that iss_keypoints_dev left on the device go straight in; fpfh float32 (m, 33), or (n_in, 33) without rows; spfh float32
        (n_in, 33) and pairs uint32 (n_in,)), enqueued on the index's stream with no synchronisation."""
        check(self._lib.pcpx_fpfh_self_dev(self._h, self._dptr(d_normals), float(radius), self._dptr(d_rows), int(m) if d_rows is not None else 0, 0,
                                           *(self._dptr(d) for d in (d_fpfh, d_spfh, d_pairs))))

    # ---- iterative closest point (include/pcpx_icp.h) ----
    @staticmethod
    def _pose16(pose):
        if pose is None:
            return None
        p = np.ascontiguousarray(pose, dtype=np.float64).reshape(-1)
        if p.size != 16:
            raise ValueError("pose must be 4 x 4")
        return p

    def nearest_posed(self, source, radius, pose=None, want_d2=False):
        """The exact nearest indexed point of every row of `source` ((m, 3) float32-convertible) moved by `pose` ((4, 4) float64,
        source -> this cloud; None: the identity) among those within `radius`: the smallest (d2, input index), so ties go to the
        lowest input index.  Returns partner uint32 (m,) -- 0xFFFFFFFF where there is none -- [, d2 float32 (m,), +inf there]."""
        s = _f32(source, 3)
        partner = np.empty(len(s), np.uint32)
        d2 = np.empty(len(s), np.float32) if want_d2 else None
        check(self._lib.pcpx_nearest_posed(self._h, _vp(s) if len(s) else None, len(s), _vp(self._pose16(pose)), float(radius), _vp(partner), _vp(d2)))
        return (partner, d2) if want_d2 else partner

    def nearest_posed_dev(self, d_source, m, radius, d_partner, d_pose=None, d_d2=None):
        """Device form (torch tensors or device addresses: source float32 (m, 3), pose 16 float64 or None, partner uint32 (m,), d2
        float32 (m,)), enqueued on the index's stream with no synchronisation."""
        check(self._lib.pcpx_nearest_posed_dev(self._h, self._dptr(d_source), int(m), self._dptr(d_pose), float(radius), self._dptr(d_partner),
                                               self._dptr(d_d2)))

    def icp(self, source, radius, pose=None, max_iterations=50, normals=None, want_partner=False):
        """Iterative closest point of `source` onto this cloud from `pose` (None: the identity): nearest partners within `radius`
        under the pose, a new pose from the pairs, until the partner list repeats.  Point to point (Horn's least-squares fit over the
        pairs, always of the original source) or, with `normals` ((n_in, 3) float32 by input row of this cloud), point to plane.
        Returns a dict: "transform" ((4, 4) float64), "status" (0 = max_iterations reached, 1 = converged: the partners repeated,
        2 = too few partners, 3 = degenerate normal equations), "iterations" (pose updates made), "last_count" (partners in the
        last search), "count" and "rms" (per update, length iterations)[, "partner" uint32 (m,): the last partner list]."""
        s = _f32(source, 3)
        nrm = None
        if normals is not None:
            nrm = _f32(normals).reshape(-1)
            if len(nrm) != 3 * self.n_in:
                raise ValueError("one normal per input point")
        it = int(max_iterations)
        xf = np.empty(16, np.float64)
        words = [C.c_uint32(0) for _ in range(3)]
        count, rms = np.empty(max(it, 1), np.uint32), np.empty(max(it, 1), np.float64)
        partner = np.empty(len(s), np.uint32) if want_partner else None
        check(self._lib.pcpx_icp_rigid(self._h, _vp(s) if len(s) else None, len(s), _vp(self._pose16(pose)), float(radius), it,
                                       _capi.PCPX_ICP_POINT_TO_PLANE if nrm is not None else 0, _vp(nrm), _vp(xf), *(C.byref(w) for w in words), _vp(count),
                                       _vp(rms), _vp(partner)))
        done = words[1].value
        out = {"transform": xf.reshape(4, 4), "status": words[0].value, "iterations": done, "last_count": words[2].value,
               "count": count[:done].copy(), "rms": rms[:done].copy()}
        if want_partner:
            out["partner"] = partner
        return out

    def icp_dev(self, d_source, m, radius, d_transform, d_pose=None, max_iterations=50, d_normals=None, d_status=None, d_iterations=None,
                d_last_count=None, d_count=None, d_rms=None, d_partner=None):
        """Device form: source float32 (m, 3); pose 16 float64 -- the refit array of ransac_rigid_dev goes straight in -- or None;
        normals float32 (n_in, 3) for point to plane; transform 16 float64; status / iterations / last_count one uint32 each; count
        uint32 and rms float64 with room for max_iterations; partner uint32 (m,).  All max_iterations rounds are enqueued on the
        index's stream with no synchronisation and no read-back."""
        check(self._lib.pcpx_icp_rigid_dev(self._h, self._dptr(d_source), int(m), self._dptr(d_pose), float(radius), int(max_iterations),
                                           _capi.PCPX_ICP_POINT_TO_PLANE if d_normals is not None else 0,
                                           *(self._dptr(d) for d in (d_normals, d_transform, d_status, d_iterations, d_last_count, d_count, d_rms,
                                                                     d_partner))))

    # ---- Generalized ICP (include/pcpx_gicp.h) ----
    def gicp(self, source, radius, source_normals=None, normals=None, epsilon=1e-3, pose=None, max_iterations=50, source_cov=None, cov=None,
             want_partner=False):
        """Generalized ICP of `source` onto this cloud from `pose` (None: the identity): the loop of icp() with a plane-to-plane
        step -- a pair's residual is weighted by the inverse of C_target + R C_source R^T.  Either both clouds' normals
        (`source_normals` (m, 3) by source row, `normals` (n_in, 3) by input row of this cloud; neither oriented nor unit length
        needed) with `epsilon` in (0, 1], the variance along a normal relative to the variance across it; or both clouds'
        covariances (`source_cov` (m, 6), `cov` (n_in, 6): the upper triangles xx, xy, xz, yy, yz, zz), with which epsilon is not
        used.  Returns icp()'s dict; "rms" is the root mean Mahalanobis residual over the usable rows."""
        s = _f32(source, 3)
        by_cov = source_cov is not None or cov is not None
        if by_cov and (source_normals is not None or normals is not None):
            raise ValueError("normals or covariances, not both")
        a, b, width = (source_cov, cov, 6) if by_cov else (source_normals, normals, 3)
        if a is None or b is None:
            raise ValueError("both clouds' normals, or both clouds' covariances")
        a, b = _f32(a).reshape(-1), _f32(b).reshape(-1)
        if len(a) != width * len(s) or len(b) != width * self.n_in:
            raise ValueError("one row of %d per source point and per input point" % width)
        if not len(b):
            b = np.zeros(width, np.float32)  # (an empty target still passes an address: nothing is read through it)
        it = int(max_iterations)
        xf = np.empty(16, np.float64)
        words = [C.c_uint32(0) for _ in range(3)]
        count, rms = np.empty(max(it, 1), np.uint32), np.empty(max(it, 1), np.float64)
        partner = np.empty(len(s), np.uint32) if want_partner else None
        check(self._lib.pcpx_gicp_rigid(self._h, _vp(s) if len(s) else None, len(s), _vp(self._pose16(pose)), float(radius), it,
                                        _capi.PCPX_GICP_COVARIANCES if by_cov else 0, _vp(a) if len(s) else None, _vp(b),
                                        0.0 if by_cov else float(epsilon), _vp(xf), *(C.byref(w) for w in words), _vp(count), _vp(rms), _vp(partner)))
        done = words[1].value
        out = {"transform": xf.reshape(4, 4), "status": words[0].value, "iterations": done, "last_count": words[2].value,
               "count": count[:done].copy(), "rms": rms[:done].copy()}
        if want_partner:
            out["partner"] = partner
        return out

    def gicp_dev(self, d_source, m, radius, d_transform, d_source_normals=None, d_normals=None, epsilon=1e-3, d_pose=None, max_iterations=50,
                 d_source_cov=None, d_cov=None, d_status=None, d_iterations=None, d_last_count=None, d_count=None, d_rms=None, d_partner=None):
        """Device form (pcpx_gicp_rigid with PCPX_GICP_ON_DEVICE): the arrays of icp_dev, and float32 normals ((m, 3) and (n_in, 3) -- what range_neighbourhoods_self_dev left on
        the device goes straight in) or covariances ((m, 6) and (n_in, 6)).  All max_iterations rounds are enqueued on the index's
        stream with no synchronisation and no read-back."""
        by_cov = d_source_cov is not None or d_cov is not None
        if by_cov and (d_source_normals is not None or d_normals is not None):
            raise ValueError("normals or covariances, not both")
        a, b = (d_source_cov, d_cov) if by_cov else (d_source_normals, d_normals)
        check(self._lib.pcpx_gicp_rigid(self._h, self._dptr(d_source), int(m), self._dptr(d_pose), float(radius), int(max_iterations),
                                        _capi.PCPX_GICP_ON_DEVICE | (_capi.PCPX_GICP_COVARIANCES if by_cov else 0), self._dptr(a), self._dptr(b),
                                        0.0 if by_cov else float(epsilon),
                                        *(self._dptr(d) for d in (d_transform, d_status, d_iterations, d_last_count, d_count, d_rms, d_partner))))

    # ---- normals ----
    def normals_knn_self(self, k, eps=1e-5, want_knn=False):
        nrm = np.empty((self.n_in, 3), np.float32)
        idx = np.empty((self.n_in, k), np.uint32) if want_knn else None
        cnt = np.empty(self.n_in, np.uint32) if want_knn else None
        check(self._lib.pcpx_normals_knn_self(self._h, k, eps, _vp(nrm), _vp(idx), _vp(cnt)))
        return (nrm, idx, cnt) if want_knn else nrm

    def normals_knn_self_curve_order(self, k, eps=1e-5, want_normals=True):
        """(normals, idx, cnt, perm, position_of) with the rows in curve order: row p belongs to input point perm[p]; position_of is
        the inverse table (0xFFFFFFFF for a point outside the voxel grid).  The copies overlap the kernels (include/pcpx.h)."""
        n, n_in = self.size(), self.n_in
        nrm = np.empty((n, 3), np.float32) if want_normals else None
        idx = np.empty((n, k), np.uint32)
        cnt = np.empty(n, np.uint32)
        perm = np.empty(n, np.uint32)
        pos = np.empty(n_in, np.uint32)
        check(self._lib.pcpx_normals_knn_self_curve_order(self._h, k, eps, _vp(nrm), _vp(idx), _vp(cnt), _vp(perm), _vp(pos)))
        return nrm, idx, cnt, perm, pos

    def oriented_normals_knn_self(self, k, eps=1e-5, want_knn=False):
        """estimate_normals followed by propagate_normal_orientations, both on the GPU (the rows stay there).
        Returns normals (and rows, counts if want_knn) plus the number of points reached from the root."""
        n = self.n_in
        nrm = np.empty((n, 3), np.float32)
        idx = np.empty((n, k), np.uint32) if want_knn else None
        cnt = np.empty(n, np.uint32) if want_knn else None
        reached = C.c_uint64(0)
        check(self._lib.pcpx_oriented_normals_knn_self(self._h, k, eps, _vp(nrm), _vp(idx) if want_knn else None,
                                                       _vp(cnt) if want_knn else None, C.byref(reached)))
        return (nrm, idx, cnt, int(reached.value)) if want_knn else (nrm, int(reached.value))

    def orient_normals_knn_self(self, normals, k, eps=1e-5):
        """propagate_normal_orientations for normals the caller has (n x 3, input order); kNN graph built on the GPU."""
        out = np.array(normals, dtype=np.float32, order="C", copy=True).reshape(-1, 3)
        if out.shape[0] != self.n_in:
            raise ValueError("normals must be n x 3")
        reached = C.c_uint64(0)
        check(self._lib.pcpx_orient_normals_knn_self(self._h, k, eps, _vp(out), C.byref(reached)))
        return out, int(reached.value)

    def tangent_planes_knn_self(self, k, eps=1e-5):
        """pcp::algorithm::estimate_tangent_planes: (centroids, normals) of every point's k-neighbourhood."""
        cen = np.empty((self.n_in, 3), np.float32)
        nrm = np.empty((self.n_in, 3), np.float32)
        check(self._lib.pcpx_tangent_planes_knn_self(self._h, k, eps, _vp(cen), _vp(nrm)))
        return cen, nrm

    def tangent_plane_sdf(self, centroids, normals, grid, eps=1e-5):
        """The tangent-plane signed distance at every corner of `grid` (surface.tangent_plane_sdf)."""
        from . import surface
        return surface.tangent_plane_sdf(self, centroids, normals, grid, eps)

    def reconstruct_surface(self, k, dims, eps=1e-5, isovalue=0.0, want_planes=False):
        """Tangent-plane surface reconstruction in one call: (vertices (V,3) float32, triangles (T,3) uint32)
        (surface.reconstruct_surface)."""
        from . import surface
        return surface.reconstruct_surface(self, k, dims, eps, isovalue, want_planes)

    def mean_knn_distance_self(self, k, eps=1e-5):
        """pcp::algorithm::average_distances_to_neighbors: mean distance to the k nearest neighbours, per point."""
        out = np.empty(self.n_in, np.float32)
        check(self._lib.pcpx_mean_knn_distance_self(self._h, k, eps, _vp(out)))
        return out

    def surface_hint(self, xyz, k, eps=1e-5):
        """The hint of the example's `graph` meshing variant (examples/tangent_plane_surface_reconstruction.cpp:393-445) for
        surface_nets_from_hint: the densest point -- the smallest mean distance to its k nearest neighbours, the first index on
        a tie (std::min_element) -- and the centroid of its k nearest neighbours, summed from zero in row order.  xyz: the
        indexed points, in input order."""
        xyz = _f32(xyz, 3)
        if len(xyz) != self.n_in:
            raise ValueError("xyz must be the %d indexed points" % self.n_in)
        mean = self.mean_knn_distance_self(k, eps)
        densest = int(np.argmin(np.where(np.isnan(mean), np.float32(np.inf), mean)))
        idx, cnt = self.knn(xyz[densest:densest + 1], k, eps)
        acc = np.zeros(3, np.float32)
        for j in idx[0, :int(cnt[0])]:
            acc = (acc + xyz[j]).astype(np.float32)
        return (acc / np.float32(cnt[0])).astype(np.float32)

    def normals_from_knn(self, nbr, cnt, want_evals=False):
        nbr = np.ascontiguousarray(nbr, np.uint32)
        cnt = np.ascontiguousarray(cnt, np.uint32)
        nq, k = nbr.shape
        nrm = np.empty((nq, 3), np.float32)
        ev = np.empty((nq, 3), np.float32) if want_evals else None
        check(self._lib.pcpx_normals_from_knn(self._h, _vp(nbr), _vp(cnt), nq, k, _vp(nrm), _vp(ev)))
        return (nrm, ev) if want_evals else nrm

    # ---- device-pointer forms (torch tensors / raw pointers), used by bench.py ----
    @classmethod
    def from_device(cls, d_xyz_ptr, n, device=0, stream=None, voxel_grid=None, coarse_order=False, shard=None, k_hint=0, borrow=False, shard_range=None):
        self = cls.__new__(cls)
        self._lib = _capi.load()
        self._h = C.c_void_p(None)
        self.device = device
        self.n_in = n
        check(self._lib.pcpx_index_create_dev(C.c_void_p(d_xyz_ptr), n, cls._params(voxel_grid, coarse_order, shard, k_hint, borrow, shard_range), device,
                                              C.c_void_p(stream) if stream else None, C.byref(self._h)))
        return self

    def rebuild_dev(self, d_xyz_ptr, n, voxel_grid=None, coarse_order=False, shard=None, k_hint=0, borrow=False, shard_range=None):
        check(self._lib.pcpx_index_rebuild_dev(self._h, C.c_void_p(d_xyz_ptr), n, self._params(voxel_grid, coarse_order, shard, k_hint, borrow, shard_range)))
        self.n_in = n

    def knn_self_curve_order_dev(self, k, eps, d_idx, d_cnt, d_d2=None, d_normals=None, first=0, count=_capi.UINT64_MAX):
        """Rows by curve position (row p = the p-th point of the curve order = input point perm[p], perm_dev)."""
        check(self._lib.pcpx_knn_self_curve_order_dev(self._h, k, eps, first, count, C.c_void_p(d_idx), C.c_void_p(d_cnt),
                                                      C.c_void_p(d_d2) if d_d2 else None, C.c_void_p(d_normals) if d_normals else None))

    def perm_dev(self, d_perm=None, d_position_of=None):
        check(self._lib.pcpx_index_perm_dev(self._h, C.c_void_p(d_perm) if d_perm else None, C.c_void_p(d_position_of) if d_position_of else None))

    def knn_self_dev(self, k, eps, d_idx, d_cnt, d_d2=None, first=0, count=_capi.UINT64_MAX):
        check(self._lib.pcpx_knn_self_dev(self._h, k, eps, first, count, C.c_void_p(d_idx), C.c_void_p(d_cnt),
                                          C.c_void_p(d_d2) if d_d2 else None))

    def knn_self_strided_dev(self, k, eps, row_stride, d_idx, d_cnt, d_d2=None, first=0, count=_capi.UINT64_MAX):
        """knn_self_dev with row_stride entries between rows (16 for k = 15 / 16: a row is one aligned 64-byte piece)."""
        check(self._lib.pcpx_knn_self_strided_dev(self._h, k, eps, first, count, row_stride, C.c_void_p(d_idx), C.c_void_p(d_cnt),
                                                  C.c_void_p(d_d2) if d_d2 else None))

    def normals_knn_self_strided_dev(self, k, eps, row_stride, d_normals, d_idx=None, d_cnt=None, first=0, count=_capi.UINT64_MAX):
        check(self._lib.pcpx_normals_knn_self_strided_dev(self._h, k, eps, first, count, row_stride, C.c_void_p(d_normals),
                                                          C.c_void_p(d_idx) if d_idx else None, C.c_void_p(d_cnt) if d_cnt else None))

    def knn_group_costs(self, k, eps=1e-5, group_stride=16):
        """pcpx_knn_group_costs_dev: event counts (nsamples x 4, uint32, on the host) of one query group in every group_stride of the
        curve order -- what shard_cuts_by_cost cuts by.  Deterministic: every rank gets the same table from the same cloud and grid."""
        ns = C.c_uint64(0)
        st = self._lib.pcpx_knn_group_costs_dev(self._h, k, eps, group_stride, None, 0, C.byref(ns))
        if st not in (_capi.PCPX_OK, _capi.PCPX_ERR_CAPACITY):
            check(st)
        out = np.zeros((int(ns.value), 4), np.uint32)
        if ns.value == 0:
            return out
        d = C.c_void_p(None)
        check(self._lib.pcpx_device_malloc(out.nbytes, self.device, C.byref(d)))
        try:
            check(self._lib.pcpx_knn_group_costs_dev(self._h, k, eps, group_stride, d, ns.value, C.byref(ns)))
            self.synchronize()
            check(self._lib.pcpx_device_download(_vp(out), d, out.nbytes, self.device, None))
        finally:
            self._lib.pcpx_device_free(d, self.device)
        return out

    def debug_set(self, name, value):
        """pcpx_debug_set: 'long_groups_first', 'gather_outputs', 'icp_resort', 'fps_bucket_height', 'fps_prune', 'fps_one_block' (how work is done, never what comes out); 'poison' (a byte):
        fills everything that is scratch by contract, of the handle, its device's pool and the idle index blocks (include/pcpx.h)."""
        check(self._lib.pcpx_debug_set(self._h, name.encode(), int(value)))

    def debug_get(self, name):
        """pcpx_debug_get: 'build_redos', 'full_buckets', 'schedule_state', 'poisoned_bytes', 'poisoned_shared_bytes', 'poisoned_cache_bytes',
        'scratch_bytes', 'knn_row_form'."""
        v = C.c_int64(0)
        check(self._lib.pcpx_debug_get(self._h, name.encode(), C.byref(v)))
        return int(v.value)

    def debug_group_times(self):
        """Ticks / 64 per query group of the last recorded self-kNN launch (uint32 array; empty: nothing recorded)."""
        ng = C.c_uint64(0)
        st = self._lib.pcpx_debug_group_times(self._h, None, 0, C.byref(ng))
        if st not in (_capi.PCPX_OK, _capi.PCPX_ERR_CAPACITY):
            check(st)
        out = np.zeros(int(ng.value), np.uint32)
        if ng.value:
            check(self._lib.pcpx_debug_group_times(self._h, _vp(out), ng.value, C.byref(ng)))
        return out

    def debug_tree(self):
        """pcpx_debug_tree (for tests): the structure the last build left, as host arrays.  A dict of n (indexed points), nleaves, depth,
        written (nodes the build writes per level 0 ... depth), leaves (nleaves x 32 uint32: x[8], y[8], z[8], id[8] as bits), nodes
        (heap order x 8 uint32: lo[3], hi[3], poison, 0 as bits; defined are written[d] nodes from (4^d - 1) / 3 of every level) and
        first_pass (256 uint32; zeros: the last build sorted nothing)."""
        shape = (C.c_uint64 * 20)()
        fp = np.zeros(256, np.uint32)
        st = self._lib.pcpx_debug_tree(self._h, shape, None, 0, None, 0, fp.ctypes.data_as(_capi.u32p))
        if st not in (_capi.PCPX_OK, _capi.PCPX_ERR_CAPACITY):
            check(st)
        nleaves, depth, nnodes = int(shape[1]), int(shape[2]), int(shape[3])
        leaves = np.zeros((nleaves, 32), np.uint32)
        nodes = np.zeros((nnodes, 8), np.uint32)
        # (never a null array pointer, also for an empty tree: NULL asks for the sizes)
        spare = np.zeros(8, np.uint32)
        check(self._lib.pcpx_debug_tree(self._h, shape, _vp(leaves if nleaves else spare), nleaves, _vp(nodes if nnodes else spare), nnodes,
                                        fp.ctypes.data_as(_capi.u32p)))
        return {"n": int(shape[0]), "nleaves": nleaves, "depth": depth, "written": [int(shape[4 + d]) for d in range(depth + 1)] if nleaves else [],
                "leaves": leaves, "nodes": nodes, "first_pass": fp}

    def knn_batch_dev(self, d_queries, nq, k, eps, d_idx, d_cnt, d_d2=None):
        """kNN of nq arbitrary device-resident query points (curve-sorted internally, rows in query order)."""
        check(self._lib.pcpx_knn_batch_dev(self._h, d_queries, nq, k, eps, d_idx, d_cnt, d_d2))

    def normals_knn_self_dev(self, k, eps, d_normals, d_idx=None, d_cnt=None, first=0, count=_capi.UINT64_MAX):
        check(self._lib.pcpx_normals_knn_self_dev(self._h, k, eps, first, count, C.c_void_p(d_normals),
                                                  C.c_void_p(d_idx) if d_idx else None,
                                                  C.c_void_p(d_cnt) if d_cnt else None))

    def neighbourhoods_self_dev(self, k, eps, d_normals=None, d_centroids=None, d_meandist=None, first=0, count=_capi.UINT64_MAX):
        """Per-neighbourhood products of every indexed point's k nearest neighbours, in input order: PCA normals (n x 3),
        centroids (n x 3), mean Euclidean distances (n; NaN for an empty row).  Any output may be None, not all."""
        check(self._lib.pcpx_neighbourhoods_self_dev(self._h, k, eps, first, count, C.c_void_p(d_normals) if d_normals else None,
                                                     C.c_void_p(d_centroids) if d_centroids else None,
                                                     C.c_void_p(d_meandist) if d_meandist else None))

    def range_count_self_dev(self, radius, d_cnt, first=0, count=_capi.UINT64_MAX):
        check(self._lib.pcpx_range_count_self_dev(self._h, radius, first, count, C.c_void_p(d_cnt)))

    def range_count_self_curve_order_dev(self, radius, d_cnt, first=0, count=_capi.UINT64_MAX):
        """Counts at curve positions (d_cnt[p] = count around the p-th point of the index's order; perm_dev gives the order)."""
        check(self._lib.pcpx_range_count_self_curve_order_dev(self._h, radius, first, count, C.c_void_p(d_cnt)))

    def range_lists_self_dev(self, radius, d_offsets, d_idx=None, capacity=0):
        """pcpx_range_lists_self_dev: CSR lists of every indexed point's sphere range, device resident.  Returns the total; with d_idx
        None (or too small) only the offsets are filled -- allocate `total` indices and call again."""
        total = C.c_uint64(0)
        st = self._lib.pcpx_range_lists_self_dev(self._h, radius, C.c_void_p(d_offsets), C.c_void_p(d_idx) if d_idx else None, capacity, C.byref(total))
        if st != _capi.PCPX_OK and not (st == _capi.PCPX_ERR_CAPACITY and (not d_idx or capacity < total.value)):
            check(st)
        return int(total.value)

    def synchronize(self):
        check(self._lib.pcpx_index_synchronize(self._h))

    def debug_eps_test_mode(self, mode):
        """0: automatic; 1: eps-box test on buffered keys (compaction); 2: on every candidate.  Same results, different cost."""
        check(self._lib.pcpx_debug_eps_test_mode(self._h, int(mode)))

    def debug_knn_stats(self, k, eps=1e-5, want_waves=False, floor=False):
        """floor=True: every lane starts from its true k-th distance (what a perfect visiting order could reach)."""
        cap = 16 + 5 * 65536
        out = (C.c_uint64 * cap)()
        check(self._lib.pcpx_debug_knn_stats(self._h, k, eps, out, cap | ((1 << 63) if floor else 0)))
        names = ["leaves", "expansions", "compactions", "appended", "waves", "seed_leaves", "second_round_groups",
                 "cycles_walk", "cycles_compact", "cycles_leaf", "cycles_search_loop", "cycles_group",
                 "seed_compactions", "seed_appended", "sparse_leaves", "sparse_leaf_lanes"]
        d = {n: int(out[i]) for i, n in enumerate(names)}
        d["cycles_later_rounds"] = int(out[cap - 8])   # walk rounds after a group's first (lanes whose k-th distance lay beyond the cap)
        d["lanes_in_later_rounds"] = int(out[cap - 7])
        if want_waves:
            w = np.frombuffer(out, dtype=np.uint64)[16:16 + 5 * 65534].reshape(-1, 5)  # (the last two records' words hold the round-4 counters)
            d["wave_times"] = w[w[:, 1] > 0].copy()
        return d

    def profile_begin(self):
        check(self._lib.pcpx_profile_begin(self._h))

    def profile_end(self):
        """{family: (launches, total_ms)} from hipEvents recorded on the index's stream."""
        p = _capi.Profile()
        check(self._lib.pcpx_profile_end(self._h, C.byref(p)))
        names = ["build", "knn", "normals", "range", "query_prep"]
        return {n: (int(p.launches[i]), float(p.total_ms[i])) for i, n in enumerate(names)}


class LinkedOctree(Index):
    """pcp::basic_linked_octree_t over index elements.  node_capacity / max_depth are accepted for
    signature parity (include/pcp/octree/linked_octree_node.hpp:31-40) but do not shape the GPU
    structure: only query results are observable."""

    def __init__(self, xyz, node_capacity=32, max_depth=21, voxel_grid=None, device=0):
        assert node_capacity > 0 and max_depth > 0  # linked_octree_node.hpp:87-88
        super().__init__(xyz, voxel_grid=voxel_grid, device=device)

    def voxel_grid(self):
        return self.bbox()

    def nearest_neighbours(self, targets, k, eps=1e-5):
        return self.knn(targets, k, eps)

    def range_search(self, centers, radius):
        return self.range_sphere(centers, radius)


class LinkedKdTree(Index):
    """pcp::basic_linked_kdtree_t over index elements (construction_params_t accepted, unused)."""

    def __init__(self, xyz, max_depth=12, compute_max_depth=False, max_elements_per_leaf=64, device=0):
        super().__init__(xyz, voxel_grid=None, device=device)

    def aabb(self):
        return self.bbox()

    def nearest_neighbours(self, targets, k, eps=1e-5):
        return self.knn(targets, k, eps)

    def range_search(self, centers, radius):
        return self.range_sphere(centers, radius)


class KdTreeK:
    """pcp::basic_linked_kdtree_t for K > 3 coordinates (4 ... 16): nearest_neighbours and range_search with a kd box, by
    exhaustive search on the GPU (include/pcpx.h: pcpx_kd_*; csrc/pcpx_kd.hip).  K <= 3 goes through LinkedKdTree."""

    def __init__(self, points, device=0):
        pts = np.ascontiguousarray(points, dtype=np.float32)
        if pts.ndim != 2:
            raise ValueError("points: an (n, K) array")
        self.n_in, self.dims = int(pts.shape[0]), int(pts.shape[1])
        self._lib = _capi.load()
        h = C.c_void_p()
        check(self._lib.pcpx_kd_create(_vp(pts), self.n_in, self.dims, device, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pcpx_kd_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def size(self):
        return int(self._lib.pcpx_kd_size(self._h))

    def nearest_neighbours(self, targets, k, eps=1e-5, want_d2=False):
        """(idx (nq, k) uint32 padded with 0xFFFFFFFF, count (nq,)[, d2 (nq, k) padded with +inf]): ascending (d2, index)."""
        q = _f32(targets, self.dims)
        idx = np.empty((len(q), k), np.uint32)
        cnt = np.empty(len(q), np.uint32)
        d2 = np.empty((len(q), k), np.float32) if want_d2 else None
        check(self._lib.pcpx_kd_knn_batch(self._h, _vp(q), len(q), k, eps, _vp(idx), _vp(cnt), _vp(d2)))
        return (idx, cnt, d2) if want_d2 else (idx, cnt)

    def range_search(self, boxes):
        """CSR (offsets, indices) of the points inside each kd box; boxes (nb, 2 K): min then max."""
        b = _f32(boxes, 2 * self.dims)
        off = np.zeros(len(b) + 1, np.uint64)
        st = self._lib.pcpx_kd_range_aabb_batch(self._h, _vp(b), len(b), _vp(off), None, 0)
        if st == _capi.PCPX_OK:
            return off, np.empty(0, np.uint32)
        if st != _capi.PCPX_ERR_CAPACITY:
            check(st)
        out = np.empty(int(off[-1]), np.uint32)
        check(self._lib.pcpx_kd_range_aabb_batch(self._h, _vp(b), len(b), _vp(off), _vp(out), len(out)))
        return off, out


def estimate_normals(tree, k, eps=1e-5):
    """pcp::algorithm::estimate_normals with knn_map = tree.nearest_neighbours(point, k): one normal
    per indexed point (examples/simple_example.cpp:83-99)."""
    return tree.normals_knn_self(k, eps)


def propagate_normal_orientations_dev(d_xyz, n, d_knn_idx, d_knn_count, k, d_normals, device=0, stream=None):
    """Device-pointer form (level-synchronous search on the GPU, same flips as the host form); returns
    (vertices reached, BFS depth).  Normals are updated in place."""
    reached, levels = C.c_uint64(0), C.c_uint32(0)
    check(_capi.load().pcpx_propagate_normal_orientations_dev(d_xyz, n, d_knn_idx, d_knn_count, k, d_normals, device, stream,
                                                              C.byref(reached), C.byref(levels)))
    return int(reached.value), int(levels.value)


def propagate_normal_orientations(points, knn_idx, normals, knn_count=None):
    """pcp::algorithm::propagate_normal_orientations (include/pcp/algorithm/estimate_normals.hpp:187-302) over
    the kNN rows the query kernels return (knn_idx n x k, optional per-row counts): root = first point of
    largest z with normal (0,0,1), breadth-first flips.  Returns (oriented normals, vertices reached)."""
    pts = _f32(points, 3)
    nbr = np.ascontiguousarray(knn_idx, dtype=np.uint32)
    if nbr.ndim != 2 or nbr.shape[0] != pts.shape[0]:
        raise ValueError("knn_idx must be n x k")
    out = np.array(normals, dtype=np.float32, order="C", copy=True).reshape(-1, 3)
    if out.shape[0] != pts.shape[0]:
        raise ValueError("normals must be n x 3")
    cnt = None if knn_count is None else np.ascontiguousarray(knn_count, dtype=np.uint32)
    reached = C.c_uint64(0)
    check(_capi.load().pcpx_propagate_normal_orientations(_vp(pts), pts.shape[0], _vp(nbr), None if cnt is None else _vp(cnt),
                                                          nbr.shape[1], _vp(out), C.byref(reached)))
    return out, int(reached.value)
