"""ctypes view of oracle/_ref/libpcp_ref.so, a build of the reference's own headers -- TEST INFRASTRUCTURE ONLY.

build() compiles it (oracle/Makefile, target _ref/libpcp_ref.so) where the reference's source tree exists: $PCP_REFERENCE,
else the Makefile's default.  Without the source, a library already built into oracle/_ref/ is used; without either,
available() is False.  See oracle/pcp_ref.cpp for what each entry point instantiates.  GPU tests never import this module:
they read the outputs it recorded under tests/golden/ (tests/golden/make_reference_golden.py).
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_ref", "libpcp_ref.so")
_LIB = None
_WHY = None

_f32p = C.POINTER(C.c_float)
_u32p = C.POINTER(C.c_uint32)
_u64p = C.POINTER(C.c_uint64)
NONE = np.uint32(0xFFFFFFFF)


def reference_dir():
    """$PCP_REFERENCE, else a checkout named `reference` beside this repository (the Makefile's default)."""
    return os.path.abspath(os.environ.get("PCP_REFERENCE", os.path.join(_HERE, "..", "..", "reference")))


def build():
    """Build _ref/libpcp_ref.so if the reference source exists; returns the library's path or None."""
    global _WHY
    if os.path.isdir(os.path.join(reference_dir(), "include", "pcp")):
        r = subprocess.run(["make", "-C", _HERE, "PCP_REFERENCE=" + reference_dir(), "_ref/libpcp_ref.so"],
                           stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            _WHY = "building _ref/libpcp_ref.so failed:\n" + r.stderr[-4000:]
            raise RuntimeError(_WHY)
    if os.path.exists(_SO):
        return _SO
    _WHY = "no reference source at %s (set PCP_REFERENCE) and no prebuilt oracle/_ref/libpcp_ref.so" % reference_dir()
    return None


def available():
    try:
        return lib() is not None
    except OSError as e:
        global _WHY
        _WHY = str(e)
        return False


def why_unavailable():
    return _WHY


def lib():
    global _LIB
    if _LIB is None:
        if build() is None:
            return None
        L = C.CDLL(_SO)
        for name in ("ref_octree_create", "ref_kd_create", "ref_surface_nets"):
            getattr(L, name).restype = C.c_void_p
        for name in ("ref_octree_size", "ref_octree_range_sphere", "ref_octree_range_aabb", "ref_kd_range_aabb"):
            getattr(L, name).restype = C.c_uint64
        L.ref_octree_create.argtypes = [_f32p, C.c_uint64, C.c_uint32, C.c_uint32, _f32p]
        L.ref_octree_destroy.argtypes = L.ref_kd_destroy.argtypes = L.ref_mesh_destroy.argtypes = [C.c_void_p]
        L.ref_octree_size.argtypes = [C.c_void_p]
        L.ref_octree_grid.argtypes = [C.c_void_p, _f32p]
        L.ref_octree_knn.argtypes = [C.c_void_p, _f32p, C.c_uint64, C.c_uint32, C.c_double, _u32p, _u32p, C.c_int]
        L.ref_octree_range_sphere.argtypes = [C.c_void_p, _f32p, C.c_float, _u32p, C.c_uint64]
        L.ref_octree_range_count_spheres.argtypes = [C.c_void_p, _f32p, _f32p, C.c_uint64, _u32p, C.c_int]
        L.ref_octree_range_aabb.argtypes = [C.c_void_p, _f32p, _u32p, C.c_uint64]
        L.ref_kd_create.argtypes = [C.c_uint64, _f32p, C.c_uint64, C.c_int, C.c_uint64, C.c_int, C.c_uint64]
        L.ref_kd_knn.argtypes = [C.c_void_p, C.c_uint64, _f32p, C.c_uint64, C.c_uint32, C.c_float, _u32p, _u32p, C.c_int]
        L.ref_kd_range_aabb.argtypes = [C.c_void_p, _f32p, _u32p, C.c_uint64]
        L.ref_average_distances.argtypes = [_f32p, C.c_uint64, _u32p, _u32p, C.c_uint32, _f32p]
        L.ref_surface_nets.argtypes = [_f32p, _f32p, _u64p, C.c_float, _f32p, C.c_uint64, C.c_int, C.c_float]
        L.ref_mesh_sizes.argtypes = [C.c_void_p, _u64p, _u64p]
        L.ref_mesh_copy.argtypes = [C.c_void_p, _f32p, _u32p]
        L.ref_wlop_from_sample.argtypes = [_f32p, C.c_uint64, _u64p, C.c_uint64, C.c_double, C.c_double, C.c_uint64, C.c_int, _f32p]
        L.ref_wlop_public.argtypes = [_f32p, C.c_uint64, C.c_uint64, C.c_double, C.c_double, C.c_uint64, C.c_int, _f32p]
        _LIB = L
    return _LIB


def _f32(a, cols=3):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, cols)


def _p(a, t):
    return a.ctypes.data_as(t) if a is not None else None


def _threads():
    return min(16, os.cpu_count() or 1)


class Octree:
    """pcp::basic_linked_octree_t<std::uint32_t> over point indices.  No voxel_grid and the default capacity and depth:
    the constructor that computes the bounding box (linked_octree.hpp:103-121); otherwise the explicit one (:83-91)."""

    def __init__(self, xyz, node_capacity=32, max_depth=21, voxel_grid=None):
        self.xyz = _f32(xyz)
        g = None if voxel_grid is None else _f32(np.asarray(voxel_grid).reshape(6), 6)
        self._h = C.c_void_p(lib().ref_octree_create(_p(self.xyz, _f32p), len(self.xyz), node_capacity, max_depth, _p(g, _f32p)))

    def __del__(self):
        try:
            lib().ref_octree_destroy(self._h)
        except Exception:
            pass

    def size(self):
        return int(lib().ref_octree_size(self._h))

    def voxel_grid(self):
        out = np.zeros(6, np.float32)
        lib().ref_octree_grid(self._h, _p(out, _f32p))
        return out

    def knn(self, queries, k, eps=1e-5):
        """nearest_neighbours(q, k, point_view, eps) per query: (idx (nq, k) padded with 0xFFFFFFFF, count (nq,))."""
        q = _f32(queries)
        idx = np.empty((len(q), k), np.uint32)
        cnt = np.empty(len(q), np.uint32)
        lib().ref_octree_knn(self._h, _p(q, _f32p), len(q), k, float(eps), _p(idx, _u32p), _p(cnt, _u32p), _threads())
        return idx, cnt

    def range_sphere(self, center, r):
        """Sorted indices inside sphere_t{center, r}."""
        c = _f32(center).reshape(3)
        out = np.empty(max(len(self.xyz), 1), np.uint32)
        n = lib().ref_octree_range_sphere(self._h, _p(c, _f32p), float(r), _p(out, _u32p), len(out))
        return out[:int(n)].copy()

    def range_counts(self, centers, radii):
        """Counts of sphere_t{centers[i], radii[i]} (a scalar radius for every sphere, or one radius per sphere)."""
        c = _f32(centers)
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(radii, np.float32), (len(c),)))
        cnt = np.empty(len(c), np.uint32)
        lib().ref_octree_range_count_spheres(self._h, _p(c, _f32p), _p(r, _f32p), len(c), _p(cnt, _u32p), _threads())
        return cnt

    def range_aabb(self, bmin, bmax):
        b = np.concatenate([np.asarray(bmin, np.float32).reshape(3), np.asarray(bmax, np.float32).reshape(3)])
        out = np.empty(max(len(self.xyz), 1), np.uint32)
        n = lib().ref_octree_range_aabb(self._h, _p(b, _f32p), _p(out, _u32p), len(out))
        return out[:int(n)].copy()


class KdTree:
    """pcp::basic_linked_kdtree_t<std::size_t, K, map> for K = points.shape[1] in 1 ... 16.  params None: the reference's
    default construction_params_t; else (max_depth, compute_max_depth, max_elements_per_leaf)."""

    def __init__(self, points, params=None):
        self.pts = np.ascontiguousarray(points, np.float32)
        self.dims = self.pts.shape[1]
        assert 1 <= self.dims <= 16
        md, cmd, leaf = params if params is not None else (12, False, 64)
        self._h = C.c_void_p(lib().ref_kd_create(self.dims, _p(self.pts, _f32p), len(self.pts), int(params is not None), md,
                                                 int(cmd), leaf))

    def __del__(self):
        try:
            lib().ref_kd_destroy(self._h)
        except Exception:
            pass

    def knn(self, queries, k, eps=1e-5):
        q = _f32(queries, self.dims)
        idx = np.empty((len(q), k), np.uint32)
        cnt = np.empty(len(q), np.uint32)
        lib().ref_kd_knn(self._h, self.dims, _p(q, _f32p), len(q), k, float(eps), _p(idx, _u32p), _p(cnt, _u32p), _threads())
        return idx, cnt

    def range_aabb(self, box):
        """box = (min[0..K), max[0..K)): sorted indices inside."""
        b = np.ascontiguousarray(box, np.float32).reshape(2 * self.dims)
        out = np.empty(max(len(self.pts), 1), np.uint32)
        n = lib().ref_kd_range_aabb(self._h, _p(b, _f32p), _p(out, _u32p), len(out))
        return out[:int(n)].copy()


def average_distances_to_neighbors(xyz, nbr, cnt):
    """pcp::algorithm::average_distances_to_neighbors with knn_map(i) = the first cnt[i] entries of row i."""
    xyz = _f32(xyz)
    nbr = np.ascontiguousarray(nbr, np.uint32)
    cnt = np.ascontiguousarray(cnt, np.uint32)
    out = np.empty(len(xyz), np.float32)
    lib().ref_average_distances(_p(xyz, _f32p), len(xyz), _p(nbr, _u32p), _p(cnt, _u32p), nbr.shape[1], _p(out, _f32p))
    return out


def _g(grid, name):
    return grid[name] if isinstance(grid, dict) else getattr(grid, name)


def surface_nets(field, grid, isovalue=0.0, hint=None, queue_max=32768, outside=None):
    """surface_nets(std::execution::seq, f, grid, isovalue), or the hint overload with hint given, over the corner array.
    outside: the value of f at positions outside the grid's box (the hint overload evaluates cubes past the faces); None
    makes any such evaluation abort.  Returns (vertices (V, 3) float32, triangles (T, 3) uint32) in the reference's order."""
    g6 = np.array([_g(grid, n) for n in ("x", "y", "z", "dx", "dy", "dz")], np.float32)
    s3 = np.array([_g(grid, n) for n in ("sx", "sy", "sz")], np.uint64)
    f = np.ascontiguousarray(field, np.float32).ravel()
    assert len(f) == int(np.prod(s3 + 1))
    h = None if hint is None else np.asarray(hint, np.float32).reshape(3).copy()
    L = lib()
    m = C.c_void_p(L.ref_surface_nets(_p(f, _f32p), _p(g6, _f32p), _p(s3, _u64p), float(isovalue), _p(h, _f32p), queue_max,
                                      int(outside is not None), float(0.0 if outside is None else outside)))
    try:
        nv, nt = C.c_uint64(0), C.c_uint64(0)
        L.ref_mesh_sizes(m, C.byref(nv), C.byref(nt))
        v = np.zeros((nv.value, 3), np.float32)
        t = np.zeros((nt.value, 3), np.uint32)
        L.ref_mesh_copy(m, _p(v, _f32p), _p(t, _u32p))
    finally:
        L.ref_mesh_destroy(m)
    return v, t


def wlop_from_sample(xyz, sample, mu, h, K, uniform=True):
    """The body of pcp::algorithm::wlop::wlop with the initial sample given (see ref_wlop_from_sample)."""
    xyz = _f32(xyz)
    sample = np.ascontiguousarray(sample, np.uint64)
    out = np.empty((len(sample), 3), np.float32)
    lib().ref_wlop_from_sample(_p(xyz, _f32p), len(xyz), _p(sample, _u64p), len(sample), float(mu), float(h), K, int(uniform),
                               _p(out, _f32p))
    return out


def wlop_public(xyz, I, mu, h, K, uniform=True):
    """pcp::algorithm::wlop::wlop itself (a random sample of I points)."""
    xyz = _f32(xyz)
    out = np.empty((I, 3), np.float32)
    lib().ref_wlop_public(_p(xyz, _f32p), len(xyz), I, float(mu), float(h), K, int(uniform), _p(out, _f32p))
    return out
