"""Surface reconstruction over the C ABI: pcp::common::regular_grid3d_t / regular_grid_containing
(include/pcp/common/regular_grid3d.hpp) and pcp::algorithm::isosurface::surface_nets
(include/pcp/algorithm/surface_nets.hpp:357-650, the overload that marches over the whole grid; :653-1119, the overload with a
hint point, is surface_nets_from_hint).

A field holds one value per grid corner, corner (i, j, k) at i + j*(sx+1) + k*(sx+1)*(sy+1): a numpy array of shape
(sz+1, sy+1, sx+1) or anything of that many float32 values.  Meshes are (vertices (V, 3) float32, triangles (T, 3) uint32).
Host arrays in, host arrays out; torch tensors on the GPU in, torch tensors out (the device-pointer entry points).
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import Grid3d, check


def _grid_of(grid):
    if isinstance(grid, Grid3d):
        return grid
    g = Grid3d()
    for name in ("x", "y", "z", "dx", "dy", "dz", "sx", "sy", "sz"):
        setattr(g, name, getattr(grid, name))
    return g


def grid3d(x, y, z, dx, dy, dz, sx, sy, sz):
    """A Grid3d from its nine values (origin, voxel size, voxels per axis)."""
    return Grid3d(float(x), float(y), float(z), float(dx), float(dy), float(dz), int(sx), int(sy), int(sz))


def corners_shape(grid):
    """Shape of a field over `grid`: (sz+1, sy+1, sx+1), x fastest."""
    return (int(grid.sz) + 1, int(grid.sy) + 1, int(grid.sx) + 1)


def corner_positions(grid):
    """World positions of every corner in field order ((sx+1)(sy+1)(sz+1) x 3 float32), computed as get_world_point_of."""
    nz, ny, nx = corners_shape(grid)
    f = np.float32
    x = f(grid.x) + np.arange(nx, dtype=np.float32) * f(grid.dx)
    y = f(grid.y) + np.arange(ny, dtype=np.float32) * f(grid.dy)
    z = f(grid.z) + np.arange(nz, dtype=np.float32) * f(grid.dz)
    zz, yy, xx = np.meshgrid(z, y, x, indexing="ij")
    return np.stack([xx.ravel(), yy.ravel(), zz.ravel()], axis=1).astype(np.float32)


def regular_grid_containing(min3, max3, dims):
    """pcp::common::regular_grid_containing (regular_grid3d.hpp:63-90), quirk included: the origin moves back by dx on
    every axis."""
    lo = np.ascontiguousarray(min3, np.float32).reshape(3)
    hi = np.ascontiguousarray(max3, np.float32).reshape(3)
    d = np.ascontiguousarray(dims, np.uint64).reshape(3)
    g = Grid3d()
    check(_capi.load().pcpx_regular_grid_containing(lo.ctypes.data_as(_capi.f32p), hi.ctypes.data_as(_capi.f32p),
                                                     d.ctypes.data_as(_capi.u64p), C.byref(g)))
    return g


def _is_device_tensor(a):
    return hasattr(a, "data_ptr") and getattr(a, "is_cuda", False)


def _corners(grid):
    return (int(grid.sx) + 1) * (int(grid.sy) + 1) * (int(grid.sz) + 1)


def surface_nets(field, grid, isovalue=0.0, device=0):
    """Naive surface nets of `field` at `isovalue` (positive corners: s >= isovalue).  Vertices in ascending cube index,
    triangles in (cube, quad, triangle) order; every grid cube meshed once."""
    lib = _capi.load()
    g = _grid_of(grid)
    nv, nt = C.c_uint64(0), C.c_uint64(0)
    if _is_device_tensor(field):
        import torch
        if field.dtype != torch.float32 or not field.is_contiguous() or field.numel() != _corners(g):
            raise ValueError("field must be a contiguous float32 tensor of (sx+1)(sy+1)(sz+1) values")
        dev = field.device.index or 0
        stream = torch.cuda.current_stream(field.device).cuda_stream
        st = lib.pcpx_surface_nets_dev(C.c_void_p(field.data_ptr()), C.byref(g), float(isovalue), dev, C.c_void_p(stream), None, 0, None, 0,
                                       C.byref(nv), C.byref(nt))
        if st not in (_capi.PCPX_OK, _capi.PCPX_ERR_CAPACITY):
            check(st)
        v = torch.empty((nv.value, 3), dtype=torch.float32, device=field.device)
        t = torch.empty((nt.value, 3), dtype=torch.int32, device=field.device)  # (uint32 vertex indices)
        if st == _capi.PCPX_ERR_CAPACITY:
            check(lib.pcpx_surface_nets_dev(C.c_void_p(field.data_ptr()), C.byref(g), float(isovalue), dev, C.c_void_p(stream),
                                            C.c_void_p(v.data_ptr()), nv.value, C.c_void_p(t.data_ptr()), nt.value, C.byref(nv), C.byref(nt)))
        return v, t
    f = np.ascontiguousarray(field, np.float32).ravel()
    if f.size != _corners(g) and min(g.sx, g.sy, g.sz) > 0:
        raise ValueError("field has %d values, the grid %d corners" % (f.size, _corners(g)))
    st = lib.pcpx_surface_nets(f.ctypes.data_as(C.c_void_p), C.byref(g), float(isovalue), device, None, 0, None, 0, C.byref(nv), C.byref(nt))
    if st not in (_capi.PCPX_OK, _capi.PCPX_ERR_CAPACITY):
        check(st)
    v = np.empty((nv.value, 3), np.float32)
    t = np.empty((nt.value, 3), np.uint32)
    if st == _capi.PCPX_ERR_CAPACITY:
        check(lib.pcpx_surface_nets(f.ctypes.data_as(C.c_void_p), C.byref(g), float(isovalue), device, v.ctypes.data_as(C.c_void_p), nv.value,
                                    t.ctypes.data_as(C.c_void_p), nt.value, C.byref(nv), C.byref(nt)))
    return v, t


def surface_nets_from_hint(field, grid, hint, isovalue=0.0, queue_max=32768, with_seed=False, device=0):
    """Surface nets of the connected component that the reference's search from `hint` reaches first (pcpx_surface_nets_hint,
    DESIGN.md section 15): the whole-grid mesh restricted to that component, vertices in ascending cube index.  queue_max: the
    reference's breadth_first_search_queue_max_size (0: no bound).  with_seed: also the seed's linear cube index, or None
    where the search fell back to the whole grid (or found no active cube)."""
    lib = _capi.load()
    g = _grid_of(grid)
    h = np.ascontiguousarray(hint, np.float32).reshape(3)
    hp = h.ctypes.data_as(_capi.f32p)
    nv, nt, seed = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    if _is_device_tensor(field):
        import torch
        if field.dtype != torch.float32 or not field.is_contiguous() or field.numel() != _corners(g):
            raise ValueError("field must be a contiguous float32 tensor of (sx+1)(sy+1)(sz+1) values")
        dev = field.device.index or 0
        stream = torch.cuda.current_stream(field.device).cuda_stream

        def call(v, t):
            return lib.pcpx_surface_nets_hint_dev(C.c_void_p(field.data_ptr()), C.byref(g), float(isovalue), hp, int(queue_max), dev,
                                                  C.c_void_p(stream), None if v is None else C.c_void_p(v.data_ptr()),
                                                  0 if v is None else len(v), None if t is None else C.c_void_p(t.data_ptr()),
                                                  0 if t is None else len(t), C.byref(nv), C.byref(nt), C.byref(seed))
        st = call(None, None)
        if st not in (_capi.PCPX_OK, _capi.PCPX_ERR_CAPACITY):
            check(st)
        v = torch.empty((nv.value, 3), dtype=torch.float32, device=field.device)
        t = torch.empty((nt.value, 3), dtype=torch.int32, device=field.device)  # (uint32 vertex indices)
        if st == _capi.PCPX_ERR_CAPACITY:
            check(call(v, t))
    else:
        f = np.ascontiguousarray(field, np.float32).ravel()
        if f.size != _corners(g) and min(g.sx, g.sy, g.sz) > 0:
            raise ValueError("field has %d values, the grid %d corners" % (f.size, _corners(g)))

        def call(v, t):
            return lib.pcpx_surface_nets_hint(f.ctypes.data_as(C.c_void_p), C.byref(g), float(isovalue), hp, int(queue_max), device,
                                              None if v is None else v.ctypes.data_as(C.c_void_p), 0 if v is None else len(v),
                                              None if t is None else t.ctypes.data_as(C.c_void_p), 0 if t is None else len(t),
                                              C.byref(nv), C.byref(nt), C.byref(seed))
        st = call(None, None)
        if st not in (_capi.PCPX_OK, _capi.PCPX_ERR_CAPACITY):
            check(st)
        v = np.empty((nv.value, 3), np.float32)
        t = np.empty((nt.value, 3), np.uint32)
        if st == _capi.PCPX_ERR_CAPACITY:
            check(call(v, t))
    if not with_seed:
        return v, t
    return v, t, None if seed.value == _capi.UINT64_MAX else int(seed.value)


def surface_nets_hint_raw(field, grid, hint, isovalue, queue_max, vertex_capacity, triangle_capacity, device=0):
    """pcpx_surface_nets_hint with explicit capacities: (status, V, T, vertices, triangles, seed), the arrays sized by the
    capacities."""
    lib = _capi.load()
    g = _grid_of(grid)
    f = np.ascontiguousarray(field, np.float32).ravel()
    h = np.ascontiguousarray(hint, np.float32).reshape(3)
    v = np.zeros((vertex_capacity, 3), np.float32)
    t = np.zeros((triangle_capacity, 3), np.uint32)
    nv, nt, seed = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    st = lib.pcpx_surface_nets_hint(f.ctypes.data_as(C.c_void_p), C.byref(g), float(isovalue), h.ctypes.data_as(_capi.f32p), int(queue_max),
                                    device, v.ctypes.data_as(C.c_void_p), vertex_capacity, t.ctypes.data_as(C.c_void_p), triangle_capacity,
                                    C.byref(nv), C.byref(nt), C.byref(seed))
    return st, int(nv.value), int(nt.value), v, t, int(seed.value)


def search_order(queue_max):
    """The hint search's table (pcpx_surface_nets_search_order): ((N, 3) int32 offsets from the hint cube in the reference's
    first-pop order, bounded)."""
    lib = _capi.load()
    n, b = C.c_uint64(0), C.c_int(0)
    st = lib.pcpx_surface_nets_search_order(int(queue_max), None, 0, C.byref(n), C.byref(b))
    if st not in (_capi.PCPX_OK, _capi.PCPX_ERR_CAPACITY):
        check(st)
    out = np.zeros((n.value, 3), np.int32)
    if n.value:
        check(lib.pcpx_surface_nets_search_order(int(queue_max), out.ctypes.data_as(C.c_void_p), n.value, C.byref(n), C.byref(b)))
    return out, bool(b.value)


def surface_nets_raw(field, grid, isovalue, vertex_capacity, triangle_capacity, device=0):
    """pcpx_surface_nets with explicit capacities (the capacity protocol as the C ABI has it): (status, V, T, vertices,
    triangles), the arrays sized by the capacities."""
    lib = _capi.load()
    g = _grid_of(grid)
    f = np.ascontiguousarray(field, np.float32).ravel()
    if f.size != _corners(g):
        raise ValueError("field has %d values, the grid %d corners" % (f.size, _corners(g)))
    v = np.zeros((vertex_capacity, 3), np.float32)
    t = np.zeros((triangle_capacity, 3), np.uint32)
    nv, nt = C.c_uint64(0), C.c_uint64(0)
    st = lib.pcpx_surface_nets(f.ctypes.data_as(C.c_void_p), C.byref(g), float(isovalue), device, v.ctypes.data_as(C.c_void_p), vertex_capacity,
                               t.ctypes.data_as(C.c_void_p), triangle_capacity, C.byref(nv), C.byref(nt))
    return st, int(nv.value), int(nt.value), v, t


def tangent_plane_sdf(index, centroids, normals, grid, eps=1e-5):
    """The example's signed-distance function at every corner: dot(c - o_j, n_j), j the 1-NN of corner c (eps-box
    exclusion).  Host arrays: a numpy field of shape (sz+1, sy+1, sx+1); GPU tensors: a flat GPU tensor."""
    lib = _capi.load()
    g = _grid_of(grid)
    ncorner = _corners(g)
    if _is_device_tensor(centroids):
        import torch
        out = torch.empty(ncorner, dtype=torch.float32, device=centroids.device)
        check(lib.pcpx_tangent_plane_sdf_dev(index._h, C.c_void_p(centroids.data_ptr()), C.c_void_p(normals.data_ptr()), C.byref(g), float(eps),
                                             C.c_void_p(out.data_ptr())))
        return out
    cen = np.ascontiguousarray(centroids, np.float32).reshape(-1, 3)
    nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    if len(cen) != index.n_in or len(nrm) != index.n_in:
        raise ValueError("centroids and normals must be n x 3")
    out = np.empty(corners_shape(g), np.float32)
    bufs = []
    try:
        for nbytes in (cen.nbytes, nrm.nbytes, out.nbytes):
            p = C.c_void_p(None)
            check(lib.pcpx_device_malloc(max(nbytes, 16), index.device, C.byref(p)))
            bufs.append(p)
        check(lib.pcpx_device_upload(bufs[0], cen.ctypes.data_as(C.c_void_p), cen.nbytes, index.device, None))
        check(lib.pcpx_device_upload(bufs[1], nrm.ctypes.data_as(C.c_void_p), nrm.nbytes, index.device, None))
        check(lib.pcpx_tangent_plane_sdf_dev(index._h, bufs[0], bufs[1], C.byref(g), float(eps), bufs[2]))
        check(lib.pcpx_device_download(out.ctypes.data_as(C.c_void_p), bufs[2], out.nbytes, index.device, None))
    finally:
        for p in bufs:
            lib.pcpx_device_free(p, index.device)
    return out


def reconstruct_surface(index, k, dims, eps=1e-5, isovalue=0.0, want_planes=False):
    """Tangent-plane surface reconstruction (examples/tangent_plane_surface_reconstruction.cpp:233-455) in one call:
    (vertices, triangles), plus (centroids, oriented normals, grid) with want_planes."""
    lib = _capi.load()
    d = np.ascontiguousarray(dims, np.uint64).reshape(3)
    nv, nt = C.c_uint64(0), C.c_uint64(0)
    g = Grid3d()
    cen = np.empty((index.n_in, 3), np.float32) if want_planes else None
    nrm = np.empty((index.n_in, 3), np.float32) if want_planes else None

    def call(v, t):
        return lib.pcpx_reconstruct_surface(index._h, int(k), float(eps), d.ctypes.data_as(_capi.u64p), float(isovalue),
                                            v.ctypes.data_as(C.c_void_p) if v is not None else None, 0 if v is None else len(v),
                                            t.ctypes.data_as(C.c_void_p) if t is not None else None, 0 if t is None else len(t),
                                            C.byref(nv), C.byref(nt), cen.ctypes.data_as(C.c_void_p) if want_planes else None,
                                            nrm.ctypes.data_as(C.c_void_p) if want_planes else None, C.byref(g))

    st = call(None, None)
    if st not in (_capi.PCPX_OK, _capi.PCPX_ERR_CAPACITY):
        check(st)
    v = np.empty((nv.value, 3), np.float32)
    t = np.empty((nt.value, 3), np.uint32)
    if st == _capi.PCPX_ERR_CAPACITY:
        check(call(v, t))
    return (v, t, cen, nrm, g) if want_planes else (v, t)
