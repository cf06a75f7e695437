"""Hint-seeded surface nets without a GPU: the library's search table against the model's literal queue, the model on the
reference's own test case, and the drop-in overload's shape."""
import os
import subprocess

import numpy as np

import surface_nets_hint_model as H
import surface_nets_model as M
from conftest import ROOT

F = np.float32


def test_search_order_matches_the_literal_queue(pkg):
    """Q = 1024 stops after 398 pops and 120 cubes; Q = 32768 after 15 277 pops and 560 cubes, out to Manhattan distance 7
    (all of distances 0-6 and 183 of the 198 cubes at 7)."""
    for q, n in ((1024, 120), (32768, 560)):
        got, bounded = pkg.surface.search_order(q)
        want, want_bounded = H.search_order(q)
        assert bounded and want_bounded
        assert len(got) == n
        assert np.array_equal(got, np.asarray(want, np.int32))
    got, _ = pkg.surface.search_order(32768)
    d = np.abs(got).sum(1)
    assert np.all(np.diff(d) >= 0) and d.max() == 7
    assert (d < 7).sum() == 377 and (d == 7).sum() == 183  # 377 cubes within distance 6 of the origin


def test_search_order_unbounded(pkg):
    """Q = 64, 4096 and 0 are never the queue's size before a pop: the search has no bound, and the table is the first
    2^20 pops' distinct cubes, whole shells up to the last."""
    tables = []
    for q in (64, 4096, 0):
        got, bounded = pkg.surface.search_order(q)
        assert not bounded
        tables.append(got)
    assert all(np.array_equal(t, tables[0]) for t in tables)
    d = np.abs(tables[0]).sum(1)
    assert np.all(np.diff(d) >= 0)
    top = d.max()
    r = top - 1  # every cube within distance top - 1: (2r+1)(2r^2+2r+3)/3 of them
    assert (d <= r).sum() == (2 * r + 1) * (2 * r * r + 2 * r + 3) // 3
    # the bounded tables are prefixes of this order
    for q in (1024, 32768):
        b, _ = pkg.surface.search_order(q)
        assert np.array_equal(b, tables[0][:len(b)])


def test_search_order_capacity_protocol(pkg):
    import ctypes as C
    lib = pkg.surface._capi.load()
    n, b = C.c_uint64(0), C.c_int(0)
    out = np.full((200, 3), 7, np.int32)
    assert lib.pcpx_surface_nets_search_order(1024, out.ctypes.data_as(C.c_void_p), 119, C.byref(n), C.byref(b)) == -4
    assert (n.value, b.value) == (120, 1) and np.all(out == 7)
    assert lib.pcpx_surface_nets_search_order(1024, out.ctypes.data_as(C.c_void_p), 200, C.byref(n), C.byref(b)) == 0
    assert np.all(out[120:] == 7)
    # the queue holds one cube before the first pop: Q = 1 stops at once with an empty table
    assert lib.pcpx_surface_nets_search_order(1, None, 0, C.byref(n), C.byref(b)) == 0 and (n.value, b.value) == (0, 1)
    assert lib.pcpx_surface_nets_search_order(1024, None, 0, None, C.byref(b)) == -1


def test_model_reference_kat():
    """test/algorithm/surface_nets.cpp:64-75: the unit sphere on regular_grid_containing((-1,-1,-1), (1,1,1), {5,5,5}), hint
    (0, 0, 0.99): check_mesh_validity (every index a vertex, every vertex in the grid's domain); here the sphere is one
    component, so the hint mesh is the whole-grid mesh with its cubes reordered."""
    g = M.regular_grid_containing((-1, -1, -1), (1, 1, 1), (5, 5, 5))
    f = M.sphere_field(g)
    v, t, cubes, seed = H.surface_nets_hint(f, g, (0, 0, 0.99))
    assert seed is not None and len(v) > 0 and len(t) > 0
    assert t.max() < len(v)
    hi = g["x"] + F(g["sx"]) * g["dx"]
    assert np.all(v >= g["x"]) and np.all(v <= hi)
    wv, wt = M.surface_nets(f, g)
    cv, cc, ct = H.canonical(v, t, cubes)
    active = H.active_cubes(f, g)
    assert np.array_equal(cc, active)
    assert np.array_equal(cv.view(np.uint32), wv.view(np.uint32))
    assert np.array_equal(ct, active[wt.astype(np.int64)])


def test_model_keeps_one_of_two_spheres():
    g = M.regular_grid_containing((-1, -1, -1), (1, 1, 1), (24, 24, 24))
    f = np.minimum(M.sphere_field(g, 0.35, (-0.5, 0, 0)), M.sphere_field(g, 0.35, (0.5, 0, 0)))
    v, t, cubes, seed = H.surface_nets_hint(f, g, (0.5, 0, 0.3))
    x = v[:, 0]
    assert len(v) > 100 and np.all(x > 0)
    wv, _ = M.surface_nets(f, g)
    assert np.sum(wv[:, 0] > 0) == len(v)


def test_hint_header_overload_compiles(tmp_path):
    """The hint overload with the reference's signature, its defaults, and the whole-grid overload beside it."""
    src = tmp_path / "t.cpp"
    src.write_text(r'''
#include <pcp/pcp.hpp>
#include <pcp/algorithm/surface_nets.hpp>
#include <cmath>
#include <execution>
int main(int argc, char**)
{
    auto const grid = pcp::common::regular_grid_containing(pcp::point_t{-1.f, -1.f, -1.f}, pcp::point_t{1.f, 1.f, 1.f}, {5, 5, 5});
    auto const sphere = [](float x, float y, float z) { return std::sqrt(x * x + y * y + z * z) - 1.f; };
    if (argc > 5) {
        pcp::point_t const hint{0.f, 0.f, 0.99f};
        auto const [v, t] = pcp::algorithm::isosurface::surface_nets(std::execution::par, sphere, grid, hint);
        auto const [v2, t2] = pcp::algorithm::isosurface::surface_nets(std::execution::seq, sphere, grid, hint, 0.25f, 1024u);
        auto const [v3, t3] = pcp::algorithm::isosurface::surface_nets(std::execution::par, sphere, grid, 0.25f);
        return static_cast<int>(v.size() + t.size() + v2.size() + t2.size() + v3.size() + t3.size());
    }
    return 0;
}
''')
    inc = os.path.join(ROOT, "include")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", inc, str(src)], check=True)
