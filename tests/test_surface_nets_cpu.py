"""Surface nets without a GPU: the numpy restatement of the reference (tests/surface_nets_model.py) on the reference test's
own conditions and on small cases worked by hand, and the C++ drop-in headers of the surface-reconstruction path compiled."""
import os
import subprocess

import numpy as np

import surface_nets_model as M
from conftest import ROOT

F = np.float32


def test_model_unit_sphere_on_5_cubed_grid():
    """test/algorithm/surface_nets.cpp: the unit sphere on regular_grid_containing((-1,-1,-1), (1,1,1), {5,5,5}); every
    triangle index is a vertex, every vertex lies in the grid's domain."""
    g = M.regular_grid_containing((-1, -1, -1), (1, 1, 1), (5, 5, 5))
    v, t = M.surface_nets(M.sphere_field(g), g)
    assert len(v) > 0 and len(t) > 0
    assert t.max() < len(v)
    hi = g["x"] + F(g["sx"]) * g["dx"]
    assert np.all(v >= g["x"]) and np.all(v <= hi)
    # the sphere is closed inside the grid: every vertex sits near radius 1
    r = np.linalg.norm(v.astype(np.float64), axis=1)
    assert np.all(np.abs(r - 1.0) < 0.5)


def _unit_grid(n):
    return M.grid_dict(0, 0, 0, 1, 1, 1, n, n, n)


def test_model_one_negative_corner():
    """2 x 2 x 2 cubes, field +1 except -1 at corner (1, 1, 0): the four cubes around it (k = 0) are active, each vertex is the
    centroid of the midpoints of the three cube edges at the negative corner, and no cube with i, j, k >= 1 is active."""
    g = _unit_grid(2)
    f = np.ones((3, 3, 3), F)
    f[0, 1, 1] = -1  # [k, j, i]
    v, t = M.surface_nets(f, g)
    assert len(t) == 0
    assert len(v) == 4
    # cubes (0,0,0), (1,0,0), (0,1,0), (1,1,0) in that order; the negative corner n = (1,1,0), its cube-edge neighbours
    expect = []
    for (ci, cj) in [(0, 0), (1, 0), (0, 1), (1, 1)]:
        n = np.array([1, 1, 0], F)
        others = []
        for ax in range(3):
            o = n.copy()
            lo = (ci, cj, 0)[ax]
            o[ax] = lo if n[ax] == lo + 1 else lo + 1
            others.append(o)
        mids = [n + F(0.5) * (o - n) for o in others]
        expect.append((mids[0] + mids[1] + mids[2]) / F(3))
    np.testing.assert_allclose(v, np.array(expect, F), rtol=0, atol=1e-6)


def test_model_negative_centre_corner():
    """3 x 3 x 3 corners, -1 at the centre: the 8 cubes around it are active; only cube (1,1,1) has i, j, k >= 1, its three
    neighbour triples are all active, so it emits 3 quads = 6 triangles.  The directed edges (0,4) and (0,1) rise from the
    centre (order [0,1,2]), the directed edge (3,0) falls into it (order [2,1,0])."""
    g = _unit_grid(2)
    f = np.ones((3, 3, 3), F)
    f[1, 1, 1] = -1
    v, t = M.surface_nets(f, g)
    assert len(v) == 8
    # vertex of cube (i,j,k): the centroid of the 3 edge midpoints at the centre corner
    for c in range(8):
        i, j, k = c % 2, (c // 2) % 2, c // 4
        far = np.array([i, j, k], F) * F(2) - F(1) + F(1)  # the cube's corner opposite the centre, per axis 0 or 2
        expect = F(1) + (far - F(1)) * F(0.5) / F(3)
        np.testing.assert_allclose(v[c], expect, atol=1e-6)
    # neighbours of cube 7 = (1,1,1): n0=(0,1,1)=6, n1=(0,0,1)=4, n2=(1,0,1)=5, n3=(1,0,0)=1, n4=(1,1,0)=3, n5=(0,1,0)=2
    assert t.tolist() == [[7, 6, 4], [7, 4, 5], [7, 3, 2], [7, 2, 6], [7, 5, 1], [7, 1, 3]]


def test_model_winding_flips_with_the_edge():
    """The same with the signs swapped: every quad reverses."""
    g = _unit_grid(2)
    f = -np.ones((3, 3, 3), F)
    f[1, 1, 1] = 1
    _, t = M.surface_nets(f, g)
    assert t.tolist() == [[7, 5, 4], [7, 4, 6], [7, 6, 2], [7, 2, 3], [7, 3, 1], [7, 1, 5]]


def test_model_grid_containing_quirk():
    g = M.regular_grid_containing((0, 10, 20), (2, 14, 26), (2, 2, 2))
    assert (g["dx"], g["dy"], g["dz"]) == (1, 2, 3)
    assert (g["x"], g["y"], g["z"]) == (-1, 9, 19)  # every axis moves back by dx
    assert (g["sx"], g["sy"], g["sz"]) == (4, 4, 4)


def test_mesh_ply_round_trip(tmp_path, pkg):
    g = M.regular_grid_containing((-1, -1, -1), (1, 1, 1), (6, 6, 6))
    v, t = M.surface_nets(M.sphere_field(g), g)
    for fmt in ("binary_little_endian", "binary_big_endian", "ascii"):
        p = str(tmp_path / ("m_%s.ply" % fmt))
        pkg.ply.write_mesh_ply(p, v, t, fmt)
        rv, rt = pkg.ply.read_mesh_ply(p)
        assert np.array_equal(rv, v) and np.array_equal(rt, t)


def test_surface_headers_compile(tmp_path):
    """regular_grid3d / mesh_triangle / surface_nets (with a lambda) / the mesh write_ply / the GPU convenience."""
    src = tmp_path / "t.cpp"
    src.write_text(r'''
#include <pcp/pcp.hpp>
#include <pcp/algorithm/surface_nets.hpp>
#include <pcp/common/mesh_triangle.hpp>
#include <pcp/common/regular_grid3d.hpp>
#include <pcp/gpu/surface_reconstruction.hpp>
#include <pcp/io/ply.hpp>
#include <cmath>
#include <execution>
int main(int argc, char**)
{
    auto const grid = pcp::common::regular_grid_containing(pcp::point_t{-1.f, -1.f, -1.f}, pcp::point_t{1.f, 1.f, 1.f}, {5, 5, 5});
    auto const sphere = [](float x, float y, float z) { return std::sqrt(x * x + y * y + z * z) - 1.f; };
    if (argc > 5) {
        auto const [v, t] = pcp::algorithm::isosurface::surface_nets(std::execution::par, sphere, grid);
        pcp::io::write_ply("m.ply", v, t, pcp::io::ply_format_t::binary_little_endian);
    }
    static_assert(pcp::traits::is_shared_vertex_mesh_triangle_v<pcp::common::shared_vertex_mesh_triangle<std::uint32_t>>);
    static_assert(pcp::traits::is_3d_scalar_function_v<decltype(sphere), float>);
    return 0;
}
''')
    inc = os.path.join(ROOT, "include")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", inc, str(src)], check=True)
