// pcp::algorithm::isosurface::surface_nets -- drop-in for the reference's naive surface nets over a whole grid
// (include/pcp/algorithm/surface_nets.hpp:357-650 of the reference), meshed on the GPU (pcpx_surface_nets, include/pcpx.h).
//
// The user's f is evaluated on the host, ONCE PER GRID CORNER -- (sx+1)(sy+1)(sz+1) calls, spread over `policy` with
// std::for_each -- instead of 8 per cube plus 4 per active cube (about 8*sx*sy*sz calls) as in the reference; only an impure
// f can tell the difference.  The field is uploaded and the mesh is built on the device with the reference's arithmetic.
// Differences in what comes back ("Surface reconstruction"):
//   * the order is deterministic: vertices by ascending cube index i + j*sx + k*sx*sy, triangles by (cube, quad 0..2,
//     triangle 0..1) -- the reference's order is the push order under a mutex;
//   * every grid cube is meshed once -- the reference's loop corrupts its counters when sx or sy is strictly the longest
//     dimension and then meshes cubes outside the grid.  Where neither is (cubes, z longest, ties) the cube sets agree.
//
// The overload with a hint point (:653-1119 of the reference) meshes only the connected component of the isosurface that the
// search from the hint reaches first (pcpx_surface_nets_hint).  f is evaluated as above, once per
// corner.  Differences: the grid is the world -- cubes outside it are never active, where the reference walks linear
// indices across faces and evaluates f outside the grid; the seed is the first active cube in the reference's search order,
// or, when that search has no bound (breadth_first_search_queue_max_size 0, or a size its queue steps over), the active
// cube nearest the hint cube in Manhattan distance beyond 2^20 simulated pops; the output is the whole-grid mesh restricted
// to the component, vertices in ascending cube index (the reference's order is its search order).  A hint that finds no
// active cube before the queue holds exactly breadth_first_search_queue_max_size cubes gives the whole-grid mesh, as in the
// reference.
#ifndef PCP_ALGORITHM_SURFACE_NETS_HPP
#define PCP_ALGORITHM_SURFACE_NETS_HPP

#include "pcp/common/mesh_triangle.hpp"
#include "pcp/common/points/point.hpp"
#include "pcp/common/regular_grid3d.hpp"
#include "pcp/gpu/device_index.hpp"
#include "pcp/traits/function_traits.hpp"
#include "pcp/traits/point_traits.hpp"
#include "pcp/traits/triangle_traits.hpp"
#include "pcpx.h"

#include <algorithm>
#include <cstdint>
#include <execution>
#include <numeric>
#include <type_traits>
#include <utility>
#include <vector>

namespace pcp {
namespace algorithm {
namespace isosurface {

namespace detail {

inline pcpx_grid3d to_pcpx_grid(common::regular_grid3d_t<float> const& g)
{
    return pcpx_grid3d{g.x, g.y, g.z, g.dx, g.dy, g.dz, g.sx, g.sy, g.sz};
}

// the mesh of a device call as the caller's vertex and triangle types
template <class Point, class Triangle>
std::pair<std::vector<Point>, std::vector<Triangle>>
to_mesh(std::vector<float> const& xyz, std::vector<std::uint32_t> const& tri, std::uint64_t nv, std::uint64_t nt)
{
    using index_type = typename Triangle::index_type;
    using coord_type = typename Point::coordinate_type;
    std::vector<Point> vertices;
    std::vector<Triangle> triangles;
    vertices.reserve(nv);
    triangles.reserve(nt);
    for (std::uint64_t v = 0; v < nv; ++v)
        vertices.push_back(Point{static_cast<coord_type>(xyz[3 * v]), static_cast<coord_type>(xyz[3 * v + 1]),
                                 static_cast<coord_type>(xyz[3 * v + 2])});
    for (std::uint64_t t = 0; t < nt; ++t)
        triangles.push_back(Triangle{static_cast<index_type>(tri[3 * t]), static_cast<index_type>(tri[3 * t + 1]),
                                     static_cast<index_type>(tri[3 * t + 2])});
    return {std::move(vertices), std::move(triangles)};
}

// pcpx_surface_nets on a host field, sized by a first call that reports the totals
inline void surface_nets_host(std::vector<float> const& field, pcpx_grid3d const& g, float isovalue, std::vector<float>& xyz,
                              std::vector<std::uint32_t>& tri, std::uint64_t& nv, std::uint64_t& nt)
{
    int const device = gpu::default_device().load();
    int st = pcpx_surface_nets(field.data(), &g, isovalue, device, nullptr, 0, nullptr, 0, &nv, &nt);
    if (st == PCPX_ERR_CAPACITY)
    {
        xyz.resize(nv * 3);
        tri.resize(nt * 3);
        st = pcpx_surface_nets(field.data(), &g, isovalue, device, xyz.data(), nv, tri.data(), nt, &nv, &nt);
    }
    gpu::check(st, "pcpx_surface_nets");
}

// f at every corner (i, j, k), at get_world_point_of(i, j, k): one task per z-slab of corners
template <class ExecutionPolicy, class Func>
std::vector<float> corner_field(ExecutionPolicy&& policy, Func&& f, common::regular_grid3d_t<float> const& grid)
{
    std::size_t const nx = grid.sx + 1, ny = grid.sy + 1, nz = grid.sz + 1;
    std::vector<float> field(nx * ny * nz);
    std::vector<std::size_t> slabs(nz);
    std::iota(slabs.begin(), slabs.end(), std::size_t{0});
    std::for_each(policy, slabs.cbegin(), slabs.cend(), [&](std::size_t k) {
        float const z = grid.z + static_cast<float>(k) * grid.dz;
        for (std::size_t j = 0; j < ny; ++j)
        {
            float const y = grid.y + static_cast<float>(j) * grid.dy;
            float* row    = field.data() + (k * ny + j) * nx;
            for (std::size_t i = 0; i < nx; ++i)
                row[i] = static_cast<float>(f(grid.x + static_cast<float>(i) * grid.dx, y, z));
        }
    });
    return field;
}

// pcpx_surface_nets_hint on a host field, sized by a first call that reports the totals
inline void surface_nets_hint_host(std::vector<float> const& field, pcpx_grid3d const& g, float isovalue, float const hint[3],
                                   std::uint64_t queue_max, std::vector<float>& xyz, std::vector<std::uint32_t>& tri, std::uint64_t& nv,
                                   std::uint64_t& nt)
{
    int const device = gpu::default_device().load();
    int st = pcpx_surface_nets_hint(field.data(), &g, isovalue, hint, queue_max, device, nullptr, 0, nullptr, 0, &nv, &nt, nullptr);
    if (st == PCPX_ERR_CAPACITY)
    {
        xyz.resize(nv * 3);
        tri.resize(nt * 3);
        st = pcpx_surface_nets_hint(field.data(), &g, isovalue, hint, queue_max, device, xyz.data(), nv, tri.data(), nt, &nv, &nt, nullptr);
    }
    gpu::check(st, "pcpx_surface_nets_hint");
}

} // namespace detail

template <
    class ExecutionPolicy,
    class Func,
    class Scalar,
    class Point                    = pcp::point_t,
    class SharedVertexMeshTriangle = pcp::common::shared_vertex_mesh_triangle<std::uint32_t>>
auto surface_nets(
    ExecutionPolicy&& policy,
    Func&& f,
    common::regular_grid3d_t<Scalar> const& grid,
    Scalar const isovalue = static_cast<Scalar>(0)) -> std::pair<std::vector<Point>, std::vector<SharedVertexMeshTriangle>>
{
    static_assert(
        traits::is_3d_scalar_function_v<Func, Scalar>,
        "Func must be 3d scalar function Scalar Func(Scalar, Scalar, Scalar)");
    static_assert(traits::is_point_v<Point>, "Point must satisfy Point concept");
    static_assert(
        traits::is_shared_vertex_mesh_triangle_v<SharedVertexMeshTriangle>,
        "Triangle must satisfy SharedVertexMeshTriangle concept");
    static_assert(std::is_same_v<Scalar, float>, "the device meshes float grids (pcpx_grid3d)");

    if (grid.sx == 0 || grid.sy == 0 || grid.sz == 0) return {};
    std::vector<float> const field = detail::corner_field(policy, f, grid);
    std::vector<float> xyz;
    std::vector<std::uint32_t> tri;
    std::uint64_t nv = 0, nt = 0;
    detail::surface_nets_host(field, detail::to_pcpx_grid(grid), isovalue, xyz, tri, nv, nt);
    return detail::to_mesh<Point, SharedVertexMeshTriangle>(xyz, tri, nv, nt);
}

template <
    class ExecutionPolicy,
    class Func,
    class Scalar,
    class Point                    = pcp::point_t,
    class SharedVertexMeshTriangle = pcp::common::shared_vertex_mesh_triangle<std::uint32_t>>
auto surface_nets(
    ExecutionPolicy&& policy,
    Func&& f,
    common::regular_grid3d_t<Scalar> const& grid,
    Point const& hint,
    Scalar const isovalue                           = static_cast<Scalar>(0),
    std::size_t breadth_first_search_queue_max_size = 32768u)
    -> std::pair<std::vector<Point>, std::vector<SharedVertexMeshTriangle>>
{
    static_assert(
        traits::is_3d_scalar_function_v<Func, Scalar>,
        "Func must be 3d scalar function Scalar Func(Scalar, Scalar, Scalar)");
    static_assert(traits::is_point_v<Point>, "Point must satisfy Point concept");
    static_assert(
        traits::is_shared_vertex_mesh_triangle_v<SharedVertexMeshTriangle>,
        "Triangle must satisfy SharedVertexMeshTriangle concept");
    static_assert(std::is_same_v<Scalar, float>, "the device meshes float grids (pcpx_grid3d)");

    float const h[3] = {static_cast<float>(hint.x()), static_cast<float>(hint.y()), static_cast<float>(hint.z())};
    if (grid.sx == 0 || grid.sy == 0 || grid.sz == 0) return {};
    std::vector<float> const field = detail::corner_field(policy, f, grid);
    std::vector<float> xyz;
    std::vector<std::uint32_t> tri;
    std::uint64_t nv = 0, nt = 0;
    detail::surface_nets_hint_host(field, detail::to_pcpx_grid(grid), isovalue, h, breadth_first_search_queue_max_size, xyz, tri, nv, nt);
    return detail::to_mesh<Point, SharedVertexMeshTriangle>(xyz, tri, nv, nt);
}

} // namespace isosurface
} // namespace algorithm
} // namespace pcp

#endif
