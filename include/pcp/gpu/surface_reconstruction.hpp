// pcp::gpu::reconstruct_surface -- examples/tangent_plane_surface_reconstruction.cpp:233-455 of the reference after the
// tree, in one device call (pcpx_reconstruct_surface): k-nearest-neighbour tangent planes of every point of the tree,
// their normals oriented (propagate_normal_orientations), the grid regular_grid_containing(box of the tree, dims), the
// signed distance to the nearest point's plane at every grid corner, surface nets at `isovalue`.  Only counts cross to the
// host until the mesh is copied out.  Not part of the reference API.
#ifndef PCP_GPU_SURFACE_RECONSTRUCTION_HPP
#define PCP_GPU_SURFACE_RECONSTRUCTION_HPP

#include "pcp/algorithm/surface_nets.hpp"
#include "pcp/common/mesh_triangle.hpp"
#include "pcp/common/points/point.hpp"
#include "pcp/gpu/device_index.hpp"
#include "pcpx.h"

#include <array>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace pcp {
namespace gpu {

// Tree: pcp::basic_linked_kdtree_t<Element, 3, ...> or pcp::basic_linked_octree_t (anything with index() returning the
// device_index_t of its points).  Vertices are world coordinates; triangles index them.
template <
    class Tree,
    class Point    = pcp::point_t,
    class Triangle = pcp::common::shared_vertex_mesh_triangle<std::uint32_t>>
std::pair<std::vector<Point>, std::vector<Triangle>>
reconstruct_surface(Tree const& tree, std::size_t k, std::array<std::size_t, 3> dims, float eps = 1e-5f, float isovalue = 0.f)
{
    pcpx_index* const h = tree.index().handle();
    if (!h) return {};
    std::uint64_t const d[3] = {dims[0], dims[1], dims[2]};
    std::uint64_t nv = 0, nt = 0;
    std::vector<float> xyz;
    std::vector<std::uint32_t> tri;
    auto const call = [&](float* v, std::uint64_t vcap, std::uint32_t* t, std::uint64_t tcap) {
        return pcpx_reconstruct_surface(h, static_cast<std::uint32_t>(k), eps, d, isovalue, v, vcap, t, tcap, &nv, &nt, nullptr, nullptr,
                                        nullptr);
    };
    int st = call(nullptr, 0, nullptr, 0);
    if (st == PCPX_ERR_CAPACITY)
    {
        xyz.resize(nv * 3);
        tri.resize(nt * 3);
        st = call(xyz.data(), nv, tri.data(), nt);
    }
    check(st, "pcpx_reconstruct_surface");
    return algorithm::isosurface::detail::to_mesh<Point, Triangle>(xyz, tri, nv, nt);
}

} // namespace gpu
} // namespace pcp

#endif
