// Drop-in check for the reference's surface-reconstruction caller, examples/tangent_plane_surface_reconstruction.cpp:233-455.
// Not that program (it needs libigl and a window): the same pcp call SEQUENCE with the same argument types --
//   io::read_ply<point_t, normal_t>; a basic_linked_kdtree_t<size_t, 3, CoordinateMap> with construction_params_t
//   {compute_max_depth}; algorithm::estimate_tangent_planes(par, ...) with kdtree.nearest_neighbours(v, k) as the KnnMap and
//   default_plane_transform; propagate_normal_orientations(index map, knn map, point map, normal map, transform); the
//   signed-distance lambda (1-NN of the corner, inner_product(p - o, n)); regular_grid_containing over kdtree.aabb();
//   isosurface::surface_nets(std::execution::par, sdf, grid) --
// and, for comparison, the same mesh from the one-call device path (pcp::gpu::reconstruct_surface).
// usage: surface_reconstruction_shape <in.ply> <dim> <out_sequence.ply> <out_one_call.ply>
#include <pcp/pcp.hpp>
#include <pcp/gpu/surface_reconstruction.hpp>

#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <execution>
#include <filesystem>
#include <numeric>
#include <vector>

int main(int argc, char** argv)
{
    if (argc < 5) return 2;
    using point_type  = pcp::point_t;
    using plane_type  = pcp::common::plane3d_t;
    using vertex_type = std::size_t;
    std::size_t const k   = 10;  // the example's default
    std::size_t const dim = std::strtoull(argv[2], nullptr, 10);

    auto [points, unused] = pcp::io::read_ply<pcp::point_t, pcp::normal_t>(std::filesystem::path{argv[1]});
    (void)unused;
    if (points.empty()) return 1;

    std::vector<vertex_type> vertices(points.size());
    std::iota(vertices.begin(), vertices.end(), 0u);
    auto const point_map      = [&](vertex_type const& v) { return points[v]; };
    auto const coordinate_map = [&](vertex_type const& v) { return std::array<float, 3u>{points[v].x(), points[v].y(), points[v].z()}; };

    pcp::kdtree::construction_params_t params;
    params.compute_max_depth = true;
    pcp::basic_linked_kdtree_t<vertex_type, 3u, decltype(coordinate_map)> kdtree{vertices.begin(), vertices.end(), coordinate_map, params};

    auto const knn_map = [&](vertex_type const& v) { return kdtree.nearest_neighbours(v, k); };
    std::vector<plane_type> tangent_planes(points.size());
    pcp::algorithm::estimate_tangent_planes(std::execution::par, vertices.cbegin(), vertices.cend(), tangent_planes.begin(), point_map,
                                            knn_map, pcp::algorithm::default_plane_transform<vertex_type, plane_type>);

    auto const normal_map   = [&](vertex_type const& v) { return tangent_planes[v].normal(); };
    auto const transform_op = [&](vertex_type const& v, pcp::normal_t const& n) { tangent_planes[v].normal(n); };
    auto const index_map    = [](vertex_type const& v) { return v; };
    pcp::algorithm::propagate_normal_orientations(vertices.begin(), vertices.end(), index_map, knn_map, point_map, normal_map, transform_op);

    auto const signed_distance_function = [&](float x, float y, float z) {
        point_type const p{x, y, z};
        auto const nearest_neighbours = kdtree.nearest_neighbours({p.x(), p.y(), p.z()}, 1u);
        auto const& tangent_plane     = tangent_planes[nearest_neighbours.front()];
        auto const o                  = tangent_plane.point();
        auto const n                  = tangent_plane.normal();
        auto const op                 = p - o;
        return pcp::common::inner_product(op, n);
    };
    auto const& aabb = kdtree.aabb();
    auto const grid  = pcp::common::regular_grid_containing(pcp::point_t{aabb.min[0], aabb.min[1], aabb.min[2]},
                                                           pcp::point_t{aabb.max[0], aabb.max[1], aabb.max[2]}, {dim, dim, dim});
    auto const [mesh_vertices, mesh_triangles] = pcp::algorithm::isosurface::surface_nets(std::execution::par, signed_distance_function, grid);
    pcp::io::write_ply(std::filesystem::path{argv[3]}, mesh_vertices, mesh_triangles, pcp::io::ply_format_t::binary_little_endian);

    auto const [v1, t1] = pcp::gpu::reconstruct_surface(kdtree, k, {dim, dim, dim});
    pcp::io::write_ply(std::filesystem::path{argv[4]}, v1, t1, pcp::io::ply_format_t::binary_little_endian);
    std::printf("{\"points\": %zu, \"vertices\": %zu, \"triangles\": %zu, \"one_call_vertices\": %zu, \"one_call_triangles\": %zu}\n",
                points.size(), mesh_vertices.size(), mesh_triangles.size(), v1.size(), t1.size());
    return 0;
}
