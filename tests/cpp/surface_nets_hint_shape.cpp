// Drop-in check for the `graph` meshing variant of examples/tangent_plane_surface_reconstruction.cpp:393-445 (the caller of
// the surface-nets overload with a hint point).  Not that program (it needs libigl and a window): the same pcp call SEQUENCE
// with the same argument types -- io::read_ply; a basic_linked_kdtree_t with construction_params_t{compute_max_depth};
// estimate_tangent_planes(par, ...) and propagate_normal_orientations over kdtree.nearest_neighbours(v, k); the
// signed-distance lambda; regular_grid_containing over kdtree.aabb(); the densest point (smallest mean distance to its k
// nearest neighbours, std::min_element) and the centroid of its k nearest neighbours as the hint;
// isosurface::surface_nets(std::execution::par, sdf, grid, hint).
// The example's min_element compares mean distances recomputed by two kNN queries per comparison; here the means come from
// average_distances_to_neighbors over the same kNN rows, and min_element runs over them -- the same point.
// usage: surface_nets_hint_shape <in.ply> <dim> <out.ply>   (prints the hint and the mesh sizes as JSON)
#include <pcp/pcp.hpp>

#include <algorithm>
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
    if (argc < 4) return 2;
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

    // the hint: the densest point's k nearest neighbours, averaged
    std::vector<float> const mean_distances =
        pcp::algorithm::average_distances_to_neighbors(vertices.begin(), vertices.end(), point_map, pcp::gpu::self_knn_map(kdtree, k));
    auto const densest = static_cast<std::size_t>(std::min_element(mean_distances.cbegin(), mean_distances.cend()) - mean_distances.cbegin());
    auto const kneighbours = kdtree.nearest_neighbours({points[densest].x(), points[densest].y(), points[densest].z()}, k);
    auto const hint        = std::accumulate(kneighbours.cbegin(), kneighbours.cend(), pcp::point_t{0.f, 0.f, 0.f},
                                             [&](pcp::point_t const& val, vertex_type const& v) {
                                          auto p = point_map(v);
                                          return val + p;
                                      }) /
                      static_cast<float>(kneighbours.size());

    auto const [mesh_vertices, mesh_triangles] = pcp::algorithm::isosurface::surface_nets(std::execution::par, signed_distance_function, grid, hint);
    pcp::io::write_ply(std::filesystem::path{argv[3]}, mesh_vertices, mesh_triangles, pcp::io::ply_format_t::binary_little_endian);
    std::printf("{\"points\": %zu, \"densest\": %zu, \"hint\": [%.9g, %.9g, %.9g], \"vertices\": %zu, \"triangles\": %zu}\n", points.size(),
                densest, static_cast<double>(hint.x()), static_cast<double>(hint.y()), static_cast<double>(hint.z()), mesh_vertices.size(),
                mesh_triangles.size());
    return 0;
}
