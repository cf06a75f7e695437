// pcp::gpu::euclidean_clusters and pcp::gpu::dbscan (include/pcp/gpu/clustering.hpp) through both drop-in containers: an octree of
// point views and a K = 3 kd-tree over index elements, on one cloud.  The labels of each call are written as raw uint32 to
// <out prefix>.<tree>.<call>.u32 for the caller to compare (tests/test_gpu_cluster.py compares them with Python's).
// usage: cluster_shape <in.ply> <radius> <min_pts> <out prefix>
// prints one JSON object; exit status 0 when both containers agree with each other
#include <pcp/gpu/clustering.hpp>
#include <pcp/pcp.hpp>

#include <array>
#include <cstdio>
#include <cstdlib>
#include <filesystem>
#include <numeric>
#include <string>
#include <vector>

namespace {
bool dump(std::string const& path, std::vector<std::uint32_t> const& v)
{
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    bool const ok = std::fwrite(v.data(), sizeof(std::uint32_t), v.size(), f) == v.size();
    return std::fclose(f) == 0 && ok;
}
} // namespace

int main(int argc, char** argv)
{
    if (argc < 5) return 2;
    using point_type      = pcp::point_t;
    using point_view_type = pcp::point_view_t;
    using normal_type     = pcp::normal_t;
    float const r         = std::strtof(argv[2], nullptr);
    auto const min_pts    = static_cast<std::uint32_t>(std::strtoul(argv[3], nullptr, 10));
    std::string const prefix{argv[4]};

    auto [points, unused] = pcp::io::read_ply<point_type, normal_type>(std::filesystem::path{argv[1]});
    (void)unused;
    if (points.empty()) return 1;
    std::size_t const n = points.size();
    std::vector<point_view_type> views;
    views.reserve(n);
    for (auto& p : points) views.push_back(point_view_type{&p});
    auto const view_map = [](point_view_type const& p) { return p; };
    pcp::basic_linked_octree_t<point_view_type> octree{views.begin(), views.end(), view_map};
    if (octree.size() != n) return 3;

    std::vector<std::size_t> ids(n);
    std::iota(ids.begin(), ids.end(), std::size_t{0});
    auto const coords_of = [&](std::size_t const& i) { return std::array<float, 3u>{points[i].x(), points[i].y(), points[i].z()}; };
    pcp::kdtree::construction_params_t params;
    params.compute_max_depth = true;
    pcp::basic_linked_kdtree_t<std::size_t, 3u, decltype(coords_of)> kdtree{ids.begin(), ids.end(), coords_of, params};

    auto const oe = pcp::gpu::euclidean_clusters(octree, r);
    auto const od = pcp::gpu::dbscan(octree, r, min_pts);
    auto const ke = pcp::gpu::euclidean_clusters(kdtree, r);
    auto const kd = pcp::gpu::dbscan(kdtree, r, min_pts);
    auto const kr = pcp::gpu::dbscan(kdtree, r, min_pts, false);

    bool ok = dump(prefix + ".octree.euclidean.u32", oe.labels) && dump(prefix + ".octree.dbscan.u32", od.labels) &&
              dump(prefix + ".kdtree.euclidean.u32", ke.labels) && dump(prefix + ".kdtree.dbscan.u32", kd.labels) &&
              dump(prefix + ".kdtree.dbscan_representatives.u32", kr.labels);
    bool const same = oe.labels == ke.labels && od.labels == kd.labels && od.core == kd.core && oe.cluster_count == ke.cluster_count &&
                      od.cluster_count == kd.cluster_count && kr.cluster_count == kd.cluster_count;
    std::size_t core = 0, noise = 0;
    for (std::size_t i = 0; i < n; ++i) core += od.core[i], noise += od.labels[i] == pcp::gpu::clusters_t::noise ? 1u : 0u;
    std::printf("{\"points\": %zu, \"radius\": %.9g, \"min_pts\": %u, \"euclidean_clusters\": %llu, \"dbscan_clusters\": %llu, "
                "\"core\": %zu, \"noise\": %zu, \"containers_agree\": %s, \"written\": %s}\n",
                n, double(r), min_pts, static_cast<unsigned long long>(oe.cluster_count), static_cast<unsigned long long>(od.cluster_count),
                core, noise, same ? "true" : "false", ok ? "true" : "false");
    return same && ok ? 0 : 4;
}
