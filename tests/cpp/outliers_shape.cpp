// The flow of the reference's examples/filter_point_cloud_noise_by_density.cpp -- read a cloud, build a tree over point views, drop
// the points whose ball holds too few points, write the rest -- with the example's ball radius and its remove_if as ONE call:
// pcp::gpu::density_outlier_removal (include/pcp/gpu/outliers.hpp).  tests/cpp/density_filter_shape.cpp is the same flow through the
// reference's own call shapes; tests/test_gpu_outliers.py runs both on one cloud.
// usage: outliers_shape <in.ply> <out.ply> [min points per ball = 5] [radius multiplier = 1] [k = 15]
// prints one JSON object: cloud size before and after, the ball radius, the resolution
#include <pcp/gpu/outliers.hpp>
#include <pcp/pcp.hpp>

#include <cstdio>
#include <cstdlib>
#include <filesystem>
#include <vector>

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    auto const at_least    = static_cast<std::uint32_t>(argc > 3 ? std::strtoul(argv[3], nullptr, 10) : 5u);
    float const multiplier = argc > 4 ? std::strtof(argv[4], nullptr) : 1.f;
    auto const k           = static_cast<std::uint32_t>(argc > 5 ? std::strtoul(argv[5], nullptr, 10) : 15u);

    auto [cloud, normals] = pcp::io::read_ply<pcp::point_t, pcp::normal_t>(std::filesystem::path{argv[1]});
    (void)normals;
    if (cloud.empty()) return 1;
    std::size_t const before = cloud.size();

    std::vector<pcp::point_view_t> views;
    views.reserve(before);
    for (auto& p : cloud) views.push_back(pcp::point_view_t{&p});
    auto const identity = [](pcp::point_view_t const& v) { return v; };
    pcp::basic_linked_octree_t<pcp::point_view_t> tree{views.begin(), views.end(), identity};
    if (tree.size() != before) return 3;

    auto const filtered = pcp::gpu::density_outlier_removal(tree, k, multiplier, at_least);

    std::vector<pcp::point_t> kept;
    kept.reserve(filtered.kept.size());
    for (std::uint32_t const i : filtered.kept) kept.push_back(cloud[i]);
    pcp::io::write_ply(std::filesystem::path{argv[2]}, kept, std::vector<pcp::normal_t>{}, pcp::io::ply_format_t::binary_little_endian);

    std::printf("{\"points_before\": %zu, \"points_after\": %zu, \"radius\": %.9g, \"mean\": %.17g, \"std\": %.17g, \"usable\": %llu}\n", before,
                kept.size(), static_cast<double>(filtered.cut), filtered.resolution.mean, filtered.resolution.std,
                static_cast<unsigned long long>(filtered.resolution.usable));
    return 0;
}
