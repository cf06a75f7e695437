// The flow of a downsampling example -- read a cloud, thin it, write the thinned cloud -- with pcp::gpu::poisson_disk_subsample
// (include/pcp/gpu/subsampling.hpp) as the downsampler, through both drop-in containers: an octree of point views and a K = 3
// kd-tree over index elements, on one cloud.  The kept element indices of each container are written as raw uint32 to
// <out prefix>.<tree>.u32 and the thinned cloud to <out prefix>.ply (tests/test_gpu_subsample.py compares them with Python's).
// usage: subsample_shape <in.ply> <radius> <seed> <out prefix>
// prints one JSON object; exit status 0 when both containers agree with each other and the owners are consistent
#include <pcp/gpu/subsampling.hpp>
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
    float const radius    = std::strtof(argv[2], nullptr);
    auto const seed       = static_cast<std::uint32_t>(std::strtoul(argv[3], nullptr, 10));
    std::string const prefix{argv[4]};

    auto [input_point_cloud, input_normals] = pcp::io::read_ply<point_type, normal_type>(std::filesystem::path{argv[1]});
    (void)input_normals;
    if (input_point_cloud.empty()) return 1;
    std::size_t const n = input_point_cloud.size();

    std::vector<point_view_type> views;
    views.reserve(n);
    for (auto& p : input_point_cloud) views.push_back(point_view_type{&p});
    auto const view_map = [](point_view_type const& p) { return p; };
    pcp::basic_linked_octree_t<point_view_type> octree{views.begin(), views.end(), view_map};
    if (octree.size() != n) return 3;

    std::vector<std::size_t> ids(n);
    std::iota(ids.begin(), ids.end(), std::size_t{0});
    auto const coords_of = [&](std::size_t const& i) {
        return std::array<float, 3u>{input_point_cloud[i].x(), input_point_cloud[i].y(), input_point_cloud[i].z()};
    };
    pcp::kdtree::construction_params_t params;
    params.compute_max_depth = true;
    pcp::basic_linked_kdtree_t<std::size_t, 3u, decltype(coords_of)> kdtree{ids.begin(), ids.end(), coords_of, params};

    auto const from_octree = pcp::gpu::poisson_disk_subsample(octree, radius, seed);
    auto const from_kdtree = pcp::gpu::poisson_disk_subsample(kdtree, radius, seed);
    auto const other_seed  = pcp::gpu::poisson_disk_subsample(octree, radius, seed + 1u);

    std::vector<point_type> output_point_cloud;
    output_point_cloud.reserve(from_octree.kept.size());
    for (std::uint32_t const i : from_octree.kept) output_point_cloud.push_back(input_point_cloud[i]);
    pcp::io::write_ply(std::filesystem::path{prefix + ".ply"}, output_point_cloud, std::vector<normal_type>{}, pcp::io::ply_format_t::binary_little_endian);

    // every element's owner is a kept element; a kept element owns itself
    std::vector<std::uint8_t> is_kept(n, std::uint8_t{0});
    for (std::uint32_t const i : from_octree.kept) is_kept[i] = 1;
    bool owners_ok = from_octree.owner.size() == n;
    for (std::size_t i = 0; owners_ok && i < n; ++i)
    {
        std::uint32_t const o = from_octree.owner[i];
        owners_ok = o < n && is_kept[o] && (!is_kept[i] || o == i);
    }

    bool const written = dump(prefix + ".octree.u32", from_octree.kept) && dump(prefix + ".kdtree.u32", from_kdtree.kept) &&
                         dump(prefix + ".octree.owner.u32", from_octree.owner) && dump(prefix + ".octree.other_seed.u32", other_seed.kept);
    bool const same = from_octree.kept == from_kdtree.kept && from_octree.owner == from_kdtree.owner;
    std::printf("{\"points\": %zu, \"radius\": %.9g, \"seed\": %u, \"kept\": %zu, \"kept_other_seed\": %zu, \"rounds\": %u, "
                "\"containers_agree\": %s, \"owners_consistent\": %s, \"written\": %s}\n",
                n, double(radius), seed, from_octree.kept.size(), other_seed.kept.size(), from_octree.rounds, same ? "true" : "false",
                owners_ok ? "true" : "false", written ? "true" : "false");
    return same && owners_ok && written ? 0 : 4;
}
