// The flow of a descriptor example -- read a cloud with normals, describe some of its points, write the descriptors -- with
// pcp::gpu::fpfh (include/pcp/gpu/descriptors.hpp), through both drop-in containers: an octree of point views and a K = 3 kd-tree
// over index elements, on one cloud.  The descriptors of the whole cloud are written as raw float32 (33 per point) to
// <out prefix>.all.f32 and those of the rows read from <rows.u32> to <out prefix>.rows.f32 (tests/test_gpu_fpfh.py compares them
// with Python's).
// usage: fpfh_shape <in.ply with normals> <rows.u32: raw uint32 element indices> <radius> <out prefix>
// prints one JSON object; exit status 0 when both containers agree with each other
#include <pcp/gpu/descriptors.hpp>
#include <pcp/pcp.hpp>

#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <numeric>
#include <string>
#include <vector>

namespace {
bool dump(std::string const& path, std::vector<pcp::gpu::fpfh_t> const& v)
{
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    bool const ok = v.empty() || std::fwrite(v.data(), sizeof(pcp::gpu::fpfh_t), v.size(), f) == v.size();
    return std::fclose(f) == 0 && ok;
}
bool load(std::string const& path, std::vector<std::uint32_t>& v)
{
    std::FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    std::uint32_t x;
    while (std::fread(&x, sizeof(x), 1, f) == 1) v.push_back(x);
    return std::fclose(f) == 0;
}
// bit for bit (the descriptors hold no NaN)
bool same(std::vector<pcp::gpu::fpfh_t> const& a, std::vector<pcp::gpu::fpfh_t> const& b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(pcp::gpu::fpfh_t)) == 0);
}
} // namespace

int main(int argc, char** argv)
{
    if (argc < 5) return 2;
    using point_type      = pcp::point_t;
    using point_view_type = pcp::point_view_t;
    using normal_type     = pcp::normal_t;
    float const radius    = std::strtof(argv[3], nullptr);
    std::string const prefix{argv[4]};

    auto [input_point_cloud, input_normals] = pcp::io::read_ply<point_type, normal_type>(std::filesystem::path{argv[1]});
    if (input_point_cloud.empty() || input_normals.size() != input_point_cloud.size()) return 1;
    std::size_t const n = input_point_cloud.size();
    std::vector<std::uint32_t> rows;
    if (!load(argv[2], rows)) return 1;

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

    auto const& normals_ref = input_normals;
    auto const normal_map   = [&normals_ref](std::size_t i) { return normals_ref[i]; };
    auto const all_octree  = pcp::gpu::fpfh(octree, normal_map, radius);
    auto const all_kdtree  = pcp::gpu::fpfh(kdtree, normal_map, radius);
    auto const rows_octree = pcp::gpu::fpfh(octree, normal_map, radius, &rows);
    auto const rows_kdtree = pcp::gpu::fpfh(kdtree, normal_map, radius, &rows);

    // the described rows of the subset call are those rows of the whole-cloud call
    bool subset_is_whole = rows_octree.size() == rows.size();
    for (std::size_t k = 0; subset_is_whole && k < rows.size(); ++k)
        if (rows[k] < n) subset_is_whole = std::memcmp(rows_octree[k].data(), all_octree[rows[k]].data(), sizeof(pcp::gpu::fpfh_t)) == 0;

    bool const written = dump(prefix + ".all.f32", all_octree) && dump(prefix + ".rows.f32", rows_octree);
    bool const agree   = same(all_octree, all_kdtree) && same(rows_octree, rows_kdtree);
    std::printf("{\"points\": %zu, \"rows\": %zu, \"containers_agree\": %s, \"subset_is_whole\": %s, \"written\": %s}\n", n, rows.size(),
                agree ? "true" : "false", subset_is_whole ? "true" : "false", written ? "true" : "false");
    return agree && subset_is_whole && written ? 0 : 4;
}
