// The flow of a keypoint example -- read a cloud, pick its keypoints, write them -- with pcp::gpu::local_maxima over a score read
// from a file and pcp::gpu::iss_keypoints (include/pcp/gpu/keypoints.hpp), through both drop-in containers: an octree of point
// views and a K = 3 kd-tree over index elements, on one cloud.  The kept element indices are written as raw uint32 to
// <out prefix>.<maxima|iss>.<tree>.u32, the saliency as raw float32 to <out prefix>.saliency.f32 and the ISS keypoints as a cloud
// to <out prefix>.ply (tests/test_gpu_keypoints.py compares them with Python's).
// usage: keypoints_shape <in.ply> <score.f32: one float32 per point> <radius> <min_neighbours> <salient radius> <non-max radius> <out prefix>
// prints one JSON object; exit status 0 when both containers agree with each other
#include <pcp/gpu/keypoints.hpp>
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
template <class T>
bool dump(std::string const& path, std::vector<T> const& v)
{
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    bool const ok = std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
    return std::fclose(f) == 0 && ok;
}
bool load(std::string const& path, std::vector<float>& v)
{
    std::FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    bool const ok = std::fread(v.data(), sizeof(float), v.size(), f) == v.size();
    return std::fclose(f) == 0 && ok;
}
// NaN positions equal and every other value equal as a float
bool same_floats(std::vector<float> const& a, std::vector<float> const& b)
{
    if (a.size() != b.size()) return false;
    for (std::size_t i = 0; i < a.size(); ++i)
        if (!(a[i] == b[i]) && !(a[i] != a[i] && b[i] != b[i])) return false;
    return true;
}
} // namespace

int main(int argc, char** argv)
{
    if (argc < 8) return 2;
    using point_type      = pcp::point_t;
    using point_view_type = pcp::point_view_t;
    using normal_type     = pcp::normal_t;
    float const radius    = std::strtof(argv[3], nullptr);
    auto const min_nb     = static_cast<std::uint32_t>(std::strtoul(argv[4], nullptr, 10));
    pcp::gpu::iss_params_t iss;
    iss.salient_radius = std::strtof(argv[5], nullptr);
    iss.non_max_radius = std::strtof(argv[6], nullptr);
    std::string const prefix{argv[7]};

    auto [input_point_cloud, input_normals] = pcp::io::read_ply<point_type, normal_type>(std::filesystem::path{argv[1]});
    (void)input_normals;
    if (input_point_cloud.empty()) return 1;
    std::size_t const n = input_point_cloud.size();
    std::vector<float> score(n);
    if (!load(argv[2], score)) return 1;

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

    auto const maxima_octree = pcp::gpu::local_maxima(octree, score, radius, -std::numeric_limits<float>::infinity(), min_nb);
    auto const maxima_kdtree = pcp::gpu::local_maxima(kdtree, score, radius, -std::numeric_limits<float>::infinity(), min_nb);
    auto const iss_octree    = pcp::gpu::iss_keypoints(octree, iss);
    auto const iss_kdtree    = pcp::gpu::iss_keypoints(kdtree, iss);

    std::vector<point_type> output_point_cloud;
    output_point_cloud.reserve(iss_octree.kept.size());
    for (std::uint32_t const i : iss_octree.kept) output_point_cloud.push_back(input_point_cloud[i]);
    pcp::io::write_ply(std::filesystem::path{prefix + ".ply"}, output_point_cloud, std::vector<normal_type>{}, pcp::io::ply_format_t::binary_little_endian);

    bool const written = dump(prefix + ".maxima.octree.u32", maxima_octree.kept) && dump(prefix + ".maxima.kdtree.u32", maxima_kdtree.kept) &&
                         dump(prefix + ".iss.octree.u32", iss_octree.kept) && dump(prefix + ".iss.kdtree.u32", iss_kdtree.kept) &&
                         dump(prefix + ".saliency.f32", iss_octree.saliency);
    bool const same = maxima_octree.kept == maxima_kdtree.kept && iss_octree.kept == iss_kdtree.kept &&
                      same_floats(iss_octree.saliency, iss_kdtree.saliency);
    std::printf("{\"points\": %zu, \"maxima\": %zu, \"iss\": %zu, \"containers_agree\": %s, \"written\": %s}\n", n, maxima_octree.kept.size(),
                iss_octree.kept.size(), same ? "true" : "false", written ? "true" : "false");
    return same && written ? 0 : 4;
}
