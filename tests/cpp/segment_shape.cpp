// pcp::gpu::smooth_segments (include/pcp/gpu/segmentation.hpp) through both drop-in containers -- an octree of point views and a
// K = 3 kd-tree over index elements -- and through its device-normals form, on one cloud with the normals of a raw float32 file
// (n x 3, element order).  The labels of each call are written as raw uint32 to <out prefix>.<call>.u32 for the caller to compare
// (tests/test_gpu_segment.py compares them with Python's).
// usage: segment_shape <in.ply> <normals.f32> <radius> <max_angle> <min_size> <out prefix>
// prints one JSON object; exit status 0 when the three routes agree with each other
#include <pcp/gpu/segmentation.hpp>
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
struct raw_normal_t  // (pcp::normal_t normalises what it is given; the segmentation takes normals as they are)
{
    float a, b, c;
    float x() const { return a; }
    float y() const { return b; }
    float z() const { return c; }
};
} // namespace

int main(int argc, char** argv)
{
    if (argc < 7) return 2;
    using point_type      = pcp::point_t;
    using point_view_type = pcp::point_view_t;
    using normal_type     = pcp::normal_t;
    float const r         = std::strtof(argv[3], nullptr);
    float const max_angle = std::strtof(argv[4], nullptr);
    auto const min_size   = static_cast<std::uint32_t>(std::strtoul(argv[5], nullptr, 10));
    std::string const prefix{argv[6]};

    auto [points, unused] = pcp::io::read_ply<point_type, normal_type>(std::filesystem::path{argv[1]});
    (void)unused;
    if (points.empty()) return 1;
    std::size_t const n = points.size();
    std::vector<float> normals(3 * n);
    {
        std::FILE* f = std::fopen(argv[2], "rb");
        if (!f) return 1;
        bool const ok = std::fread(normals.data(), sizeof(float), normals.size(), f) == normals.size();
        std::fclose(f);
        if (!ok) return 1;
    }
    auto const normal_map = [&](std::size_t i) { return raw_normal_t{normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]}; };

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

    pcp::gpu::segment_params_t filtered;
    filtered.min_size = min_size;
    pcp::gpu::segment_params_t representatives;
    representatives.compact = false;
    pcp::gpu::device_array_t<float> d_normals(3 * n);
    d_normals.upload(normals.data(), 3 * n);

    auto const oa = pcp::gpu::smooth_segments(octree, normal_map, r, max_angle);
    auto const ka = pcp::gpu::smooth_segments(kdtree, normal_map, r, max_angle);
    auto const da = pcp::gpu::smooth_segments(octree, d_normals, r, max_angle);
    auto const kf = pcp::gpu::smooth_segments(kdtree, normal_map, r, max_angle, filtered);
    auto const df = pcp::gpu::smooth_segments(kdtree, d_normals, r, max_angle, filtered);
    auto const kr = pcp::gpu::smooth_segments(kdtree, normal_map, r, max_angle, representatives);

    bool const ok = dump(prefix + ".all.u32", oa.labels) && dump(prefix + ".filtered.u32", kf.labels) &&
                    dump(prefix + ".representatives.u32", kr.labels);
    bool const same = oa.labels == ka.labels && oa.labels == da.labels && oa.smooth == ka.smooth && oa.smooth == da.smooth &&
                      oa.segment_count == ka.segment_count && oa.segment_count == da.segment_count && kf.labels == df.labels &&
                      kf.segment_count == df.segment_count && kr.segment_count == oa.segment_count;
    std::size_t smooth = 0, noise = 0;
    for (std::size_t i = 0; i < n; ++i) smooth += kf.smooth[i], noise += kf.labels[i] == pcp::gpu::segments_t::noise ? 1u : 0u;
    std::printf("{\"points\": %zu, \"radius\": %.9g, \"max_angle\": %.9g, \"min_size\": %u, \"segments\": %llu, \"segments_filtered\": %llu, "
                "\"smooth\": %zu, \"noise_filtered\": %zu, \"routes_agree\": %s, \"written\": %s}\n",
                n, double(r), double(max_angle), min_size, static_cast<unsigned long long>(oa.segment_count),
                static_cast<unsigned long long>(kf.segment_count), smooth, noise, same ? "true" : "false", ok ? "true" : "false");
    return same && ok ? 0 : 4;
}
