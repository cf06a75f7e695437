// pcp::gpu::shape_features / surface_variation (include/pcp/gpu/shape_features.hpp) through both drop-in containers -- an octree
// of point views and a K = 3 kd-tree over index elements -- and the pipeline they exist for: normals and curvature on the device,
// handed to pcp::gpu::smooth_segments with a curvature gate, against the same through host arrays.
// usage: shape_features_shape <in.ply> <radius> <max_angle> <max_curvature>
// prints one JSON object (tests/test_gpu_shape_features.py compares its counts with Python's); exit status 0 when the routes agree
#include <pcp/gpu/segmentation.hpp>
#include <pcp/gpu/shape_features.hpp>
#include <pcp/pcp.hpp>

#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <numeric>
#include <vector>

namespace {
template <class T>
bool same_bits(std::vector<T> const& a, std::vector<T> const& b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}
struct raw_normal_t
{
    float a, b, c;
    float x() const { return a; }
    float y() const { return b; }
    float z() const { return c; }
};
} // namespace

int main(int argc, char** argv)
{
    if (argc < 5) return 2;
    using point_type      = pcp::point_t;
    using point_view_type = pcp::point_view_t;
    using normal_type     = pcp::normal_t;
    float const r         = std::strtof(argv[2], nullptr);
    float const max_angle = std::strtof(argv[3], nullptr);
    float const max_curv  = std::strtof(argv[4], nullptr);

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

    auto const of = pcp::gpu::shape_features(octree, r);
    auto const kf = pcp::gpu::shape_features(kdtree, r);
    auto const sv = pcp::gpu::surface_variation(kdtree, r);
    auto const df = pcp::gpu::shape_features_device(octree, r);
    bool const same_features = same_bits(of.evals, kf.evals) && same_bits(of.curvature, kf.curvature) && same_bits(of.normals, kf.normals) &&
                               same_bits(of.axes, kf.axes) && of.count == kf.count && same_bits(of.curvature, sv) &&
                               same_bits(of.evals, df.evals.download()) && same_bits(of.curvature, df.curvature.download()) &&
                               same_bits(of.normals, df.normals.download()) && same_bits(of.axes, df.axes.download()) &&
                               of.count == df.count.download();

    // normals -> curvature -> curvature-gated segmentation: on the device, and through host arrays
    pcp::gpu::segment_params_t on_device;
    on_device.curvature     = df.curvature.data();
    on_device.max_curvature = max_curv;
    auto const ds           = pcp::gpu::smooth_segments(octree, df.normals, r, max_angle, on_device);
    pcp::gpu::segment_params_t on_host;
    on_host.curvature     = of.curvature.data();
    on_host.max_curvature = max_curv;
    auto const normal_map = [&](std::size_t i) { return raw_normal_t{of.normals[3 * i], of.normals[3 * i + 1], of.normals[3 * i + 2]}; };
    auto const hs         = pcp::gpu::smooth_segments(kdtree, normal_map, r, max_angle, on_host);
    bool const same_segments = ds.labels == hs.labels && ds.smooth == hs.smooth && ds.segment_count == hs.segment_count;

    std::size_t smooth = 0, noise = 0, below = 0;
    std::uint64_t neighbours = 0;
    for (std::size_t i = 0; i < n; ++i)
    {
        smooth += ds.smooth[i];
        noise += ds.labels[i] == pcp::gpu::segments_t::noise ? 1u : 0u;
        below += of.curvature[i] <= max_curv ? 1u : 0u;
        neighbours += of.count[i];
    }
    std::printf("{\"points\": %zu, \"radius\": %.9g, \"max_angle\": %.9g, \"max_curvature\": %.9g, \"segments\": %llu, \"smooth\": %zu, "
                "\"noise\": %zu, \"below_threshold\": %zu, \"neighbours\": %llu, \"features_agree\": %s, \"segments_agree\": %s}\n",
                n, double(r), double(max_angle), double(max_curv), static_cast<unsigned long long>(ds.segment_count), smooth, noise, below,
                static_cast<unsigned long long>(neighbours), same_features ? "true" : "false", same_segments ? "true" : "false");
    return same_features && same_segments ? 0 : 4;
}
