// Farthest point sampling through the C++ layer: read a cloud, build a tree over point views, take m samples with
// pcp::gpu::farthest_point_sample (include/pcp/gpu/farthest_points.hpp) -- once through host vectors and once with every output
// left on the device -- and write the sampled points in selection order.  tests/test_gpu_fps.py runs it and compares with the
// numpy model.
// usage: fps_shape <in.ply> <out.ply> <m> [stop radius = 0]
// prints one JSON object: cloud size, samples of both paths, whether the two paths agree bit for bit
#include <pcp/gpu/farthest_points.hpp>
#include <pcp/pcp.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <vector>

namespace {
bool same_bits(std::vector<float> const& a, std::vector<float> const& b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0);
}
} // namespace

int main(int argc, char** argv)
{
    if (argc < 4) return 2;
    std::size_t const m = static_cast<std::size_t>(std::strtoull(argv[3], nullptr, 10));
    pcp::gpu::fps_params_t params;
    if (argc > 4) params.stop_radius = std::strtof(argv[4], nullptr);
    params.want_d2 = params.want_min_d2 = params.want_owner = params.want_evaluations = true;

    auto [cloud, file_normals] = pcp::io::read_ply<pcp::point_t, pcp::normal_t>(std::filesystem::path{argv[1]});
    (void)file_normals;
    if (cloud.empty()) return 1;
    std::size_t const n = cloud.size();

    std::vector<pcp::point_view_t> views;
    views.reserve(n);
    for (auto& p : cloud) views.push_back(pcp::point_view_t{&p});
    auto const identity = [](pcp::point_view_t const& v) { return v; };
    pcp::basic_linked_octree_t<pcp::point_view_t> tree{views.begin(), views.end(), identity};
    if (tree.size() != n) return 3;

    // host vectors
    auto const host = pcp::gpu::farthest_point_sample(tree, m, params);

    // device arrays: one wait at the end
    pcp::gpu::device_fps_t dev;
    pcp::gpu::farthest_point_sample(tree, m, dev, params);
    pcp::gpu::check(pcpx_index_synchronize(tree.index().handle()), "pcpx_index_synchronize");
    std::uint64_t const dev_count = dev.count.download()[0];
    std::size_t const c = static_cast<std::size_t>(dev_count);
    bool same = c == host.samples.size() && dev.samples.download(0, c) == host.samples && same_bits(dev.d2.download(0, c), host.d2);
    same = same && same_bits(dev.min_d2.download(), host.min_d2) && dev.owner.download() == host.owner;
    same = same && dev.evaluations.download()[0] == host.evaluations;

    std::vector<pcp::point_t> sampled;
    sampled.reserve(host.samples.size());
    for (std::uint32_t const i : host.samples) sampled.push_back(cloud[i]);
    pcp::io::write_ply(std::filesystem::path{argv[2]}, sampled, std::vector<pcp::normal_t>{}, pcp::io::ply_format_t::binary_little_endian);

    std::printf("{\"points\": %zu, \"samples\": %zu, \"device_samples\": %llu, \"evaluations\": %llu, \"same\": %s}\n", n, host.samples.size(),
                static_cast<unsigned long long>(dev_count), static_cast<unsigned long long>(host.evaluations), same ? "true" : "false");
    return same ? 0 : 4;
}
