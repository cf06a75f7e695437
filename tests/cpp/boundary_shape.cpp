// The border of a scanned surface through the C++ layer: read a cloud, build a tree over point views, estimate fixed-radius normals,
// find the boundary elements with pcp::gpu::boundary_points (include/pcp/gpu/boundary.hpp) -- once through host vectors and once
// with the normals and every output left on the device -- and write the boundary points.  tests/test_gpu_boundary.py runs it and
// compares with the Python binding and the numpy model.
// usage: boundary_shape <in.ply> <out.ply> <radius> [gap sectors = 16] [min neighbours = 1]
// prints one JSON object: cloud size, boundary points of both paths, whether the two paths agree row for row
#include <pcp/gpu/boundary.hpp>
#include <pcp/pcp.hpp>
#include <pcpx_radius.h>

#include <cstdio>
#include <cstdlib>
#include <filesystem>
#include <vector>

int main(int argc, char** argv)
{
    if (argc < 4) return 2;
    float const radius = std::strtof(argv[3], nullptr);
    pcp::gpu::boundary_params_t params;
    if (argc > 4) params.gap_sectors = static_cast<std::uint32_t>(std::strtoul(argv[4], nullptr, 10));
    if (argc > 5) params.min_neighbours = static_cast<std::uint32_t>(std::strtoul(argv[5], nullptr, 10));
    params.want_gaps = params.want_counts = params.want_sectors = true;

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
    std::vector<float> normals(3 * n);
    tree.index().range_neighbourhoods_self(radius, n, normals.data(), nullptr, nullptr, nullptr);
    auto const host = pcp::gpu::boundary_points(tree, normals, radius, params);

    // device arrays: normals -> boundary without a copy in between, one wait at the end
    pcp::gpu::device_array_t<float> d_normals(3 * n);
    pcp::gpu::check(pcpx_range_neighbourhoods_self_dev(tree.index().handle(), radius, 0, UINT64_MAX, d_normals.data(), nullptr, nullptr, nullptr),
                    "pcpx_range_neighbourhoods_self_dev");
    auto const dev = pcp::gpu::boundary_points(tree, d_normals, radius, params);
    pcp::gpu::check(pcpx_index_synchronize(tree.index().handle()), "pcpx_index_synchronize");
    std::uint64_t const dev_count = dev.count.download()[0];
    bool same = dev_count == host.kept.size() && dev.kept.download(0, static_cast<std::size_t>(dev_count)) == host.kept;
    same = same && dev.gaps.download() == host.gaps && dev.counts.download() == host.counts && dev.sectors.download() == host.sectors;
    std::vector<std::uint8_t> const keep = dev.keep.download();
    std::size_t kept_flags = 0;
    for (std::uint8_t const k : keep) kept_flags += k;
    same = same && kept_flags == host.kept.size();

    std::vector<pcp::point_t> border;
    border.reserve(host.kept.size());
    for (std::uint32_t const i : host.kept) border.push_back(cloud[i]);
    pcp::io::write_ply(std::filesystem::path{argv[2]}, border, std::vector<pcp::normal_t>{}, pcp::io::ply_format_t::binary_little_endian);

    std::printf("{\"points\": %zu, \"boundary\": %zu, \"device_boundary\": %llu, \"same\": %s}\n", n, host.kept.size(),
                static_cast<unsigned long long>(dev_count), same ? "true" : "false");
    return same ? 0 : 4;
}
