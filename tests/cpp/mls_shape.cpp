// pcp::gpu::mls_project / mls_project_device (include/pcp/gpu/mls.hpp) through both drop-in containers -- an octree of point views
// and a K = 3 kd-tree over index elements --, host and device routes, both orders.
// usage: mls_shape <in.ply> <radius> <gauss_h>
// prints one JSON object; exit status 0 when the routes agree
#include <pcp/gpu/mls.hpp>
#include <pcp/pcp.hpp>

#include <array>
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
bool same(pcp::gpu::mls_t const& a, pcp::gpu::mls_t const& b)
{
    return same_bits(a.points, b.points) && same_bits(a.displacements, b.displacements) && same_bits(a.normals, b.normals) &&
           same_bits(a.curvatures, b.curvatures) && a.count == b.count && a.fit == b.fit;
}
} // namespace

int main(int argc, char** argv)
{
    if (argc < 4) return 2;
    using point_type      = pcp::point_t;
    using point_view_type = pcp::point_view_t;
    using normal_type     = pcp::normal_t;
    float const r         = std::strtof(argv[2], nullptr);
    float const h         = std::strtof(argv[3], nullptr);

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

    bool agree = true;
    std::size_t fits[2][3] = {{0, 0, 0}, {0, 0, 0}};
    std::uint64_t neighbours = 0;
    for (int order = 1; order <= 2; ++order)
    {
        auto const om = pcp::gpu::mls_project(octree, r, h, order);
        auto const km = pcp::gpu::mls_project(kdtree, r, h, order);
        auto const dm = pcp::gpu::mls_project_device(octree, r, h, order);
        pcp::gpu::mls_t down;
        down.points        = dm.points.download();
        down.displacements = dm.displacements.download();
        down.normals       = dm.normals.download();
        down.curvatures    = dm.curvatures.download();
        down.count         = dm.count.download();
        down.fit           = dm.fit.download();
        agree              = agree && same(om, km) && same(om, down) && om.points.size() == 3 * n && om.curvatures.size() == 2 * n;
        for (std::size_t i = 0; i < n; ++i)
        {
            if (om.fit[i] > 2u) return 5;
            fits[order - 1][om.fit[i]] += 1;
            if (order == 2) neighbours += om.count[i];
        }
    }
    std::printf("{\"points\": %zu, \"radius\": %.9g, \"gauss_h\": %.9g, \"order1_fits\": [%zu, %zu, %zu], \"order2_fits\": [%zu, %zu, %zu], "
                "\"neighbours\": %llu, \"routes_agree\": %s}\n",
                n, double(r), double(h), fits[0][0], fits[0][1], fits[0][2], fits[1][0], fits[1][1], fits[1][2],
                static_cast<unsigned long long>(neighbours), agree ? "true" : "false");
    return agree ? 0 : 4;
}
