// Drop-in check for the hierarchy branch of the reference's examples/downsample.cpp (:195-214): the same call SHAPE --
// hierarchy::params_t filled from a size_t and a double, hierarchy_simplification over a vector of std::size_t indices
// with a point map that returns a point BY VALUE, output through std::back_inserter into a vector of point_t -- plus the
// same call through a point map that returns a const reference, which must give the same points.
// usage: downsample_shape <in.ply> <cluster_size> <var_max> <out.bin>
// writes the kept points as raw float32 x, y, z; prints one JSON object with the counts
#include <pcp/algorithm/algorithm.hpp>
#include <pcp/common/normals/normal.hpp>
#include <pcp/common/points/point.hpp>
#include <pcp/io/ply.hpp>

#include <cstdio>
#include <cstdlib>
#include <filesystem>
#include <iterator>
#include <numeric>
#include <vector>

int main(int argc, char** argv)
{
    if (argc < 5) return 2;
    auto [input_point_cloud, normals] = pcp::io::read_ply<pcp::point_t, pcp::normal_t>(std::filesystem::path{argv[1]});
    (void)normals;
    std::vector<std::size_t> indices(input_point_cloud.size());
    std::iota(indices.begin(), indices.end(), std::size_t{0});
    auto const point_map = [&](std::size_t const i) { return input_point_cloud[i]; };

    std::vector<pcp::point_t> output_point_cloud;
    output_point_cloud.clear();
    pcp::algorithm::hierarchy::params_t params;
    params.cluster_size = static_cast<std::size_t>(std::strtoull(argv[2], nullptr, 10));
    params.var_max      = static_cast<double>(std::strtod(argv[3], nullptr));
    pcp::algorithm::hierarchy_simplification(indices.begin(), indices.end(), std::back_inserter(output_point_cloud), point_map, params);

    // the same over the points themselves, through a map that returns a reference, into a preallocated range
    auto const by_reference = [](pcp::point_t const& p) -> pcp::point_t const& { return p; };
    std::vector<pcp::point_t> again(input_point_cloud.size());
    auto const last = pcp::algorithm::hierarchy_simplification(input_point_cloud.begin(), input_point_cloud.end(), again.begin(),
                                                               by_reference, params);
    again.erase(last, again.end());
    bool same = again.size() == output_point_cloud.size();
    for (std::size_t i = 0; same && i < again.size(); ++i)
        same = again[i].x() == output_point_cloud[i].x() && again[i].y() == output_point_cloud[i].y() && again[i].z() == output_point_cloud[i].z();

    std::FILE* f = std::fopen(argv[4], "wb");
    if (!f) return 3;
    for (auto const& p : output_point_cloud)
    {
        float const xyz[3] = {p.x(), p.y(), p.z()};
        std::fwrite(xyz, sizeof(float), 3, f);
    }
    std::fclose(f);
    std::printf("{\"input\": %zu, \"kept\": %zu, \"by_reference_same\": %s}\n", input_point_cloud.size(), output_point_cloud.size(),
                same ? "true" : "false");
    return same ? 0 : 1;
}
