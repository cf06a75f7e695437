// pcp::gpu::voxel_grid_downsample -- voxel-grid downsampling on the GPU (include/pcpx_voxel.h): the points of
// every occupied cell of a regular grid replaced by their centroid, attributes averaged with them, cells in ascending key order and
// every bit defined.  Not part of the reference API: the reference has no voxel filter.  No container is involved: the cloud is a
// flat row-major x, y, z array.
#ifndef PCP_GPU_VOXEL_GRID_HPP
#define PCP_GPU_VOXEL_GRID_HPP

#include "pcp/gpu/device_index.hpp"
#include "pcpx_voxel.h"

#include <array>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace pcp {
namespace gpu {

struct voxel_grid_options_t
{
    float const* origin      = nullptr; // 3 floats; nullptr: the per-axis minimum of the finite points
    float const* attributes  = nullptr; // n x attribute_columns
    std::uint32_t attribute_columns = 0u; // at most PCPX_VOXEL_ATTRS_MAX
    int device               = 0;
};

struct voxel_grid_result_t
{
    std::vector<float> points;         // V x 3: the centroids
    std::vector<float> attributes;     // V x attribute_columns: the means
    std::vector<std::uint32_t> counts; // V: the points of every cell
    std::vector<std::uint64_t> keys;   // V, ascending: c_z * 2^42 + c_y * 2^21 + c_x
    std::vector<std::uint32_t> rows;   // V: the cell's point nearest its centroid
    std::vector<std::uint32_t> owner;  // n: the cell of every point, PCPX_VOXEL_NONE for a dropped one
    std::uint64_t dropped = 0;         // points with a non-finite coordinate or outside the grid's 2^21 cells per axis
    std::array<float, 3> origin{};
    std::size_t size() const { return counts.size(); }
};

// points: n x 3.  leaf: the cell's three edges.  Two calls: the first counts the cells, the second fills arrays of that size.
inline voxel_grid_result_t voxel_grid_downsample(float const* points, std::size_t n, std::array<float, 3> const& leaf,
                                                 voxel_grid_options_t const& options = {})
{
    pcpx_voxel_params p{};
    for (int j = 0; j < 3; ++j) p.leaf[j] = leaf[static_cast<std::size_t>(j)];
    if (options.origin) {
        for (int j = 0; j < 3; ++j) p.origin[j] = options.origin[j];
        p.flags = PCPX_VOXEL_ORIGIN;
    }
    p.attr_columns = options.attributes ? options.attribute_columns : 0u;
    voxel_grid_result_t r;
    std::uint64_t count = 0;
    int const sized = pcpx_voxel_grid(points, n, options.attributes, &p, 0, options.device, &count, nullptr, nullptr, nullptr, nullptr, nullptr,
                                      nullptr, nullptr, nullptr);
    if (sized != PCPX_ERR_CAPACITY) check(sized, "pcpx_voxel_grid");
    if (n == 0) return r;
    std::size_t const V = static_cast<std::size_t>(count), room = V ? V : 1;
    r.points.resize(room * 3);
    r.attributes.resize(room * p.attr_columns);
    r.counts.resize(room);
    r.keys.resize(room);
    r.rows.resize(room);
    r.owner.resize(n);
    check(pcpx_voxel_grid(points, n, options.attributes, &p, room, options.device, &count, r.points.data(), p.attr_columns ? r.attributes.data() : nullptr,
                          r.counts.data(), r.keys.data(), r.rows.data(), r.owner.data(), &r.dropped, r.origin.data()),
          "pcpx_voxel_grid");
    r.points.resize(V * 3);
    r.attributes.resize(V * p.attr_columns);
    r.counts.resize(V);
    r.keys.resize(V);
    r.rows.resize(V);
    return r;
}

} // namespace gpu
} // namespace pcp

#endif
