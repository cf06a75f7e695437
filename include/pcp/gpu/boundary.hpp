// pcp::gpu::boundary_points -- the elements of a container that lie on the border of the sampled surface (the rim of an open scan,
// the edges of its holes), by the largest empty angle between the directions to an element's neighbours in its tangent plane, on
// the GPU (include/pcpx_boundary.h; PCL's BoundaryEstimation).  Not part of the reference API, which has no
// boundary detection.  For any container with `.index().handle()` and `.size()`: pcp::basic_linked_octree_t and
// pcp::basic_linked_kdtree_t with K <= 3.
#ifndef PCP_GPU_BOUNDARY_HPP
#define PCP_GPU_BOUNDARY_HPP

#include "pcp/gpu/device_index.hpp"
#include "pcpx_boundary.h"

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <vector>

namespace pcp {
namespace gpu {

struct boundary_params_t
{
    std::uint32_t gap_sectors    = 16u;  // 1 .. 64 sectors of 5.625 degrees: 16 = an empty angle of 90 degrees or more
    std::uint32_t min_neighbours = 1u;   // elements in the sphere, the element itself included
    bool want_gaps = false, want_counts = false, want_sectors = false;
};

struct boundary_t
{
    std::vector<std::uint32_t> kept;     // the boundary elements, ascending, in the container's element order
    std::vector<std::uint8_t> gaps;      // x 2 on request: the longest run of empty sectors and where it starts; 255 255: no frame
    std::vector<std::uint32_t> counts;   // on request: elements in the sphere
    std::vector<std::uint64_t> sectors;  // on request: bit s set iff a neighbour's direction lies in sector s
};

// the same on the index's device: nothing crosses PCIe (kept.data() and count.data() are what pcpx_boundary_self wrote)
struct device_boundary_t
{
    device_array_t<std::uint8_t> keep;   // one byte per element, 1 = on the boundary
    device_array_t<std::uint32_t> kept;  // room for every element; the first *count entries are written
    device_array_t<std::uint64_t> count; // one word
    device_array_t<std::uint8_t> gaps;
    device_array_t<std::uint32_t> counts;
    device_array_t<std::uint64_t> sectors;
};

// normals: three floats per element, in the container's element order, used as given (an element whose normal is not finite or
// is zero is never kept)
template <class Tree>
boundary_t boundary_points(Tree const& tree, std::vector<float> const& normals, float radius, boundary_params_t const& params = {})
{
    boundary_t out;
    std::size_t const n = tree.size();
    if (normals.size() != 3 * n) throw std::invalid_argument("pcp::gpu::boundary_points: three floats per element");
    if (n == 0) return out;
    std::vector<std::uint8_t> keep(n);
    out.kept.resize(n);
    if (params.want_gaps) out.gaps.resize(2 * n);
    if (params.want_counts) out.counts.resize(n);
    if (params.want_sectors) out.sectors.resize(n);
    std::uint64_t count = 0;
    check(pcpx_boundary_self(tree.index().handle(), normals.data(), radius, params.gap_sectors, params.min_neighbours, 0u, keep.data(),
                             out.kept.data(), &count, params.want_gaps ? out.gaps.data() : nullptr,
                             params.want_counts ? out.counts.data() : nullptr, params.want_sectors ? out.sectors.data() : nullptr),
          "pcpx_boundary_self");
    out.kept.resize(static_cast<std::size_t>(count));
    return out;
}

// Device arrays: `normals` is a device array of three floats per element (what range_neighbourhoods_self_dev left there).  Enqueued
// on the index's stream and not waited for: pcpx_index_synchronize, or work on the same stream, comes after it.
template <class Tree>
device_boundary_t boundary_points(Tree const& tree, device_array_t<float> const& normals, float radius, boundary_params_t const& params = {},
                                  int device = 0)
{
    device_boundary_t out;
    std::size_t const n = tree.size();
    if (normals.size() != 3 * n) throw std::invalid_argument("pcp::gpu::boundary_points: three floats per element");
    if (n == 0) return out;
    out.keep  = device_array_t<std::uint8_t>(n, device);
    out.kept  = device_array_t<std::uint32_t>(n, device);
    out.count = device_array_t<std::uint64_t>(1, device);
    if (params.want_gaps) out.gaps = device_array_t<std::uint8_t>(2 * n, device);
    if (params.want_counts) out.counts = device_array_t<std::uint32_t>(n, device);
    if (params.want_sectors) out.sectors = device_array_t<std::uint64_t>(n, device);
    check(pcpx_boundary_self(tree.index().handle(), normals.data(), radius, params.gap_sectors, params.min_neighbours, PCPX_BOUNDARY_ON_DEVICE,
                             out.keep.data(), out.kept.data(), out.count.data(), params.want_gaps ? out.gaps.data() : nullptr,
                             params.want_counts ? out.counts.data() : nullptr, params.want_sectors ? out.sectors.data() : nullptr),
          "pcpx_boundary_self");
    return out;
}

} // namespace gpu
} // namespace pcp

#endif
