// pcp::gpu::cloud_resolution, statistical_outlier_removal, radius_outlier_removal and density_outlier_removal -- the elements of a
// container that survive an outlier filter, on the GPU (include/pcpx_outliers.h).  Not part of the reference
// API; density_outlier_removal is the reference's examples/filter_point_cloud_noise_by_density.cpp -- its ball radius and its
// remove_if -- as one call.  For any container with `.index().handle()` and `.size()`: pcp::basic_linked_octree_t and
// pcp::basic_linked_kdtree_t with K <= 3.
#ifndef PCP_GPU_OUTLIERS_HPP
#define PCP_GPU_OUTLIERS_HPP

#include "pcp/gpu/device_index.hpp"
#include "pcpx_outliers.h"

#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

namespace pcp {
namespace gpu {

// mean and sample standard deviation of the mean distance to the k nearest neighbours, over the `usable` elements (those with a
// finite mean distance); float64 sums in one fixed order, so every bit depends on the elements alone
struct resolution_t
{
    double mean          = std::numeric_limits<double>::quiet_NaN();
    double std           = std::numeric_limits<double>::quiet_NaN();
    std::uint64_t usable = 0u;
};

struct outliers_t
{
    std::vector<std::uint32_t> kept;  // the kept elements, ascending, in the container's element order
    resolution_t resolution;          // statistical and density filter: of the k they were given
    float cut = std::numeric_limits<float>::quiet_NaN();  // the distance threshold (statistical) or the radius (density, radius)
};

namespace detail {
inline resolution_t resolution_of(double const (&stats)[4])
{
    resolution_t r;
    r.mean   = stats[0];
    r.std    = stats[1];
    r.usable = static_cast<std::uint64_t>(stats[3]);
    return r;
}
} // namespace detail

template <class Tree>
resolution_t cloud_resolution(Tree const& tree, std::uint32_t k = 15u, float eps = 1e-5f)
{
    if (tree.size() == 0) return resolution_t{};
    double stats[4];
    check(pcpx_outliers_resolution_self(tree.index().handle(), k, eps, 0u, nullptr, stats), "pcpx_outliers_resolution_self");
    return detail::resolution_of(stats);
}

// Element i is kept iff its mean distance d_i to its k nearest neighbours is finite and d_i <= float(mean + std_ratio * std).
template <class Tree>
outliers_t statistical_outlier_removal(Tree const& tree, std::uint32_t k = 15u, float std_ratio = 2.f, float eps = 1e-5f)
{
    outliers_t out;
    std::size_t const n = tree.size();
    if (n == 0) return out;
    std::vector<std::uint8_t> keep(n);
    out.kept.resize(n);
    std::uint64_t count = 0;
    double stats[4];
    check(pcpx_outliers_statistical_self(tree.index().handle(), k, eps, std_ratio, 0u, keep.data(), out.kept.data(), &count, nullptr, stats),
          "pcpx_outliers_statistical_self");
    out.kept.resize(static_cast<std::size_t>(count));
    out.resolution = detail::resolution_of(stats);
    out.cut        = static_cast<float>(stats[2]);
    return out;
}

// Element i is kept iff at least max(min_neighbours, 1) elements, itself included, are within `radius` (float32, the rule of
// range_search(sphere_t)): `range_search(ball).size() < min_neighbours` drops it.
template <class Tree>
outliers_t radius_outlier_removal(Tree const& tree, float radius, std::uint32_t min_neighbours = 5u)
{
    outliers_t out;
    std::size_t const n = tree.size();
    if (n == 0) return out;
    std::vector<std::uint8_t> keep(n);
    out.kept.resize(n);
    std::uint64_t count = 0;
    check(pcpx_outliers_radius_self(tree.index().handle(), radius, min_neighbours, 0u, keep.data(), out.kept.data(), &count, nullptr),
          "pcpx_outliers_radius_self");
    out.kept.resize(static_cast<std::size_t>(count));
    out.cut = radius;
    return out;
}

// radius_outlier_removal at float(radius_scale * mean) with the mean of cloud_resolution(tree, k): the radius is formed and used
// on the device, and comes back in `cut`.
template <class Tree>
outliers_t density_outlier_removal(Tree const& tree, std::uint32_t k = 15u, float radius_scale = 1.f, std::uint32_t min_neighbours = 5u,
                                   float eps = 1e-5f)
{
    outliers_t out;
    std::size_t const n = tree.size();
    if (n == 0) return out;
    std::vector<std::uint8_t> keep(n);
    out.kept.resize(n);
    std::uint64_t count = 0;
    double stats[4];
    check(pcpx_outliers_density_self(tree.index().handle(), k, eps, radius_scale, min_neighbours, 0u, keep.data(), out.kept.data(), &count,
                                     nullptr, stats),
          "pcpx_outliers_density_self");
    out.kept.resize(static_cast<std::size_t>(count));
    out.resolution = detail::resolution_of(stats);
    out.cut        = static_cast<float>(stats[2]);
    return out;
}

} // namespace gpu
} // namespace pcp

#endif
