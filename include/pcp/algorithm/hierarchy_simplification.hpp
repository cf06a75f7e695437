// pcp::algorithm::hierarchy_simplification -- drop-in for include/pcp/algorithm/hierarchy_simplification.hpp (:63-149;
// params_t :20-27): Pauly et al.'s hierarchy simplification.  A cluster (at first the whole input) is split by the plane
// through its mean normal to its largest eigenvector while it holds more than cluster_size points or its variation
// lambda0 / (lambda0 + lambda1 + lambda2) exceeds var_max; otherwise the point nearest to its mean is kept.  Same
// signature, same output order (the reference's queue: breadth first, first child before second), same return value.
// The whole recursion is one call into libpcpx (pcpx_hierarchy_simplification), level by level on the GPU, with the
// decisions taken in double; where that departs from the reference (the sign of the normal, which picks the first child;
// a split that would leave a side empty ends as a leaf instead of looping) is in include/pcpx.h and DESIGN.md section 14.
// Eigen is not needed: covariance / pca / eigen_sorted are not part of this header.
#ifndef PCP_ALGORITHM_HIERARCHY_SIMPLIFICATION_HPP
#define PCP_ALGORITHM_HIERARCHY_SIMPLIFICATION_HPP

#include "pcp/gpu/device_index.hpp"
#include "pcp/traits/output_iterator_traits.hpp"

#include <cstddef>
#include <cstdint>
#include <iterator>
#include <stdexcept>
#include <vector>

namespace pcp {
namespace algorithm {
namespace hierarchy {

struct params_t
{
    std::size_t cluster_size = 0u; ///< Maximum size of subdivided clusters
    double var_max = 1. / 3.;      ///< Maximum variation permitted after which a cluster will be subdivided
};

} // namespace hierarchy

template <class RandomAccessIter, class OutputIter, class PointMap>
OutputIter hierarchy_simplification(
    RandomAccessIter begin,
    RandomAccessIter end,
    OutputIter out_begin,
    PointMap const& point_map,
    hierarchy::params_t const& params)
{
    using output_point_type = typename xstd::output_iterator_traits<OutputIter>::value_type;
    using T                 = typename output_point_type::coordinate_type;
    // the reference asserts cluster_size > 0 and var_max >= 0 (:89-90)
    if (params.cluster_size == 0u || !(params.var_max >= 0.))
        throw std::invalid_argument("hierarchy_simplification: need cluster_size > 0 and var_max >= 0");
    std::size_t const n = static_cast<std::size_t>(std::distance(begin, end));
    std::vector<float> xyz;
    xyz.reserve(3u * n);
    for (RandomAccessIter it = begin; it != end; ++it)
    {
        auto const& p = point_map(*it);  // (binds to a returned value as well as to a returned reference)
        xyz.push_back(static_cast<float>(p.x()));
        xyz.push_back(static_cast<float>(p.y()));
        xyz.push_back(static_cast<float>(p.z()));
    }
    pcpx_hierarchy_params prm{};
    prm.struct_size  = sizeof(pcpx_hierarchy_params);
    prm.cluster_size = static_cast<std::uint64_t>(params.cluster_size);
    prm.var_max      = params.var_max;
    std::vector<float> out(3u * n);
    std::uint64_t count = 0;
    gpu::check(pcpx_hierarchy_simplification(xyz.data(), n, &prm, 0, out.data(), nullptr, n, &count), "pcpx_hierarchy_simplification");
    for (std::uint64_t i = 0; i < count; ++i)
        *out_begin++ = output_point_type{static_cast<T>(out[3 * i]), static_cast<T>(out[3 * i + 1]), static_cast<T>(out[3 * i + 2])};
    return out_begin;
}

} // namespace algorithm
} // namespace pcp

#endif
