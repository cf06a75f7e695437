// pcp::gpu::local_maxima and pcp::gpu::iss_keypoints -- the elements of a container that are the maxima of a per-element score over
// a radius (sphere-wise non-maximum suppression), and the ISS keypoints (Zhong 2009) of the container's own elements, on the GPU
// (include/pcpx_keypoints.h).  Not part of the reference API.  For any container with `.index().handle()`
// and `.size()`: pcp::basic_linked_octree_t and pcp::basic_linked_kdtree_t with K <= 3.
#ifndef PCP_GPU_KEYPOINTS_HPP
#define PCP_GPU_KEYPOINTS_HPP

#include "pcp/gpu/device_index.hpp"
#include "pcpx_keypoints.h"

#include <cstdint>
#include <limits>
#include <stdexcept>
#include <vector>

namespace pcp {
namespace gpu {

struct keypoints_t
{
    std::vector<std::uint32_t> kept;  // the kept elements, ascending, in the container's element order
    std::vector<float> saliency;      // iss_keypoints: one per element, l0 / count where the eigenvalue ratios pass, else NaN
};

struct iss_params_t
{
    float salient_radius         = 0.f;
    float non_max_radius         = 0.f;
    float gamma21                = 0.975f;
    float gamma32                = 0.975f;
    std::uint32_t min_neighbours = 5u;
};

// Element i is kept iff its score is not NaN and >= min_score, no element j within `radius` (float32, the rule of
// range_search(sphere_t)) has score_j > score_i or score_j == score_i and j < i, and at least min_neighbours elements (itself
// included) are within `radius`.  Exact and the same on every run.  No two kept elements are within `radius` of each other; a
// dropped element need NOT have a kept one nearby (poisson_disk_subsample promises that, this does not).  Minima: negate the score.
template <class Tree>
keypoints_t local_maxima(Tree const& tree, std::vector<float> const& score, float radius,
                         float min_score = -std::numeric_limits<float>::infinity(), std::uint32_t min_neighbours = 1u)
{
    keypoints_t out;
    std::size_t const n = tree.size();
    if (score.size() != n) throw std::invalid_argument("pcp::gpu::local_maxima: one score per element");
    if (n == 0) return out;
    std::vector<std::uint8_t> keep(n);
    out.kept.resize(n);
    std::uint64_t count = 0;
    check(pcpx_local_maxima_self(tree.index().handle(), score.data(), radius, min_score, min_neighbours, 0u, keep.data(), out.kept.data(),
                                 &count),
          "pcpx_local_maxima_self");
    out.kept.resize(static_cast<std::size_t>(count));
    return out;
}

// The local maxima, over non_max_radius, of the smallest eigenvalue of the covariance of every element's salient_radius
// neighbourhood, among the elements whose eigenvalue ratios l1 / l2 and l0 / l1 are below gamma21 and gamma32.
template <class Tree>
keypoints_t iss_keypoints(Tree const& tree, iss_params_t const& params)
{
    keypoints_t out;
    std::size_t const n = tree.size();
    if (n == 0) return out;
    std::vector<std::uint8_t> keep(n);
    out.kept.resize(n);
    out.saliency.resize(n);
    std::uint64_t count = 0;
    check(pcpx_iss_keypoints_self(tree.index().handle(), params.salient_radius, params.non_max_radius, params.gamma21, params.gamma32,
                                  params.min_neighbours, 0u, keep.data(), out.kept.data(), &count, out.saliency.data()),
          "pcpx_iss_keypoints_self");
    out.kept.resize(static_cast<std::size_t>(count));
    return out;
}

} // namespace gpu
} // namespace pcp

#endif
