// pcp::gpu::ransac_rigid / rigid_fit -- rigid registration from correspondences on the GPU (include/pcpx_register.h, DESIGN.md section
// 24): the rigid pose that most of a list of (source, target) pairs agree on, by a fixed number of three-pair hypotheses each scored
// against all pairs, and the least-squares rigid fit over a list of pairs.  Not part of the reference API: the reference has no
// registration.  No container is involved: the clouds are flat row-major x, y, z arrays, the pairs what
// pcp::gpu::match_correspondences returns or a flat array of {source, target}.  Transforms are row-major 4 x 4 and take points of
// p to points of q.
#ifndef PCP_GPU_REGISTRATION_HPP
#define PCP_GPU_REGISTRATION_HPP

#include "pcp/gpu/device_index.hpp"
#include "pcp/gpu/matching.hpp"
#include "pcpx_register.h"

#include <array>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace pcp {
namespace gpu {

using transform_t = std::array<double, 16>;

struct ransac_result_t
{
    bool found               = false;
    std::uint32_t hypothesis = 0;
    transform_t transform{}; // the winning hypothesis itself
    transform_t refit{};     // the least-squares transform over its inliers (the hypothesis again when refit was not asked for)
    std::vector<std::uint32_t> inliers; // positions into the pairs, ascending
};

struct rigid_fit_result_t
{
    transform_t transform{};
    double rms = 0.;
};

// p: np x 3, q: nq x 3, pairs: count x {row of p, row of q}.  A pair is an inlier when its target lies within max_distance of its
// moved source; edge_similarity s in [0, 1] rejects a sampled triple one of whose edges is shorter than s times its partner (0: no
// gate).  Both are squared in float32 here.  Ties in the inlier count go to the lowest hypothesis.
inline ransac_result_t ransac_rigid(float const* p, std::size_t np, float const* q, std::size_t nq, std::uint32_t const* pairs, std::size_t count,
                                    std::uint64_t hypotheses, float max_distance, std::uint32_t seed = 0u, float edge_similarity = 0.f,
                                    bool refit = true, int device = 0)
{
    ransac_result_t r;
    r.inliers.resize(count);
    std::uint32_t found = 0, score = 0;
    check(pcpx_ransac_rigid(p, np, q, nq, pairs, count, hypotheses, seed, max_distance * max_distance, edge_similarity * edge_similarity,
                            refit ? PCPX_RANSAC_REFIT : 0u, device, &found, &r.hypothesis, &score, r.inliers.data(), r.transform.data(),
                            refit ? r.refit.data() : nullptr),
          "pcpx_ransac_rigid");
    r.found = found != 0;
    r.inliers.resize(score);
    if (!refit) r.refit = r.transform;
    return r;
}

// the same over what pcp::gpu::match_correspondences returns
inline ransac_result_t ransac_rigid(float const* p, std::size_t np, float const* q, std::size_t nq, std::vector<correspondence_t> const& pairs,
                                    std::uint64_t hypotheses, float max_distance, std::uint32_t seed = 0u, float edge_similarity = 0.f,
                                    bool refit = true, int device = 0)
{
    std::vector<std::uint32_t> flat(2 * pairs.size());
    for (std::size_t k = 0; k < pairs.size(); ++k) flat[2 * k] = pairs[k].source, flat[2 * k + 1] = pairs[k].target;
    return ransac_rigid(p, np, q, nq, flat.data(), pairs.size(), hypotheses, max_distance, seed, edge_similarity, refit, device);
}

// The rigid transform minimising the sum of |R p + t - q|^2 over the pairs (positions == nullptr: all of them; else those at the
// listed positions), float64 throughout, R always a proper rotation; the identity and a NaN rms with fewer than three usable pairs.
inline rigid_fit_result_t rigid_fit(float const* p, std::size_t np, float const* q, std::size_t nq, std::uint32_t const* pairs, std::size_t count,
                                    std::uint32_t const* positions = nullptr, std::size_t positions_count = 0, int device = 0)
{
    rigid_fit_result_t r;
    check(pcpx_rigid_fit(p, np, q, nq, pairs, count, positions, positions_count, device, r.transform.data(), &r.rms), "pcpx_rigid_fit");
    return r;
}

} // namespace gpu
} // namespace pcp

#endif
