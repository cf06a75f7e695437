// pcp::gpu::smooth_segments -- the smooth surface patches of a container's own elements on the GPU: normal-constrained region
// growing (Rabbani et al. 2006) in its order-independent form (include/pcpx_segment.h).  Not part of the
// reference API: the reference estimates, orients and filters normals and has no consumer that says which elements form one
// smooth patch.  For any container with `.index().handle()` and `.size()`: pcp::basic_linked_octree_t and
// pcp::basic_linked_kdtree_t with K <= 3.
#ifndef PCP_GPU_SEGMENTATION_HPP
#define PCP_GPU_SEGMENTATION_HPP

#include "pcp/gpu/device_index.hpp"
#include "pcpx_segment.h"

#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

namespace pcp {
namespace gpu {

struct segments_t
{
    static constexpr std::uint32_t noise = PCPX_SEGMENT_NOISE;
    std::vector<std::uint32_t> labels;  // one per element, in the container's element order: 0 ... segment_count - 1, or noise
    std::vector<std::uint8_t> smooth;   // 1 = smooth element (a vertex of the growth; the others can only join as border)
    std::uint64_t segment_count = 0;
};

struct segment_params_t
{
    float const* curvature = nullptr;  // one per element (host array; device array in the device form), or none: every element is smooth
    float max_curvature    = std::numeric_limits<float>::infinity();  // smooth iff curvature <= max_curvature
    std::uint32_t min_size = 1;        // segments of fewer elements become noise
    bool oriented          = false;    // the normals' signs matter: n_i . n_j >= cos(max_angle) instead of |n_i . n_j|
    bool compact           = true;     // false: a segment is labelled with its smallest smooth element index
};

// the cosine threshold of the C ABI from an angle in radians
inline float segment_min_cos(float max_angle) { return static_cast<float>(std::cos(static_cast<double>(max_angle))); }

inline std::uint32_t segment_flags(segment_params_t const& params)
{
    return (params.compact ? PCPX_SEGMENT_COMPACT : 0u) | (params.oriented ? PCPX_SEGMENT_ORIENTED : 0u);
}

// Elements i, j are joined iff |p_i - p_j|^2 <= radius^2 (float32, the rule of range_search(sphere_t)) and their normals agree
// within max_angle (radians); segments are the connected components of the smooth elements under that.  normal_map(i) gives
// the normal of element i of the container's element order (anything with x(), y(), z()); normals are used as given.
template <class Tree, class NormalMap>
segments_t smooth_segments(Tree const& tree, NormalMap const& normal_map, float radius, float max_angle, segment_params_t const& params = {})
{
    segments_t out;
    std::size_t const n = tree.size();
    out.labels.assign(n, segments_t::noise);
    out.smooth.assign(n, std::uint8_t{0});
    if (n == 0) return out;
    std::vector<float> normals(3 * n);
    for (std::size_t i = 0; i < n; ++i)
    {
        auto const nrm     = normal_map(i);
        normals[3 * i]     = static_cast<float>(nrm.x());
        normals[3 * i + 1] = static_cast<float>(nrm.y());
        normals[3 * i + 2] = static_cast<float>(nrm.z());
    }
    check(pcpx_segment_self(tree.index().handle(), normals.data(), params.curvature, radius, segment_min_cos(max_angle), params.max_curvature,
                            params.min_size, segment_flags(params), out.labels.data(), out.smooth.data(), &out.segment_count),
          "pcpx_segment_self");
    return out;
}

// The same with the normals (n x 3 float32, element order) and params.curvature already on the index's device: nothing but the
// results crosses PCIe.
template <class Tree>
segments_t smooth_segments(Tree const& tree, device_array_t<float> const& d_normals, float radius, float max_angle,
                           segment_params_t const& params = {}, int device = 0)
{
    segments_t out;
    std::size_t const n = tree.size();
    out.labels.assign(n, segments_t::noise);
    out.smooth.assign(n, std::uint8_t{0});
    if (n == 0) return out;
    device_array_t<std::uint32_t> d_labels(n, device);
    device_array_t<std::uint8_t> d_smooth(n, device);
    device_array_t<std::uint64_t> d_count(1, device);
    pcpx_index* const h = tree.index().handle();
    check(pcpx_segment_self_dev(h, d_normals.data(), params.curvature, radius, segment_min_cos(max_angle), params.max_curvature, params.min_size,
                                segment_flags(params), d_labels.data(), d_smooth.data(), d_count.data()),
          "pcpx_segment_self_dev");
    check(pcpx_index_synchronize(h), "pcpx_index_synchronize");
    out.labels        = d_labels.download();
    out.smooth        = d_smooth.download();
    out.segment_count = d_count.download()[0];
    return out;
}

} // namespace gpu
} // namespace pcp

#endif
