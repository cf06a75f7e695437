// pcp::gpu::farthest_point_sample -- m elements of a container that cover it as evenly as a greedy choice can: each sample is the
// element farthest from the samples before it, on the GPU (include/pcpx_fps.h; Open3D's
// farthest_point_down_sample, the sampling layer of PointNet++).  Not part of the reference API, whose samplers choose by density
// or by grid and take no count.  For any container with `.index().handle()` and `.size()`: pcp::basic_linked_octree_t and
// pcp::basic_linked_kdtree_t with K <= 3.
#ifndef PCP_GPU_FARTHEST_POINTS_HPP
#define PCP_GPU_FARTHEST_POINTS_HPP

#include "pcp/gpu/device_index.hpp"
#include "pcpx_fps.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace pcp {
namespace gpu {

struct fps_params_t
{
    std::uint32_t start = PCPX_FPS_START_LOWEST;  // the first sample: an element, or the lowest element the index holds
    float stop_radius   = 0.f;                    // the selection ends when no element is farther than this from the samples
    bool want_d2 = false, want_min_d2 = false, want_owner = false, want_evaluations = false;
};

struct fps_t
{
    std::vector<std::uint32_t> samples;  // in selection order, in the container's element order
    std::vector<float> d2;               // on request: each sample's squared distance to the samples before it; the first +inf
    std::vector<float> min_d2;           // on request, per element: the squared distance to its nearest sample
    std::vector<std::uint32_t> owner;    // on request, per element: the ordinal of the earliest nearest sample; PCPX_FPS_NONE: none
    std::uint64_t evaluations = 0;       // on request: squared distances formed (a diagnostic)
};

// the same on the index's device: nothing crosses PCIe (samples.data() and count.data() are what pcpx_farthest_points_self wrote)
struct device_fps_t
{
    device_array_t<std::uint32_t> samples;  // room for m entries; the first *count are written
    device_array_t<std::uint64_t> count;    // one word
    device_array_t<float> d2;
    device_array_t<float> min_d2;
    device_array_t<std::uint32_t> owner;
    device_array_t<std::uint64_t> evaluations;
};

template <class Tree>
fps_t farthest_point_sample(Tree const& tree, std::size_t m, fps_params_t const& params = {})
{
    fps_t out;
    std::size_t const n = tree.size();
    std::size_t const most = std::min(m, n);  // the library writes [0, count), count <= min(m, n)
    out.samples.resize(std::max<std::size_t>(most, 1));
    if (params.want_d2) out.d2.resize(std::max<std::size_t>(most, 1));
    if (params.want_min_d2) out.min_d2.resize(n);
    if (params.want_owner) out.owner.resize(n);
    pcpx_fps_params const p{0u, params.start, params.stop_radius, 0u};
    std::uint64_t count = 0;
    check(pcpx_farthest_points_self(tree.index().handle(), m, &p, out.samples.data(), &count, params.want_d2 ? out.d2.data() : nullptr,
                                    params.want_min_d2 && n ? out.min_d2.data() : nullptr, params.want_owner && n ? out.owner.data() : nullptr,
                                    params.want_evaluations ? &out.evaluations : nullptr),
          "pcpx_farthest_points_self");
    out.samples.resize(static_cast<std::size_t>(count));
    if (params.want_d2) out.d2.resize(static_cast<std::size_t>(count));
    return out;
}

// Device arrays: the overload that takes a device_fps_t leaves every output on the index's device, in arrays it allocates there.
// Enqueued on the index's stream and not waited for -- the stop rule is applied on the device, nothing is read back between
// samples: pcpx_index_synchronize, or work on the same stream, comes after it.
template <class Tree>
void farthest_point_sample(Tree const& tree, std::size_t m, device_fps_t& out, fps_params_t const& params = {}, int device = 0)
{
    std::size_t const n = tree.size();
    out         = device_fps_t{};
    out.samples = device_array_t<std::uint32_t>(std::max<std::size_t>(m, 1), device);
    out.count   = device_array_t<std::uint64_t>(1, device);
    if (params.want_d2) out.d2 = device_array_t<float>(std::max<std::size_t>(m, 1), device);
    if (params.want_min_d2 && n) out.min_d2 = device_array_t<float>(n, device);
    if (params.want_owner && n) out.owner = device_array_t<std::uint32_t>(n, device);
    if (params.want_evaluations) out.evaluations = device_array_t<std::uint64_t>(1, device);
    pcpx_fps_params const p{PCPX_FPS_ON_DEVICE, params.start, params.stop_radius, 0u};
    check(pcpx_farthest_points_self(tree.index().handle(), m, &p, out.samples.data(), out.count.data(), params.want_d2 ? out.d2.data() : nullptr,
                                    params.want_min_d2 && n ? out.min_d2.data() : nullptr, params.want_owner && n ? out.owner.data() : nullptr,
                                    params.want_evaluations ? out.evaluations.data() : nullptr),
          "pcpx_farthest_points_self");
}

} // namespace gpu
} // namespace pcp

#endif
