// pcp::gpu::mls_project -- moving least squares projection of every element of a container on the GPU (Levin; Alexa et al. 2003;
// PCL's MovingLeastSquares): each element is projected onto a Gaussian-weighted plane (order 1) or a quadric over it (order 2) of
// its fixed-radius neighbourhood, with the surface normal and the mean and Gaussian curvature at the projection
// (include/pcpx_mls.h).  Not part of the reference API: its denoisers (bilateral filter, WLOP) fit no surface.
// For any container with `.index()` and `.size()`: pcp::basic_linked_octree_t and pcp::basic_linked_kdtree_t with K <= 3.
#ifndef PCP_GPU_MLS_HPP
#define PCP_GPU_MLS_HPP

#include "pcp/gpu/device_index.hpp"
#include "pcpx_mls.h"

#include <cstdint>
#include <vector>

namespace pcp {
namespace gpu {

// one row per element, in the container's element order; an element with fewer than 3 points in its sphere (an element outside
// the voxel grid among them) keeps its coordinates: displacement 0, normal (0, 0, 1), fit 0
struct mls_t
{
    std::vector<float> points;         // x 3: element + displacement
    std::vector<float> displacements;  // x 3
    std::vector<float> normals;        // x 3, unit length
    std::vector<float> curvatures;     // x 2: mean and Gaussian curvature; NaN unless fit = 2
    std::vector<std::uint32_t> count;  // elements in the sphere, the element itself included
    std::vector<std::uint32_t> fit;    // 0 unchanged, 1 plane, 2 quadric
};

// the same on the index's device: nothing crosses PCIe (points.data() is a cloud for pcpx_index_create_dev, normals.data() goes to
// smooth_segments as it is)
struct device_mls_t
{
    device_array_t<float> points, displacements, normals, curvatures;
    device_array_t<std::uint32_t> count, fit;
};

// h: the Gaussian's width, weight exp(-d^2 / h^2); radius / 2 leaves e^-4 at the sphere's rim
template <class Tree>
mls_t mls_project(Tree const& tree, float radius, float h, int order = 2)
{
    mls_t out;
    std::size_t const n = tree.size();
    out.points.assign(3 * n, 0.f);
    out.displacements.assign(3 * n, 0.f);
    out.normals.assign(3 * n, 0.f);
    out.curvatures.assign(2 * n, 0.f);
    out.count.assign(n, 0u);
    out.fit.assign(n, 0u);
    if (n)
        check(pcpx_mls_project_self(tree.index().handle(), radius, h, order, out.points.data(), out.displacements.data(), out.normals.data(),
                                    out.curvatures.data(), out.count.data(), out.fit.data()),
              "pcpx_mls_project_self");
    return out;
}

template <class Tree>
device_mls_t mls_project_device(Tree const& tree, float radius, float h, int order = 2, int device = 0)
{
    device_mls_t out;
    std::size_t const n = tree.size();
    if (n == 0) return out;
    out.points        = device_array_t<float>(3 * n, device);
    out.displacements = device_array_t<float>(3 * n, device);
    out.normals       = device_array_t<float>(3 * n, device);
    out.curvatures    = device_array_t<float>(2 * n, device);
    out.count         = device_array_t<std::uint32_t>(n, device);
    out.fit           = device_array_t<std::uint32_t>(n, device);
    check(pcpx_mls_project_self_dev(tree.index().handle(), radius, h, order, 0, UINT64_MAX, out.points.data(), out.displacements.data(),
                                    out.normals.data(), out.curvatures.data(), out.count.data(), out.fit.data()),
          "pcpx_mls_project_self_dev");
    check(pcpx_index_synchronize(tree.index().handle()), "pcpx_index_synchronize");
    return out;
}

} // namespace gpu
} // namespace pcp

#endif
