// pcp::gpu::shape_features -- the local shape descriptor of every element of a container on the GPU, over its fixed-radius
// neighbourhood: the three eigenvalues of the scatter matrix, the surface variation l0 / (l0 + l1 + l2) (Pauly et al. 2002; the
// "curvature" that pcp::gpu::smooth_segments gates on), the PCA normal and the principal axis, in one walk of the index
// (include/pcpx_features.h).  Not part of the reference API: the reference's normal estimation solves the
// same eigenproblem and keeps the normal only.  For any container with `.index()` and `.size()`: pcp::basic_linked_octree_t and
// pcp::basic_linked_kdtree_t with K <= 3.
#ifndef PCP_GPU_SHAPE_FEATURES_HPP
#define PCP_GPU_SHAPE_FEATURES_HPP

#include "pcp/gpu/device_index.hpp"
#include "pcpx_features.h"

#include <cstdint>
#include <vector>

namespace pcp {
namespace gpu {

// one row per element, in the container's element order; an empty neighbourhood (an element outside the voxel grid) has
// eigenvalues 0, curvature NaN, normal and axis (0, 0, 1), count 0
struct shape_features_t
{
    std::vector<float> evals;          // x 3, ascending: eigenvalues of the centred scatter matrix (not divided by the count)
    std::vector<float> curvature;      // surface variation max(l0, 0) / (l0 + l1 + l2), in [0, 1/3]
    std::vector<float> normals;        // x 3: the smallest eigenvalue's eigenvector, as estimate_normals with a range_search map
    std::vector<float> axes;           // x 3: the largest eigenvalue's eigenvector
    std::vector<std::uint32_t> count;  // elements in the sphere, the element itself included
};

// the same on the index's device: nothing crosses PCIe (d_normals and curvature.data() go to smooth_segments as they are)
struct device_shape_features_t
{
    device_array_t<float> evals, curvature, normals, axes;
    device_array_t<std::uint32_t> count;
};

template <class Tree>
shape_features_t shape_features(Tree const& tree, float radius)
{
    shape_features_t out;
    std::size_t const n = tree.size();
    out.evals.assign(3 * n, 0.f);
    out.curvature.assign(n, 0.f);
    out.normals.assign(3 * n, 0.f);
    out.axes.assign(3 * n, 0.f);
    out.count.assign(n, 0u);
    tree.index().shape_features_self(radius, n, out.evals.data(), out.curvature.data(), out.normals.data(), out.axes.data(), out.count.data());
    return out;
}

template <class Tree>
device_shape_features_t shape_features_device(Tree const& tree, float radius, int device = 0)
{
    device_shape_features_t out;
    std::size_t const n = tree.size();
    if (n == 0) return out;
    out.evals     = device_array_t<float>(3 * n, device);
    out.curvature = device_array_t<float>(n, device);
    out.normals   = device_array_t<float>(3 * n, device);
    out.axes      = device_array_t<float>(3 * n, device);
    out.count     = device_array_t<std::uint32_t>(n, device);
    tree.index().shape_features_self_dev(radius, out.evals.data(), out.curvature.data(), out.normals.data(), out.axes.data(), out.count.data());
    check(pcpx_index_synchronize(tree.index().handle()), "pcpx_index_synchronize");
    return out;
}

// the surface variation alone
template <class Tree>
std::vector<float> surface_variation(Tree const& tree, float radius)
{
    std::vector<float> curvature(tree.size(), 0.f);
    tree.index().shape_features_self(radius, tree.size(), nullptr, curvature.data(), nullptr, nullptr, nullptr);
    return curvature;
}

} // namespace gpu
} // namespace pcp

#endif
