// pcp::gpu::fpfh -- the Fast Point Feature Histograms (Rusu, Blodow, Beetz 2009) of a container's own elements, or of some of them,
// on the GPU (include/pcpx_descriptors.h).  Not part of the reference API: the reference estimates normals
// and has nothing that describes a point by them.  For any container with `.index().handle()` and `.size()`:
// pcp::basic_linked_octree_t and pcp::basic_linked_kdtree_t with K <= 3.
#ifndef PCP_GPU_DESCRIPTORS_HPP
#define PCP_GPU_DESCRIPTORS_HPP

#include "pcp/gpu/device_index.hpp"
#include "pcpx_descriptors.h"

#include <array>
#include <cstdint>
#include <vector>

namespace pcp {
namespace gpu {

using fpfh_t = std::array<float, PCPX_FPFH_SIZE>;  // three blocks of PCPX_FPFH_BINS bins, each summing to 100 (or all 0)

// One descriptor per entry of `rows` (distinct element indices of the container's element order), or per element when `rows` is
// null: the 1 / d^2-weighted sum, over the elements within `radius` (float32, the rule of range_search(sphere_t)), of their
// simplified histograms of the pair features.  normal_map(i) gives the normal of element i (anything with x(), y(), z());
// normals are used as given, so orient them first.  An element outside the voxel grid gets zeros.
template <class Tree, class NormalMap>
std::vector<fpfh_t> fpfh(Tree const& tree, NormalMap const& normal_map, float radius, std::vector<std::uint32_t> const* rows = nullptr)
{
    std::size_t const n = tree.size();
    std::vector<fpfh_t> out(rows ? rows->size() : n);
    if (n == 0 || out.empty()) return out;
    std::vector<float> normals(3 * n);
    for (std::size_t i = 0; i < n; ++i)
    {
        auto const nrm     = normal_map(i);
        normals[3 * i]     = static_cast<float>(nrm.x());
        normals[3 * i + 1] = static_cast<float>(nrm.y());
        normals[3 * i + 2] = static_cast<float>(nrm.z());
    }
    check(pcpx_fpfh_self(tree.index().handle(), normals.data(), radius, rows ? rows->data() : nullptr, rows ? rows->size() : 0u, 0u,
                         out.front().data(), nullptr, nullptr),
          "pcpx_fpfh_self");
    return out;
}

// The same with the normals (n x 3 float32, element order) and the rows (m of them, or none: every element) already on the index's
// device -- what shape_features and iss_keypoints leave there: nothing but the descriptors crosses PCIe.
template <class Tree>
std::vector<fpfh_t> fpfh(Tree const& tree, device_array_t<float> const& d_normals, float radius, std::uint32_t const* d_rows = nullptr,
                         std::size_t m = 0, int device = 0)
{
    std::size_t const n = tree.size();
    std::vector<fpfh_t> out(d_rows ? m : n);
    if (n == 0 || out.empty()) return out;
    device_array_t<float> d_out(out.size() * PCPX_FPFH_SIZE, device);
    pcpx_index* const h = tree.index().handle();
    check(pcpx_fpfh_self_dev(h, d_normals.data(), radius, d_rows, d_rows ? m : 0u, 0u, d_out.data(), nullptr, nullptr), "pcpx_fpfh_self_dev");
    check(pcpx_index_synchronize(h), "pcpx_index_synchronize");
    std::vector<float> const flat = d_out.download();
    for (std::size_t i = 0; i < out.size(); ++i)
        for (std::size_t b = 0; b < PCPX_FPFH_SIZE; ++b) out[i][b] = flat[i * PCPX_FPFH_SIZE + b];
    return out;
}

} // namespace gpu
} // namespace pcp

#endif
