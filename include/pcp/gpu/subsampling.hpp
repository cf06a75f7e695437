// pcp::gpu::poisson_disk_subsample -- the subsample of a container's own elements in which no two elements are within `radius` of
// each other and every dropped element has a kept one within `radius`, on the GPU (include/pcpx_subsample.h).
// Not part of the reference API: the reference's examples/downsample.cpp offers a random shuffle and hierarchy simplification,
// neither of which promises a spacing.  For any container with `.index().handle()` and `.size()`: pcp::basic_linked_octree_t and
// pcp::basic_linked_kdtree_t with K <= 3.
#ifndef PCP_GPU_SUBSAMPLING_HPP
#define PCP_GPU_SUBSAMPLING_HPP

#include "pcp/gpu/device_index.hpp"
#include "pcpx_subsample.h"

#include <cstdint>
#include <vector>

namespace pcp {
namespace gpu {

struct subsample_t
{
    static constexpr std::uint32_t none = PCPX_SUBSAMPLE_NONE;
    std::vector<std::uint32_t> kept;   // the kept elements, ascending, in the container's element order
    std::vector<std::uint32_t> owner;  // one per element: itself if kept, else the nearest kept element (ties: the smaller index); none
                                       // for an element the container did not insert
    std::uint32_t rounds = 0;          // round launches the call issued
};

// Elements i, j are neighbours iff |p_i - p_j|^2 <= radius^2 (float32, the rule of range_search(sphere_t)).  The kept set is what
// the greedy loop gives that visits the elements in ascending fmix32(index ^ seed) and keeps one iff no kept element is its
// neighbour: exact and the same on every run; another seed gives another sample.  radius 0 removes exact duplicates.
template <class Tree>
subsample_t poisson_disk_subsample(Tree const& tree, float radius, std::uint32_t seed = 0u)
{
    subsample_t out;
    std::size_t const n = tree.size();
    if (n == 0) return out;
    std::vector<std::uint8_t> keep(n);
    out.owner.assign(n, subsample_t::none);
    out.kept.resize(n);
    std::uint64_t count = 0;
    check(pcpx_subsample_self(tree.index().handle(), radius, seed, 0u, keep.data(), out.owner.data(), out.kept.data(), &count, &out.rounds),
          "pcpx_subsample_self");
    out.kept.resize(static_cast<std::size_t>(count));
    return out;
}

} // namespace gpu
} // namespace pcp

#endif
