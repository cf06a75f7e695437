// pcp::gpu::euclidean_clusters / dbscan -- radius-connected components and DBSCAN of a container's own elements on the GPU
// (include/pcpx_cluster.h).  Not part of the reference API: the reference's density filter
// (examples/filter_point_cloud_noise_by_density.cpp) keeps a point iff its ball holds enough points, which is DBSCAN's core
// test; these calls also say which points belong together.  For any container with `.index().handle()` and `.size()`:
// pcp::basic_linked_octree_t and pcp::basic_linked_kdtree_t with K <= 3.
#ifndef PCP_GPU_CLUSTERING_HPP
#define PCP_GPU_CLUSTERING_HPP

#include "pcp/gpu/device_index.hpp"
#include "pcpx_cluster.h"

#include <cstdint>
#include <vector>

namespace pcp {
namespace gpu {

struct clusters_t
{
    static constexpr std::uint32_t noise = PCPX_CLUSTER_NOISE;
    std::vector<std::uint32_t> labels;  // one per element, in the container's element order: 0 ... cluster_count - 1, or noise
    std::vector<std::uint8_t> core;     // 1 = core point (its ball holds at least min_pts elements, itself included)
    std::uint64_t cluster_count = 0;
};

// DBSCAN: elements i, j are neighbours iff |p_i - p_j|^2 <= radius^2 (float32, the rule of range_search(sphere_t)); clusters are
// the connected components of the core elements, a non-core element with a core neighbour joins the cluster of smallest label
// among them, every other element is noise.  compact = false labels a cluster with its smallest core element index instead.
template <class Tree>
clusters_t dbscan(Tree const& tree, float radius, std::uint32_t min_pts, bool compact = true)
{
    clusters_t out;
    std::size_t const n = tree.size();
    out.labels.assign(n, clusters_t::noise);
    out.core.assign(n, std::uint8_t{0});
    if (n == 0) return out;
    check(pcpx_cluster_self(tree.index().handle(), radius, min_pts, compact ? PCPX_CLUSTER_COMPACT : 0u, out.labels.data(), out.core.data(),
                            nullptr, &out.cluster_count),
          "pcpx_cluster_self");
    return out;
}

// Euclidean cluster extraction: the connected components of "within radius of each other" (DBSCAN with min_pts = 1: no noise)
template <class Tree>
clusters_t euclidean_clusters(Tree const& tree, float radius, bool compact = true)
{
    return dbscan(tree, radius, 1u, compact);
}

} // namespace gpu
} // namespace pcp

#endif
