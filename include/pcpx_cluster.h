/*
 * pcpx_cluster.h -- clustering of libpcpx.so: radius-connected components ("Euclidean cluster extraction") and DBSCAN of the
 * indexed cloud, in one walk of the index per pass and without materialising the neighbour lists.
 *
 * A companion of pcpx.h with its conventions: POD arguments, pcpx_status codes, pcpx_last_error(); a rank-local (shard) handle
 * is refused with PCPX_ERR_UNSUPPORTED.
 *
 * The contract is exact and does not depend on the tree, the voxel grid, the launch order or the run:
 *   - edge: i ~ j iff j is in i's sphere by the rule of pcpx_range_count_*: d2 <= r*r (d = p_j - p_i, float32, three roundings,
 *     no FMA); only points inside the index's voxel grid are in any sphere.  The rule is symmetric.
 *   - core: count_i >= min_pts, count_i = what pcpx_range_count_self gives (the point itself included).  min_pts = 1 makes every
 *     indexed point core: plain radius-connected components.  A point outside the voxel grid has count 0 and is noise.
 *   - cluster: a connected component of the core points under ~.
 *   - border: a non-core point with a core point in its sphere joins the cluster of smallest label among those core points.
 *   - noise: every other point; its label is PCPX_CLUSTER_NOISE.
 *   - labels: the smallest input index among the cluster's core points ("representative"), or with PCPX_CLUSTER_COMPACT the
 *     numbers 0 ... C-1 in the order of the representatives.
 * radius < 0 or NaN, min_pts == 0, unknown flag bits or a NULL label array are PCPX_ERR_INVALID.  radius 0 joins exact
 * duplicates only.  An empty cloud is fine (zero clusters).
 */
#ifndef PCPX_CLUSTER_H
#define PCPX_CLUSTER_H

#include "pcpx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCPX_CLUSTER_NOISE 0xFFFFFFFFu
/* flags */
#define PCPX_CLUSTER_COMPACT 1u /* labels 0 ... C-1 ordered by representative instead of the representatives themselves */

/* Device arrays by input row (n_in rows): d_labels (required); d_opt_core: 1 = core point; d_opt_count: the sphere counts, equal
 * to pcpx_range_count_self_dev's output; d_opt_cluster_count: one uint64_t, the number of clusters.  Enqueued on the handle's
 * stream (pcpx_index_synchronize waits for it); scratch is the handle's (8 bytes per point). */
int pcpx_cluster_self_dev(pcpx_index* idx, float radius, uint32_t min_pts, uint32_t flags, uint32_t* d_labels,
                          uint8_t* d_opt_core, uint32_t* d_opt_count, uint64_t* d_opt_cluster_count);
/* host arrays, one row per input point; *opt_cluster_count: the number of clusters */
int pcpx_cluster_self(pcpx_index* idx, float radius, uint32_t min_pts, uint32_t flags, uint32_t* labels, uint8_t* opt_core,
                      uint32_t* opt_count, uint64_t* opt_cluster_count);

#ifdef __cplusplus
}
#endif
#endif /* PCPX_CLUSTER_H */
