/*
 * pcpx_radius.h -- fixed-radius neighbourhoods of libpcpx.so: the PCA normal, the centroid, the mean distance and the count of
 * every point inside a sphere, in one walk of the index and without materialising the neighbour lists.
 *
 * What pcp::algorithm::estimate_normals, estimate_tangent_planes and average_distances_to_neighbors compute when their
 * neighbourhood map is `tree.range_search(sphere_t{p, r})` (reference: include/pcp/algorithm/estimate_normals.hpp:50-93,
 * estimate_tangent_planes.hpp, average_distance_to_neighbors.hpp).  A companion of pcpx.h with its conventions: POD
 * arguments, pcpx_status codes, pcpx_last_error(); a rank-local (shard) handle is refused with PCPX_ERR_UNSUPPORTED.
 *
 * Semantics (those of pcpx_range_count_*):
 *   - a sphere holds every indexed point with d2 <= r*r (d = p - centre, float32, no FMA), its own centre included;
 *   - a point outside the index's voxel grid is in no sphere, and its own (self) row is an empty neighbourhood;
 *   - radius < 0 or NaN is PCPX_ERR_INVALID; radius 0 holds the point itself and its exact duplicates.
 * Outputs per row: normal (3 floats) = eigenvector of the smallest eigenvalue of the neighbourhood's centred scatter matrix,
 * selected as pcp::estimate_normal does; centroid (3 floats) = the neighbourhood's mean; mean distance = mean of |d| over the
 * neighbourhood (the centre's own zero included); count.  An empty neighbourhood gets what the reference gives for an empty set:
 * normal (0, 0, 1) (the solver on a zero matrix), centroid NaN, mean distance NaN, count 0.  Any output may be NULL, not all.
 * The arithmetic is one pass of float32 moments about the sphere's centre.
 */
#ifndef PCPX_RADIUS_H
#define PCPX_RADIUS_H

#include "pcpx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* d_opt_*: device arrays by input row; sorted-slice arguments as pcpx_knn_self_dev: exactly the rows of the slice's points are
 * written, every other row is left untouched -- except that a slice that covers the whole curve order (sorted_first 0,
 * sorted_count >= the index size) also writes the empty-neighbourhood values at the rows of points outside the voxel grid.
 * Enqueued on the handle's stream (pcpx_index_synchronize waits for it). */
int pcpx_range_neighbourhoods_self_dev(pcpx_index* idx, float radius, uint64_t sorted_first, uint64_t sorted_count,
                                       float* d_opt_normals, float* d_opt_centroids, float* d_opt_mean_dist,
                                       uint32_t* d_opt_count);
/* host arrays, one row per input point (n_in rows) */
int pcpx_range_neighbourhoods_self(pcpx_index* idx, float radius, float* opt_normals, float* opt_centroids,
                                   float* opt_mean_dist, uint32_t* opt_count);
/* nq external spheres (host arrays, q_xyz nq x 3); radii NULL -> `radius` for all, as pcpx_range_sphere_batch, else one
 * radius per sphere (each >= 0) */
int pcpx_range_neighbourhoods_batch(pcpx_index* idx, const float* q_xyz, const float* radii, float radius, uint64_t nq,
                                    float* opt_normals, float* opt_centroids, float* opt_mean_dist, uint32_t* opt_count);

#ifdef __cplusplus
}
#endif
#endif /* PCPX_RADIUS_H */
