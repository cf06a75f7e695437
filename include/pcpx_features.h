/*
 * pcpx_features.h -- local shape features of libpcpx.so: the three eigenvalues of every fixed-radius neighbourhood's scatter
 * matrix, its surface variation (Pauly et al. 2002: what PCL calls "curvature" and what region growing gates on), its PCA normal
 * and its principal axis, in one walk of the index and without materialising the neighbour lists.
 *
 * A companion of pcpx.h with its conventions: POD arguments, pcpx_status codes, pcpx_last_error(); a rank-local (shard) handle
 * is refused with PCPX_ERR_UNSUPPORTED.  The neighbourhood and the moments are those of pcpx_radius.h:
 *   - a sphere holds every indexed point with d2 <= r*r (d = p - centre, float32, no FMA), its own centre included;
 *   - a point outside the index's voxel grid is in no sphere, and its own (self) row is an empty neighbourhood;
 *   - radius < 0 or NaN is PCPX_ERR_INVALID; radius 0 holds the point itself and its exact duplicates;
 *   - one pass of float32 moments about the sphere's centre: n, S = sum d, Q = sum d d^T, C = Q - S (S / n).
 * Outputs per row, all from one solve of C by the solver of pcp::estimate_normal:
 *   evals      3 floats, ascending: the eigenvalues of the centred scatter matrix C, NOT divided by n -- the convention of
 *              pcpx_normals_from_knn's opt_out_evals.  Raw: rounding may leave the smallest slightly negative.
 *   curvature  the surface variation max(l0, 0) / ((l0 + l1) + l2) in float32, in that order; 0 when the sum is <= 0 (one
 *              point, copies of one point).  In [0, 1/3].
 *   normal     3 floats: bit for bit what pcpx_range_neighbourhoods_* writes for the same sphere.
 *   axis       3 floats: the eigenvector column of the largest eigenvalue after the solver's ascending sort.  Unit length, sign
 *              arbitrary.
 *   count      the number of points in the sphere.
 * An empty neighbourhood gets evals (0, 0, 0), curvature NaN, normal (0, 0, 1), axis (0, 0, 1) (the solver on a zero matrix:
 * the identity's third column, for the normal by its "last tie wins" selection) and count 0.  A NaN curvature fails
 * pcpx_segment_*'s gate curvature <= max_curvature, so an empty neighbourhood is "not smooth" there, like a point outside the
 * grid.  Any output may be NULL, not all.
 */
#ifndef PCPX_FEATURES_H
#define PCPX_FEATURES_H

#include "pcpx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* d_opt_*: device arrays by input row; sorted-slice arguments as pcpx_knn_self_dev: exactly the rows of the slice's points are
 * written, every other row is left untouched -- except that a slice that covers the whole curve order (sorted_first 0,
 * sorted_count >= the index size) also writes the empty-neighbourhood values at the rows of points outside the voxel grid.
 * Enqueued on the handle's stream (pcpx_index_synchronize waits for it). */
int pcpx_shape_features_self_dev(pcpx_index* idx, float radius, uint64_t sorted_first, uint64_t sorted_count, float* d_opt_evals,
                                 float* d_opt_curvature, float* d_opt_normals, float* d_opt_axes, uint32_t* d_opt_count);
/* host arrays, one row per input point (n_in rows) */
int pcpx_shape_features_self(pcpx_index* idx, float radius, float* opt_evals, float* opt_curvature, float* opt_normals,
                             float* opt_axes, uint32_t* opt_count);
/* nq external spheres (host arrays, q_xyz nq x 3); radii NULL -> `radius` for all, else one radius per sphere (each >= 0) */
int pcpx_shape_features_batch(pcpx_index* idx, const float* q_xyz, const float* radii, float radius, uint64_t nq, float* opt_evals,
                              float* opt_curvature, float* opt_normals, float* opt_axes, uint32_t* opt_count);

#ifdef __cplusplus
}
#endif
#endif /* PCPX_FEATURES_H */
