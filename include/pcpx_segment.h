/*
 * pcpx_segment.h -- smooth-surface segmentation of libpcpx.so: normal-constrained region growing (Rabbani et al. 2006) of the
 * indexed cloud in its order-independent form, in one walk of the index per pass and without materialising the neighbour lists.
 *
 * A companion of pcpx.h with its conventions: POD arguments, pcpx_status codes, pcpx_last_error(); a rank-local (shard) handle
 * is refused with PCPX_ERR_UNSUPPORTED.
 *
 * The contract is exact and does not depend on the tree, the voxel grid, the launch order or the run:
 *   - near: i and j are near iff j is in i's sphere by the rule of pcpx_range_count_*: d2 <= r*r (d = p_j - p_i, float32, three
 *     roundings, no FMA); only points inside the index's voxel grid are in any sphere.
 *   - compatible: with t = (nx_i*nx_j + ny_i*ny_j) + nz_i*nz_j in float32 (every product and both sums rounded, no FMA), i and j
 *     are compatible iff |t| >= min_cos, or with PCPX_SEGMENT_ORIENTED iff t >= min_cos.  A NaN t fails.  The rule is symmetric.
 *     The normals are used as given and never normalised; the threshold is a cosine, so no cos() is part of the contract.
 *   - smooth: with curvature == NULL every indexed point; otherwise a point with curvature_i <= max_curvature (a NaN curvature is
 *     not smooth).  A point outside the voxel grid is never smooth.
 *   - segment: a connected component of the smooth points under "near and compatible".  Growth is transitive: two points of one
 *     segment may have very different normals.
 *   - border: a non-smooth indexed point takes the smallest label among the smooth points that are in its sphere and compatible
 *     with it; if there is none it is noise.
 *   - size filter: after border assignment a segment's size is the number of rows that carry its label; every row of a segment
 *     of size < min_size becomes PCPX_SEGMENT_NOISE and is not reassigned.  min_size <= 1 filters nothing.
 *   - labels: the smallest input index among the segment's smooth points ("representative"), or with PCPX_SEGMENT_COMPACT the
 *     numbers 0 ... S-1 in the order of those representatives over the surviving segments.  The segment count is S.
 * radius < 0 or NaN, a NaN min_cos, a NaN max_curvature beside a curvature array, NULL normals or labels, or unknown flag bits
 * are PCPX_ERR_INVALID.  radius 0 joins exact duplicates with compatible normals.  An empty cloud is fine (zero segments).
 * min_cos <= -1 with unit normals and no curvature array gives pcpx_cluster_self(min_pts = 1)'s labels.
 */
#ifndef PCPX_SEGMENT_H
#define PCPX_SEGMENT_H

#include "pcpx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCPX_SEGMENT_NOISE 0xFFFFFFFFu
/* flags */
#define PCPX_SEGMENT_COMPACT 1u  /* labels 0 ... S-1 ordered by representative instead of the representatives themselves */
#define PCPX_SEGMENT_ORIENTED 2u /* compatible iff t >= min_cos (the normals' signs matter) instead of |t| >= min_cos */

/* Device arrays by input row (n_in rows): d_normals (n_in x 3 float32, required), d_opt_curvature (n_in float32), d_labels
 * (required), d_opt_smooth: 1 = smooth point; d_opt_segment_count: one uint64_t, the number of segments.  Enqueued on the handle's
 * stream (pcpx_index_synchronize waits for it); scratch is the handle's (8 bytes per point and 96 bytes per leaf of 8). */
int pcpx_segment_self_dev(pcpx_index* idx, const float* d_normals, const float* d_opt_curvature, float radius, float min_cos,
                          float max_curvature, uint32_t min_size, uint32_t flags, uint32_t* d_labels, uint8_t* d_opt_smooth,
                          uint64_t* d_opt_segment_count);
/* host arrays, one row per input point; *opt_segment_count: the number of segments */
int pcpx_segment_self(pcpx_index* idx, const float* normals, const float* opt_curvature, float radius, float min_cos,
                      float max_curvature, uint32_t min_size, uint32_t flags, uint32_t* labels, uint8_t* opt_smooth,
                      uint64_t* opt_segment_count);

#ifdef __cplusplus
}
#endif
#endif /* PCPX_SEGMENT_H */
