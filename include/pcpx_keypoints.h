/*
 * pcpx_keypoints.h -- keypoints of libpcpx.so: the local maxima of a per-point score over a radius (sphere-wise non-maximum
 * suppression) and, on top of the eigenvalues of pcpx_features.h, the ISS keypoint detector (Zhong 2009), in one walk of the index
 * per step and without materialising the neighbour lists.
 *
 * A companion of pcpx.h with its conventions: POD arguments, pcpx_status codes, pcpx_last_error(); a rank-local (shard) handle
 * is refused with PCPX_ERR_UNSUPPORTED.
 *
 * LOCAL MAXIMA.  `score`: one float32 per input row.  The contract is exact and does not depend on the tree, the voxel grid, the
 * launch order or the run:
 *   - sphere: j is in i's sphere iff d2 <= r*r by the rule of pcpx_range_count_* (d = p_j - p_i, float32, three roundings, no
 *     FMA); only points inside the index's voxel grid are in any sphere; the centre is in its own sphere.
 *   - candidate: an indexed point whose score is not NaN and is >= min_score.  min_score = -inf admits every non-NaN score.
 *   - beats: j beats i iff score_j > score_i, or score_j == score_i and j < i -- float comparisons, j and i input indices.  So -0
 *     equals +0, +-inf are ordinary values and a NaN score beats nobody; on non-NaN scores this is a strict total order.
 *   - kept: i is kept iff it is a candidate, no other indexed j in its sphere beats it, and its sphere holds at least
 *     min_neighbours points, itself included (0 and 1 are the same).
 * What follows:
 *   - no two kept points lie within r of each other (one of them would beat the other);
 *   - radius 0 keeps the best point of every set of exact duplicates;
 *   - a point outside the voxel grid is never kept and never suppresses;
 *   - a point below min_score is never kept, but -- its score being below every candidate's -- it could not suppress one anyway;
 *   - there is NO domination guarantee: a dropped point need not have a kept point within r (the point that beat it may itself be
 *     beaten).  That is what distinguishes this from pcpx_subsample_*, whose kept set also covers the cloud.
 * Minima: negate the score.
 *
 * ISS KEYPOINTS.  With evals (l0 <= l1 <= l2: the scatter matrix's, raw) and count of pcpx_shape_features_* at salient_radius:
 *   saliency_i = l0 / (float)count   if l1 < gamma21 * l2 and l0 < gamma32 * l1   (each product one float32 rounding, the quotient
 *                                    the correctly rounded float32 division: the covariance convention, so that densities compare)
 *              = NaN                 otherwise -- an empty neighbourhood or one with every eigenvalue 0 fails the strict tests --
 *                                    and for a point outside the voxel grid;
 *   the keypoints are the local maxima of saliency at non_max_radius with min_score = -inf and the given min_neighbours.
 *
 * radius < 0 or NaN (either radius of the ISS call), a NaN min_score, a NaN gamma, flags != 0, a NULL keep or a NULL score array
 * are PCPX_ERR_INVALID.  An empty cloud is fine (count 0).
 */
#ifndef PCPX_KEYPOINTS_H
#define PCPX_KEYPOINTS_H

#include "pcpx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Device arrays: d_score (n_in floats); d_keep (required; n_in rows, 1 = kept, every row written); d_opt_kept_rows (room for n_in
 * entries: the kept input indices, ascending); d_opt_kept_count (one uint64_t).  Fully enqueued on the handle's stream: nothing
 * here depends on the data, so there is no read-back and no synchronisation (pcpx_index_synchronize waits for it).  Scratch is the
 * handle's (4 bytes per leaf slot, and the scan's).  Under pcpx_profile_begin/end the call is booked as ONE interval of the
 * PCPX_K_RANGE family. */
int pcpx_local_maxima_self_dev(pcpx_index* idx, const float* d_score, float radius, float min_score, uint32_t min_neighbours,
                               uint32_t flags, uint8_t* d_keep, uint32_t* d_opt_kept_rows, uint64_t* d_opt_kept_count);
/* the same with host arrays; kept_rows[0 .. *opt_kept_count) are written */
int pcpx_local_maxima_self(pcpx_index* idx, const float* score, float radius, float min_score, uint32_t min_neighbours, uint32_t flags,
                           uint8_t* keep, uint32_t* opt_kept_rows, uint64_t* opt_kept_count);

/* The outputs of the call above and d_opt_saliency (n_in floats, every row written), with which a caller can threshold again
 * (pcpx_local_maxima_self_dev with a min_score) without the eigenvalues being computed again.  Enqueued as the call above; the
 * handle's scratch also holds the eigenvalues and counts (16 bytes per row) and, without d_opt_saliency, the saliency. */
int pcpx_iss_keypoints_self_dev(pcpx_index* idx, float salient_radius, float non_max_radius, float gamma21, float gamma32,
                                uint32_t min_neighbours, uint32_t flags, uint8_t* d_keep, uint32_t* d_opt_kept_rows,
                                uint64_t* d_opt_kept_count, float* d_opt_saliency);
int pcpx_iss_keypoints_self(pcpx_index* idx, float salient_radius, float non_max_radius, float gamma21, float gamma32,
                            uint32_t min_neighbours, uint32_t flags, uint8_t* keep, uint32_t* opt_kept_rows, uint64_t* opt_kept_count,
                            float* opt_saliency);

#ifdef __cplusplus
}
#endif
#endif /* PCPX_KEYPOINTS_H */
