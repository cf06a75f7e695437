/*
 * pcpx_icp.h -- iterative closest point on a pcpx_index: the exact nearest indexed point of every source point under a pose, and
 * the ICP loop built on it (point to point by Horn's closed form, point to plane by a linearised step), every step defined to the
 * bit and the whole loop enqueued on the device without a host round trip.
 *
 * A companion of pcpx.h with its conventions: POD arguments, pcpx_status codes, pcpx_last_error().  The handle holds the TARGET
 * cloud; a rank-local handle (PCPX_BUILD_SHARD) is refused with PCPX_ERR_UNSUPPORTED.  The _dev forms take device arrays, are
 * enqueued on the handle's stream, never synchronise and read nothing back.
 *
 * INPUTS.  `s`: m x 3 float32, row-major and dense, the SOURCE.  `pose`: 16 doubles, a row-major 4 x 4 matrix T = [R t; 0 0 0 1]
 * that takes source points to target points (only its first three rows are read); in the _dev forms a DEVICE pointer, so the refit
 * array of pcpx_ransac_rigid_dev goes straight in.  NULL stands for the identity matrix, and is evaluated as that matrix.
 * `radius`: finite and >= 0.
 *
 * NEAREST PARTNER UNDER A POSE.
 *   moved point   float64, every operation rounded on its own (no FMA), in this order, then rounded to float32:
 *                     y_r = ((T[r][0]*s_0 + T[r][1]*s_1) + T[r][2]*s_2) + T[r][3]
 *   distance      to indexed point j as in pcpx.h: d = x_j - y per axis in float32, d2 = (dx*dx + dy*dy) + dz*dz, no FMA
 *   bound         r2 = radius * radius, one float32 product
 *   partner       of source row i: the indexed j with the smallest (d2, j) among those with d2 <= r2 -- ties in d2 go to the LOWEST
 *                 INPUT INDEX, so the answer does not depend on the tree or on the order the source is worked through in
 *   no partner    partner = PCPX_ICP_NONE (0xFFFFFFFF) and d2 = +inf: a row with nothing within the radius; a row whose s or y is
 *                 not finite (every comparison with a NaN is false; an infinite y is at an infinite or NaN distance of everything).
 *                 Points outside the voxel grid are not indexed and are never partners.
 * Outputs by source row: partner (m uint32, required), d2 (m float32, optional).  An empty source or an empty index is fine.
 * CONSISTENCY.  Where a partner exists, it and its d2 are row 0 of pcpx_knn_batch (k = 1, eps = 0) on the same float32 y.
 *
 * THE LOOP, POINT TO POINT (flags = 0).  T_0 = the initial pose; for k = 0, 1, ...:
 *   1. partner_k = the nearest partners under T_k, as above.
 *   2. count_k = the number of rows with a partner.
 *   3. If k > 0 and partner_k equals partner_(k-1) in every row: stop, status PCPX_ICP_CONVERGED; the result is T_k.  This is an
 *      exact fixed point: the fit depends on the pairs alone, so T_(k+1) would equal T_k in every bit.
 *   4. Else if count_k < 3: stop, status PCPX_ICP_STARVED; the result is T_k.
 *   5. Else T_(k+1) = the least-squares rigid fit of pcpx_register.h (pcpx_rigid_fit) over the m correspondences {i, partner_k[i]},
 *      i ascending, with p = the source and q = the handle's cloud by input row; a row without a partner has the target 0xFFFFFFFF,
 *      which is no row of q, so it is not usable by that header's rules.  The fit maps the ORIGINAL source: nothing is composed, no
 *      drift accumulates.  rms_k = the root mean square that fit returns.  The same kernels run, so the bits are pcpx_rigid_fit's.
 *   6. If k + 1 = max_iterations: stop, status PCPX_ICP_EXHAUSTED; the result is T_(k+1).
 * So the fused loop equals, bit for bit, the composition of pcpx_nearest_posed and pcpx_rigid_fit.
 *
 * OUTPUTS OF THE LOOP.  transform: 16 doubles, required (a result that is the initial pose carries its bits; the identity for NULL).
 * status; iterations = the number of pose updates made (steps 5 carried out); last_count = count_k of the last step 2: one uint32
 * each, optional.  Traces, optional: count[max_iterations] (uint32) and rms[max_iterations] (double) hold count_k and rms_k of the
 * steps k < iterations, and 0 and NaN from there on.  partner: m uint32, optional, the last list computed in step 1.
 *
 * POINT TO PLANE (PCPX_ICP_POINT_TO_PLANE).  `normals`: n_in x 3 float32 by input row of the target, required with the flag and
 * refused without it.  Steps 1-4 and 6 as above with "< 6" in step 4.  Step 5, all float64:
 *   o = the centre of the index's bounding box, (min + max) / 2 per axis from the float32 values of pcpx_index_bbox, widened.
 *   For every row i with a partner j whose normal n = normals[j] is finite, rows ascending:
 *       y = T_k s (as above but NOT rounded to float32),  x = the partner's point,  rho = ((y-x)_0 n_0 + (y-x)_1 n_1) + (y-x)_2 n_2,
 *       c = (y - o) x n  (c_0 = u_1 n_2 - u_2 n_1, c_1 = u_2 n_0 - u_0 n_2, c_2 = u_0 n_1 - u_1 n_0 with u = y - o),  J = [c, n]
 *   A = sum J J^T (the 21 entries of its upper triangle), b = - sum rho J, sum rho^2 and the number of such rows, formed in the fit's
 *   fixed order (per-thread strides over a fixed grid, a fixed tree within a block, the blocks in block order; no floating-point
 *   atomics), so two calls return the same bits.
 *   A x = b by Cholesky without pivoting; a pivot that is not finite, or <= 2^-40 times its own original diagonal entry, stops the
 *   loop with status PCPX_ICP_DEGENERATE, the result is T_k.
 *   x = (w, tau); dR = the rotation matrix of the unit quaternion (1, w/2) / |(1, w/2)| (square root and division only: always a
 *   proper rotation -- a Cayley step, equal to the exponential to second order, with the same fixed point);
 *   T_(k+1) = [dR R_k, dR (t_k - o) + o + tau];  rms_k = sqrt(sum rho^2 / rows).
 * Here "partners unchanged" is a stopping rule, not a proof that the pose is a fixed point: the step depends on T_k as well.
 *
 * COST.  The _dev form enqueues all max_iterations rounds; the rounds after the loop has stopped find a word set and return at
 * once (a few microseconds of empty kernels each).  The source is curve-sorted once per call, under the initial pose.
 *
 * PCPX_ERR_INVALID, from the arguments alone and before the handle or any device is touched: radius negative, NaN or infinite;
 * m >= 2^32 - 1; a NULL s with m > 0; a NULL partner (pcpx_nearest_posed) or transform (pcpx_icp_rigid); max_iterations outside
 * 1 .. 1024; an unknown flag bit; PCPX_ICP_POINT_TO_PLANE without normals, or normals without it.
 */
#ifndef PCPX_ICP_H
#define PCPX_ICP_H

#include "pcpx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCPX_ICP_NONE 0xFFFFFFFFu
#define PCPX_ICP_POINT_TO_PLANE 1u
#define PCPX_ICP_MAX_ITERATIONS 1024u
/* status words */
#define PCPX_ICP_EXHAUSTED 0u
#define PCPX_ICP_CONVERGED 1u
#define PCPX_ICP_STARVED 2u
#define PCPX_ICP_DEGENERATE 3u

/* Device arrays: d_s (m x 3 float32), d_opt_pose (16 doubles or NULL), d_out_partner (m uint32), d_opt_out_d2 (m float32). */
int pcpx_nearest_posed_dev(pcpx_index* index, const float* d_s, uint64_t m, const double* d_opt_pose, float radius, uint32_t* d_out_partner,
                           float* d_opt_out_d2);
/* the same with host arrays; waits for the result */
int pcpx_nearest_posed(pcpx_index* index, const float* s, uint64_t m, const double* opt_pose, float radius, uint32_t* out_partner,
                       float* opt_out_d2);

/* Device arrays as above; d_opt_normals: n_in x 3 float32; d_out_transform: 16 doubles; d_opt_out_status, d_opt_out_iterations,
 * d_opt_out_last_count: one uint32_t each; d_opt_out_count_trace: max_iterations uint32_t; d_opt_out_rms_trace: max_iterations
 * doubles; d_opt_out_partner: m uint32_t.  The scratch is leased from the device's pool until the stream has passed the call. */
int pcpx_icp_rigid_dev(pcpx_index* index, const float* d_s, uint64_t m, const double* d_opt_pose, float radius, uint32_t max_iterations,
                       uint32_t flags, const float* d_opt_normals, double* d_out_transform, uint32_t* d_opt_out_status,
                       uint32_t* d_opt_out_iterations, uint32_t* d_opt_out_last_count, uint32_t* d_opt_out_count_trace,
                       double* d_opt_out_rms_trace, uint32_t* d_opt_out_partner);
/* the same with host arrays; waits for the result */
int pcpx_icp_rigid(pcpx_index* index, const float* s, uint64_t m, const double* opt_pose, float radius, uint32_t max_iterations, uint32_t flags,
                   const float* opt_normals, double* out_transform, uint32_t* opt_out_status, uint32_t* opt_out_iterations,
                   uint32_t* opt_out_last_count, uint32_t* opt_out_count_trace, double* opt_out_rms_trace, uint32_t* opt_out_partner);

#ifdef __cplusplus
}
#endif
#endif /* PCPX_ICP_H */
