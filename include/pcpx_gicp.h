/*
 * pcpx_gicp.h -- Generalized ICP on a pcpx_index (Segal, Haehnel, Thrun 2009): the loop of pcpx_icp.h with a plane-to-plane step.
 * Every point of both clouds carries a covariance that is flat along its surface; a pair's residual is weighted by the inverse of
 * C_t + R C_s R^T, so a pair may slide along both surfaces for free.  Every step is defined to the operation and the whole loop is
 * enqueued on the device without a host round trip.
 *
 * A companion of pcpx.h and pcpx_icp.h with their conventions: POD arguments, pcpx_status codes, pcpx_last_error().  The handle holds
 * the TARGET cloud; a rank-local handle (PCPX_BUILD_SHARD) and a handle that keeps no copy of its cloud are refused with
 * PCPX_ERR_UNSUPPORTED.  One entry point, as in pcpx_fps.h and pcpx_boundary.h: host arrays by default, and then the call waits for
 * its result; with PCPX_GICP_ON_DEVICE every array argument, the single words (status, iterations, last_count) included, is a device
 * pointer owing its element type's alignment and no more, and the call is enqueued on the handle's stream, never synchronises and
 * reads nothing back -- the refit array of pcpx_ransac_rigid_dev and the normals of pcpx_range_neighbourhoods_self_dev go straight
 * in.  The scratch is leased from the device's pool until the stream has passed the call.  The two forms return the same bits.
 * The status words, PCPX_ICP_NONE and PCPX_ICP_MAX_ITERATIONS are pcpx_icp.h's.
 *
 * INPUTS.  `s`, `pose`, `radius`, `max_iterations`: as pcpx_icp_rigid.
 *   without the next flag     source_cov: m x 3 float32, a NORMAL per source row; target_cov: n_in x 3 float32, a normal per input row
 *                             of the target.  They need be neither oriented nor of unit length.  epsilon: in (0, 1], the variance
 *                             along the normal relative to the variance across it.
 *   PCPX_GICP_COVARIANCES     source_cov: m x 6, target_cov: n_in x 6 float32, the upper triangle of a covariance per row in the
 *                             order xx, xy, xz, yy, yz, zz.  epsilon is not used and must be 0.
 *
 * THE LOOP.  T_0 = the initial pose; for k = 0, 1, ...: steps 1-4 and 6 are the point-to-point steps of pcpx_icp.h (the partner
 * search is pcpx_nearest_posed's, bit for bit; "< 3" in step 4).  Step 5, all float64, every operation rounded on its own (no FMA),
 * every sum from left to right as written:
 *   o = the centre of the index's bounding box, as in the point-to-plane step of pcpx_icp.h.  R = the rotation rows of T_k.
 *   The matrix C of a row
 *     from a normal n (float32, widened):  q = (n_0 n_0 + n_1 n_1) + n_2 n_2; there is no C unless q is finite and > 0;
 *                                          C_rc = d_rc - ((1 - eps) * (n_r n_c)) / q   for r <= c, with d_rc = 1 where r = c, else 0,
 *                                          and eps the float32 argument widened.  (-a)(-b) is ab exactly: the sign of n changes no bit.
 *     from six floats:                     widened as they are; there is no C unless all six are finite.
 *   A source row i is USABLE when it has a partner j, C_s[i] and C_t[j] exist, and the factorisation below does not fail.
 *     M = R C_s[i]:             M_rc = (R_r0 C_0c + R_r1 C_1c) + R_r2 C_2c                         (all nine; C symmetric)
 *     S = C_t[j] + M R^T:       S_rc = Ct_rc + ((M_r0 R_c0 + M_r1 R_c1) + M_r2 R_c2)                (r <= c only)
 *     S = L L^T, for j = 0, 1, 2:   d = S_jj - L_j0 L_j0 - ... (k < j ascending, one subtraction each); the row is not usable unless
 *                                   d > 2^-40 S_jj and d < +inf (the pivot rule of the point-to-plane step; false for a NaN);
 *                                   L_jj = sqrt(d);  L_ij = (S_ji - L_i0 L_j0 - ... (k < j)) / L_jj for i > j.
 *     y = T_k s (as pcpx_icp.h, NOT rounded to float32),  r = y - x_j,  u = y - o,
 *     J = [ -[u]_x | I ] (3 x 6):  rows (0, u_2, -u_1, 1, 0, 0), (-u_2, 0, u_0, 0, 1, 0), (u_1, -u_0, 0, 0, 0, 1).
 *     z = L^-1 r and K = L^-1 J by forward substitution, column by column:
 *         v_0 = a_0 / L_00,  v_1 = (a_1 - L_10 v_0) / L_11,  v_2 = ((a_2 - L_20 v_0) - L_21 v_1) / L_22.
 *   Over the usable rows, ascending, in the fixed order of the fits (per-thread strides over a fixed grid, a fixed tree within a
 *   block, the blocks in block order; no floating-point atomics), in the slots of the point-to-plane step:
 *     A_rc += (K_0r K_0c + K_1r K_1c) + K_2r K_2c  (r <= c, 21 entries),   b_r -= (K_0r z_0 + K_1r z_1) + K_2r z_2,
 *     sum += (z_0 z_0 + z_1 z_1) + z_2 z_2,   rows += 1.
 *   A row that is not usable is left out; it does not stop the loop.
 *   From here on the point-to-plane step unchanged: A x = b by Cholesky (a failed pivot: status PCPX_ICP_DEGENERATE, the result is
 *   T_k; so is a round without a usable row), x = (w, tau), the Cayley step, T_(k+1) = [dR R_k, dR (t_k - o) + o + tau];
 *   rms_k = sqrt(sum / rows), the root mean Mahalanobis residual.  "Partners unchanged" is a stopping rule, as there.
 *
 * OUTPUTS.  As pcpx_icp_rigid.
 *
 * PCPX_ERR_INVALID, from the arguments alone and before the handle or any device is touched: everything pcpx_icp_rigid refuses
 * (the radius, m, a NULL s with m > 0, max_iterations, a NULL transform); an unknown flag bit; a NULL source_cov with m > 0; a NULL
 * target_cov with any m; without PCPX_GICP_COVARIANCES an epsilon that is not finite, <= 0 or > 1; with it an epsilon other than 0.
 */
#ifndef PCPX_GICP_H
#define PCPX_GICP_H

#include "pcpx_icp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCPX_GICP_COVARIANCES 1u
#define PCPX_GICP_ON_DEVICE 2u

/* s: m x 3 float32; opt_pose: 16 doubles or NULL; source_cov and target_cov: m and n_in rows of 3 or 6 float32; out_transform: 16
 * doubles; opt_out_status, opt_out_iterations, opt_out_last_count: one uint32_t each; opt_out_count_trace: max_iterations uint32_t;
 * opt_out_rms_trace: max_iterations doubles; opt_out_partner: m uint32_t.  Host arrays, or device arrays with PCPX_GICP_ON_DEVICE. */
int pcpx_gicp_rigid(pcpx_index* index, const float* s, uint64_t m, const double* opt_pose, float radius, uint32_t max_iterations, uint32_t flags,
                    const float* source_cov, const float* target_cov, float epsilon, double* out_transform, uint32_t* opt_out_status,
                    uint32_t* opt_out_iterations, uint32_t* opt_out_last_count, uint32_t* opt_out_count_trace, double* opt_out_rms_trace,
                    uint32_t* opt_out_partner);

#ifdef __cplusplus
}
#endif
#endif /* PCPX_GICP_H */
