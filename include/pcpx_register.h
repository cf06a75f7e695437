/*
 * pcpx_register.h -- rigid registration of libpcpx.so from correspondences: the rigid pose that most of a list of (source, target)
 * pairs agree on, by a fixed number of three-pair hypotheses each scored against all pairs (RANSAC without early termination), and
 * the least-squares rigid fit over a list of pairs (Horn's closed form).
 *
 * A companion of pcpx.h with its conventions: POD arguments, pcpx_status codes, pcpx_last_error().  No pcpx_index is involved: the
 * entry points take a device number (and the _dev forms a stream) like pcpx_match.h.  The _dev forms never synchronise and read
 * nothing back.
 *
 * INPUTS.  `p`: np x 3 float32, `q`: nq x 3 float32, row-major and dense.  `pairs`: uint32_t {source row of p, target row of q}, as
 * pcpx_match_correspondences writes them, with room for `pairs_capacity` of them (a host value, < 2^32 - 1).  The number of
 * correspondences is C = min(*d_opt_count, pairs_capacity) -- d_opt_count: one uint64_t on the device, the word that
 * pcpx_match_correspondences_dev leaves there; it is read on the device -- or pairs_capacity when d_opt_count is NULL.  The host forms
 * take C as a plain count.
 *
 * RECORDS.  Correspondence k is USABLE iff source_k < np, target_k < nq and its six coordinates are finite.  The origins are
 * correspondence 0's own points, o_p = p[source_0] and o_q = q[target_0], or both (0, 0, 0) when correspondence 0 is not usable.
 * Correspondence k becomes
 *     p_k = p[source_k] - o_p        q_k = q[target_k] - o_q        (float32, one rounding per component)
 * so a cloud far from the origin loses nothing beyond its own quantisation.  A correspondence that is not usable, or one of whose
 * six differences is not finite, gets NaN as the first component of p_k: it is then never an inlier, and a hypothesis that samples
 * it is invalid by the rules below, with no test of its own.
 *
 * SAMPLING, stateless.  fmix32 as in pcpx_subsample.h.  For hypothesis h (0 <= h < hypotheses):
 *     w      = fmix32(h XOR seed)
 *     slot_s = floor(fmix32(w + (s + 1) * 0x9E3779B9 mod 2^32) * C / 2^32)        s = 0, 1, 2  (a 64-bit product and a shift)
 * x0, x1, x2 below are the records of slots 0, 1, 2.
 *
 * HYPOTHESIS.  float32, every operation rounded on its own (no FMA), in exactly this order, for each side (x = p and x = q):
 *     a   = x1 - x0                         b = x2 - x0                       d = x2 - x1
 *     la2 = (a0*a0 + a1*a1) + a2*a2         lb2, ld2 likewise from b and d
 *     u   = a / sqrt(la2)                   (sqrt and division correctly rounded, each component divided by the one root)
 *     c   = a x b:  c0 = a1*b2 - a2*b1,  c1 = a2*b0 - a0*b2,  c2 = a0*b1 - a1*b0
 *     lc2 = (c0*c0 + c1*c1) + c2*c2         w = c / sqrt(lc2)
 *     v   = w x u:  v0 = w1*u2 - w2*u1,  v1 = w2*u0 - w0*u2,  v2 = w0*u1 - w1*u0
 *     F   = [u v w] as columns:  F[r][0] = u_r, F[r][1] = v_r, F[r][2] = w_r
 * and then
 *     R[r][c] = (Fq[r][0]*Fp[c][0] + Fq[r][1]*Fp[c][1]) + Fq[r][2]*Fp[c][2]
 *     t_r     = q0_r - ((R[r][0]*p0_0 + R[r][1]*p0_1) + R[r][2]*p0_2)            (p0, q0: the two halves of record x0)
 * This is the TRIAD alignment of the two triangles, not the three-point least-squares fit: it is exact for congruent triangles, and
 * it privileges x0 (mapped onto its partner exactly) and the edge x0 x1 (mapped onto its partner's direction exactly).
 *
 * VALIDITY.  Hypothesis h is valid iff C >= 3, its three slots differ, la2 and lc2 of both sides are > 0 and finite, and for each of
 * the three edges (L = la2, lb2, ld2) Lp >= s2 * Lq and Lq >= s2 * Lp hold -- each one float32 product and one comparison, a NaN
 * comparing false; s2 = edge_similarity_sq, 0 = no gate (the comparisons are still made: a non-finite edge fails them).
 *
 * SCORE.  For every correspondence k < C:
 *     e_r = (((R[r][0]*p_0 + R[r][1]*p_1) + R[r][2]*p_2) + t_r) - q_r
 *     d2  = (e_0*e_0 + e_1*e_1) + e_2*e_2
 * k is an inlier iff d2 <= max_distance_sq.  The score is the number of inliers.  BEST is the valid hypothesis of largest score,
 * ties going to the lowest h.  found = 0 when no hypothesis is valid.
 *
 * OUTPUTS, all optional but the first: found (0 or 1); the best h; its score; the inliers' positions in `pairs`, ascending, and their
 * number in one uint64_t; the best hypothesis as 16 doubles, a row-major 4 x 4 matrix [R t; 0 0 0 1] that takes points of p to
 * points of q: R is the float32 values widened and, in float64 without FMA,
 *     t_abs_r = (o_q_r + t_r) - ((R[r][0]*o_p_0 + R[r][1]*o_p_1) + R[r][2]*o_p_2);
 * and, with PCPX_RANSAC_REFIT, the least-squares transform over the inliers (pcpx_rigid_fit on those positions), or the hypothesis
 * transform when there are fewer than three inliers.  When found = 0: identity transforms and zero counts.  Without
 * PCPX_RANSAC_REFIT the refit array is not touched.
 *
 * RIGID FIT.  The rotation R and translation t that minimise the sum of |R p + t - q|^2 over the usable pairs, as the same 4 x 4
 * matrix, and the root of the mean of those squares.  The pairs are all C correspondences, or, with a list of positions, the
 * correspondences pairs[positions[j]] for j < min(*d_opt_positions_count, positions_capacity) (positions_capacity when that is NULL);
 * a position >= C is not usable.  Everything is float64: the centroids, H = sum (p - pbar)(q - qbar)^T, Horn's symmetric 4 x 4
 * matrix of H, the eigenvector of its largest eigenvalue by cyclic Jacobi sweeps to convergence, the unit quaternion's rotation
 * matrix (always a proper rotation, also for a mirrored set), t = qbar - R pbar.  The sums are formed in a fixed order -- per-thread
 * strides, a fixed tree within a block, the blocks' partial sums added in block order, no floating-point atomics -- so two calls
 * return the same bits; the order depends on the pairs alone, not on the capacities, so the host form, the _dev form and the refit
 * agree to the bit too.  With fewer than three usable pairs: the identity and a NaN root mean square.  For a collinear set the
 * minimiser is not unique (any rotation about the line serves); one of them is returned.
 *
 * PCPX_ERR_INVALID, before any device is touched: a NULL p, q or pairs with a non-zero size; pairs_capacity or positions_capacity
 * >= 2^32 - 1; np or nq >= 2^32; hypotheses = 0 or >= 2^32 - 1; max_distance_sq negative or NaN; edge_similarity_sq outside [0, 1] or
 * NaN; an unknown flag bit; PCPX_RANSAC_REFIT without a refit array; a NULL found or transform where it is not optional.
 */
#ifndef PCPX_REGISTER_H
#define PCPX_REGISTER_H

#include "pcpx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCPX_RANSAC_REFIT 1u

/* Host arithmetic only: how a call with `hypotheses` hypotheses and room for `pairs_capacity` correspondences is laid out.  The
 * correspondences are cut into *out_segments segments of *out_segment_rows consecutive records (a multiple of 256; the last segment
 * may be shorter; 0 and 0 when pairs_capacity = 0), one wavefront per (64 consecutive hypotheses, segment); segments that begin at
 * or beyond the device's count do nothing.  *out_scratch_bytes: the device scratch that pcpx_ransac_rigid(_dev) takes from the
 * device's pool for these sizes.  Any output may be NULL.  The calls below use exactly this plan. */
int pcpx_ransac_plan(uint64_t hypotheses, uint64_t pairs_capacity, uint32_t* out_segments, uint64_t* out_segment_rows,
                     uint64_t* out_scratch_bytes);

/* Device arrays on `device`: d_p, d_q, d_pairs, d_opt_count as above; d_out_found, d_opt_out_hypothesis, d_opt_out_score: one
 * uint32_t each; d_opt_out_inliers: room for pairs_capacity uint32_t, entries [0, *d_opt_out_inlier_count) are written;
 * d_opt_out_inlier_count: one uint64_t; d_opt_out_transform, d_opt_out_refit: 16 doubles each.  Fully enqueued on `stream`: no
 * read-back and no synchronisation.  The scratch stays taken from the device's pool until the stream has passed the call, as in
 * pcpx_match.h. */
int pcpx_ransac_rigid_dev(const float* d_p, uint64_t np, const float* d_q, uint64_t nq, const uint32_t* d_pairs, uint64_t pairs_capacity,
                          const uint64_t* d_opt_count, uint64_t hypotheses, uint32_t seed, float max_distance_sq, float edge_similarity_sq,
                          uint32_t flags, int device, void* stream, uint32_t* d_out_found, uint32_t* d_opt_out_hypothesis,
                          uint32_t* d_opt_out_score, uint32_t* d_opt_out_inliers, uint64_t* d_opt_out_inlier_count,
                          double* d_opt_out_transform, double* d_opt_out_refit);
/* the same with host arrays and a plain count; opt_out_inliers has room for `count` entries, *opt_out_score of which are written */
int pcpx_ransac_rigid(const float* p, uint64_t np, const float* q, uint64_t nq, const uint32_t* pairs, uint64_t count, uint64_t hypotheses,
                      uint32_t seed, float max_distance_sq, float edge_similarity_sq, uint32_t flags, int device, uint32_t* out_found,
                      uint32_t* opt_out_hypothesis, uint32_t* opt_out_score, uint32_t* opt_out_inliers, double* opt_out_transform,
                      double* opt_out_refit);

/* Device arrays: d_opt_positions (positions_capacity uint32_t) and d_opt_positions_count (one uint64_t) as above, or NULL, 0 and NULL
 * for all correspondences; d_out_transform: 16 doubles; d_opt_out_rms: one double.  Fully enqueued on `stream`. */
int pcpx_rigid_fit_dev(const float* d_p, uint64_t np, const float* d_q, uint64_t nq, const uint32_t* d_pairs, uint64_t pairs_capacity,
                       const uint64_t* d_opt_count, const uint32_t* d_opt_positions, uint64_t positions_capacity,
                       const uint64_t* d_opt_positions_count, int device, void* stream, double* d_out_transform, double* d_opt_out_rms);
/* the same with host arrays and plain counts (opt_positions NULL: all `count` correspondences; not NULL with positions_count = 0: a
 * list of no pairs) */
int pcpx_rigid_fit(const float* p, uint64_t np, const float* q, uint64_t nq, const uint32_t* pairs, uint64_t count,
                   const uint32_t* opt_positions, uint64_t positions_count, int device, double* out_transform, double* opt_out_rms);

#ifdef __cplusplus
}
#endif
#endif /* PCPX_REGISTER_H */
