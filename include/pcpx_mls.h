/*
 * pcpx_mls.h -- moving least squares (MLS) projection of libpcpx.so (Levin; Alexa et al. 2003; PCL's MovingLeastSquares): every
 * sphere's centre is projected onto a Gaussian-weighted plane (order 1) or onto a quadric over that plane (order 2), with the
 * surface normal and, for the quadric, the mean and Gaussian curvature at the projection -- two walks of the index, no neighbour
 * lists.  Denoised points with normals and curvatures that belong to them, for reconstruction and region growing.
 *
 * A companion of pcpx.h with its conventions: POD arguments, pcpx_status codes, pcpx_last_error(); a rank-local (shard) handle
 * is refused with PCPX_ERR_UNSUPPORTED.  The sphere and its points are those of pcpx_radius.h:
 *   - a sphere holds every indexed point with d2 <= r*r (d = p - q, float32, no FMA; q the sphere's centre), q itself included;
 *   - a point outside the index's voxel grid is in no sphere, and its own (self) row is an empty sphere; so is a NaN or +-inf row
 *     or query.
 *
 * Stage 1, the plane.  Weight w = expf(d2 * k), k = -1 / (h*h) formed once in float32 (h: gauss_h).  One walk accumulates the count,
 * W = sum w, S = sum w d and Q = sum w d d^T in float32, about q.  Then m = S / W, C = Q - S m^T, the normal n = the eigenvector of
 * C's smallest eigenvalue by the solver and selection rule of every other normal here (pcpx_radius.h), the signed offset t = m . n,
 * and the plane projection of q is q + t n.
 *
 * Stage 2, the quadric (order 2 only).  Frame: a = the coordinate axis where |n| is smallest (ties: the lowest axis),
 * U = normalise(n x a), V = n x U, origin o = t n (relative to q).  A second walk over the same sphere with the same weights: for
 * every neighbour e = d - o, u = (e . U) / r, v = (e . V) / r, z = (e . n) / r (dividing by r keeps the system's scale out of its
 * conditioning; the kernel multiplies by the float32 reciprocal of r, formed once), basis b = (1, u, v, u^2, u v, v^2); it accumulates the 21 unique terms of sum w b b^T and the 6 of sum w z b in
 * float32.  The 6 x 6 system is solved in float64 by Cholesky; the fit is refused when any pivot is <= PCPX_MLS_PIVOT_MIN times
 * that diagonal's own entry (or not finite).  With the solution c:
 *   displacement  o + c0 r n
 *   normal        normalise(n - c1 U - c2 V): the plane normal's hemisphere
 *   curvatures    of the graph z(u, v) at the origin, with h_u = c1, h_v = c2, h_uu = 2 c3 / r, h_uv = c4 / r, h_vv = 2 c5 / r and
 *                 g = 1 + h_u^2 + h_v^2:  K = (h_uu h_vv - h_uv^2) / g^2,
 *                 H = ((1 + h_v^2) h_uu - 2 h_u h_v h_uv + (1 + h_u^2) h_vv) / (2 g^(3/2)), signed with respect to the output normal.
 *
 * Outputs per row; any may be NULL, not all:
 *   displacements  3 floats: what is added to q.
 *   points         3 floats: q + displacement, one float32 rounding per coordinate.  (At |q| = 2^20 a point is quantised to
 *                  0.06 ... 0.125 and the displacement is not: hence both outputs.)
 *   normals        3 floats, unit length.
 *   curvatures     2 floats (H, K); NaN unless fit = 2.
 *   count          the number of points in the sphere.
 *   fit            0 = unchanged, 1 = plane, 2 = quadric.
 * Fallbacks:
 *   count < 3: fit 0, displacement 0, `points` is the row's (the query's) own bits, NaN payloads included, normal (0, 0, 1) -- what
 *   the solver gives for a zero matrix.  The same when W is not > 0 (a gauss_h so small that every weight underflowed).
 *   order 2 with count < 6 or a refused Cholesky: the stage-1 result, fit 1.
 *   copies of one point only (C = 0): fit 1, displacement 0.
 * PCPX_ERR_INVALID: radius < 0 or NaN, gauss_h <= 0 or NaN, order not 1 or 2, every output NULL, a NULL handle.
 */
#ifndef PCPX_MLS_H
#define PCPX_MLS_H

#include "pcpx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the smallest accepted ratio of a Cholesky pivot to its own diagonal entry: 2^-12 */
#define PCPX_MLS_PIVOT_MIN (1.0 / 4096.0)

/* d_opt_*: device arrays by input row; sorted-slice arguments as pcpx_shape_features_self_dev: exactly the rows of the slice's
 * points are written, every other row is left untouched -- except that a slice that covers the whole curve order (sorted_first 0,
 * sorted_count >= the index size) also writes the fit-0 values at the rows of points outside the voxel grid.  A slice may start
 * and end inside a query group of 64 (sorted_first need not be a multiple of 64 here): the other lanes of those groups idle.
 * Enqueued on the handle's stream (pcpx_index_synchronize waits for it). */
int pcpx_mls_project_self_dev(pcpx_index* idx, float radius, float gauss_h, int order, uint64_t sorted_first, uint64_t sorted_count,
                              float* d_opt_points, float* d_opt_displacements, float* d_opt_normals, float* d_opt_curvatures,
                              uint32_t* d_opt_count, uint32_t* d_opt_fit);
/* host arrays, one row per input point (n_in rows) */
int pcpx_mls_project_self(pcpx_index* idx, float radius, float gauss_h, int order, float* opt_points, float* opt_displacements,
                          float* opt_normals, float* opt_curvatures, uint32_t* opt_count, uint32_t* opt_fit);
/* nq external spheres (host arrays, q_xyz nq x 3); radii NULL -> `radius` for all, else one radius per sphere (each >= 0), and the
 * Gaussian's width scales with each sphere: sphere i uses gauss_h * radii[i] / radius (float32, in that order), so `radius` is then
 * the radius that gauss_h belongs to and must be > 0.  A sphere of radius 0 (copies of its centre only) has weight 1. */
int pcpx_mls_project_batch(pcpx_index* idx, const float* q_xyz, const float* radii, float radius, float gauss_h, int order, uint64_t nq,
                           float* opt_points, float* opt_displacements, float* opt_normals, float* opt_curvatures, uint32_t* opt_count,
                           uint32_t* opt_fit);

#ifdef __cplusplus
}
#endif
#endif /* PCPX_MLS_H */
