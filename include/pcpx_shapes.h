/*
 * pcpx_shapes.h -- sphere and cylinder detection of libpcpx.so: the sphere or the cylinder that most points of a cloud lie on, by a
 * fixed number of hypotheses from two oriented points each (Schnabel, Wahl, Klein 2007), every one scored against all points (RANSAC
 * without early termination); and the closed-form least-squares sphere or cylinder of a set of points.
 *
 * A companion of pcpx.h with its conventions: POD arguments, pcpx_status codes, pcpx_last_error().  No pcpx_index is involved: the
 * entry points take a device number like pcpx_planes.h.  Every refusal comes before any device is touched.
 *
 * WHERE THE ARRAYS LIVE.  Every call is declared once and takes a flag:
 *   PCPX_SHAPE_ON_DEVICE   every array argument, the single words (found, counts, status) included, is a device pointer on `device`,
 *                          owing its element type's alignment and no more.  Fully enqueued on `stream` (NULL: the legacy default
 *                          stream): no read-back and no synchronisation.  opt_rows_count is one uint64_t on the device, read on the
 *                          device.  The scratch stays taken from the device's pool until the stream has passed the call, as in
 *                          pcpx_register.h.
 *   without it             host arrays; the call returns when they are written (staged around the same device path).  `stream` must
 *                          be NULL.  opt_rows_count is one uint64_t of the host, read before anything is staged.
 *
 * INPUTS.  `points`, `normals`: n x 3 float32 each, row-major and dense.  The RANSAC needs the normals for both kinds; they are used
 * as given -- pass unit vectors -- and NOTHING DEPENDS ON THEIR SIGN: every formula below is invariant under N -> -N of any subset of
 * the rows, bit for bit, so the unoriented normals of a principal component analysis serve as they are.  `opt_rows`: uint32_t rows
 * of `points`, with room for `rows_capacity` of them (a host value, < 2^32 - 1); the number of rows is
 * C = min(*opt_rows_count, rows_capacity), or rows_capacity when opt_rows_count is NULL.  A NULL opt_rows (with rows_capacity = 0 and
 * a NULL opt_rows_count) means all n rows in order: C = n, rows[k] = k.
 *
 * RECORDS.  Those of pcpx_planes.h with the normal always present: row k (k < C) is USABLE iff rows[k] < n and its three coordinates
 * and its normal's three components are finite.  The origin o is the point of the ORIGIN ROW when that row is usable by the same
 * rule, else (0, 0, 0); the origin row is rows[0] (none when C = 0), or params->origin_row itself -- a row of `points`, whether listed
 * or not -- when that is not PCPX_SHAPE_ORIGIN_FIRST.  Row k becomes the record
 *     x_k = points[rows[k]] - o          (float32, one rounding per component)
 * and carries rows[k] and its normal N_k as given.  A row that is not usable, or one of whose differences is not finite, gets NaN as
 * x_k's first component (and a zero normal): it is then never an inlier, and a hypothesis that samples it is invalid by the rules
 * below, with no test of its own.
 *
 * SAMPLING.  That of pcpx_planes.h with two slots.  For hypothesis h (0 <= h < hypotheses):
 *     w      = fmix32(h XOR seed)
 *     slot_s = floor(fmix32(w + (s + 1) * 0x9E3779B9 mod 2^32) * C / 2^32)        s = 0, 1
 * (x_a, N_a) and (x_b, N_b) below are the records of slots 0 and 1.
 *
 * HYPOTHESIS.  float32, every operation rounded on its own (no FMA), in exactly this order.  A cross product p x q is
 * (p1*q2 - p2*q1, p2*q0 - p0*q2, p0*q1 - p1*q0); a sum of three terms is (t0 + t1) + t2; a . b = (a0*b0 + a1*b1) + a2*b2.
 *     w   = N_a x N_b                       lw2 = (w0*w0 + w1*w1) + w2*w2
 *     r   = x_b - x_a
 *     s   = ((r x N_b) . w) / lw2           t   = ((r x N_a) . w) / lw2
 *     c_a = x_a + s*N_a                     c_b = x_b + t*N_b          (the closest points of the two normal lines)
 *     c   = 0.5 * (c_a + c_b)
 *     sphere:    R = 0.5 * (sqrt(|x_a - c|^2) + sqrt(|x_b - c|^2))         |d|^2 = (d0*d0 + d1*d1) + d2*d2
 *     cylinder:  u = w / sqrt(lw2)  (each component divided by the one root),   R = 0.5 * (sqrt(q(x_a)) + sqrt(q(x_b)))   q as in SCORE
 * sqrt and division are correctly rounded.  The segment that joins the two closest points is parallel to w: c is the sphere's centre,
 * and it is a point of the cylinder's axis, whose direction is w.  One computation serves both kinds.
 *
 * VALIDITY.  Hypothesis h is valid iff all of: C >= 2 and the two slots differ; lw2 > 0 and finite; lw2 >= min_normal_sin *
 * min_normal_sin (one float32 product: the two normals span an angle whose sine is at least min_normal_sin, for unit normals); c0,
 * c1, c2 and R are finite; min_radius <= R <= max_radius (max_radius may be +inf); and for a cylinder under PCPX_SHAPE_AXIS
 * (params->axis = A, used as given -- pass a unit vector) |u . A| >= min_axis_cos, which keeps the cylinders ALONG A: the poles and
 * trunks, with A the vertical.  A NaN compares false everywhere.
 *
 * SCORE.  No square root and no division per record.  Per hypothesis, once:
 *     lo = max(R - max_distance, 0), lo2 = lo*lo, hi = R + max_distance, hi2 = hi*hi, cos2 = min_normal_cos*min_normal_cos
 * Per record k < C:
 *     d = x_k - c
 *     sphere:    e = d
 *     cylinder:  s = d . u,  e_j = d_j - s*u_j                 (not |d|^2 - s^2: that cancels far along the axis)
 *     q = (e0*e0 + e1*e1) + e2*e2
 *     inlier iff lo2 <= q and q <= hi2 and, under PCPX_SHAPE_NORMALS, also g*g >= cos2*q with g = e . N_k
 * (the record's normal is within the angle of the shape's: for unit normals |cos| >= min_normal_cos).  BEST is the valid hypothesis
 * of largest score, ties going to the lowest h; there is no early termination.  found = 0 when no hypothesis is valid.
 *
 * OUTPUTS, all optional but found: found (0 or 1); the best h; its score; the inliers as rows of `points` (rows[k] of the inlier
 * records k, in record order: ascending under a NULL opt_rows) with room for rows_capacity (n under a NULL opt_rows) entries, and
 * their number in one uint64_t; the MODEL as 8 doubles in the caller's coordinates,
 *     sphere     (cx, cy, cz, R, 0, 0, 0, 0)
 *     cylinder   (px, py, pz, ux, uy, uz, R, 0)          p: a point of the axis, u: its unit direction
 * with the centre or point double(c_j) + double(o_j), R and u the float32 values widened, and u given the sign that makes its
 * component of largest magnitude positive (the lowest index on ties); and, with PCPX_SHAPE_REFIT, the SHAPE FIT over the inliers
 * (over that list of rows), or the hypothesis model itself where that fit is degenerate.  When found = 0: zeros everywhere.  Without
 * PCPX_SHAPE_REFIT the refit array is not touched.
 *
 * SHAPE FIT.  The algebraic least-squares sphere (the one linear in the centre and R^2 - |centre|^2), or for a cylinder the axis from
 * the normals and the same fit of a circle in the plane across it, over the usable rows (rows[j] < n, finite coordinates; for a
 * cylinder a finite normal too), over all n rows or a list of them.  Normals are required for PCPX_SHAPE_CYLINDER and not read for
 * PCPX_SHAPE_SPHERE.  Everything is float64 without FMA, and every sum over the rows is formed in the fixed order of the plane fit
 * (pcpx_planes.h: 64 blocks of 256 threads striding over the list, a fixed tree within a block, the blocks' partial sums added in
 * block order), so the host form, the device form and the RANSAC refit agree to the bit.
 *   1. The number of usable rows N and the sums of their coordinates; m = sum / N.  Cylinder: also the six terms nn_00, nn_01, nn_02,
 *      nn_11, nn_12, nn_22 of sum N_a*N_b -- not centred, so the normals' signs play no part -- and u = the unit eigenvector of its
 *      smallest eigenvalue by the cyclic Jacobi sweeps of the plane fit, with that fit's sign rule: a cylinder's normals are
 *      perpendicular to its axis, so the axis is the direction they span least.
 *   2. y = x - m; cylinder: s = (y0*u0 + y1*u1) + y2*u2, then y_j <- y_j - s*u_j.  q = (y0*y0 + y1*y1) + y2*y2.  Ten sums: S_00, S_01,
 *      S_02, S_11, S_12, S_22 of y_a*y_b, B_0, B_1, B_2 of y_a*q, and Q of q.
 *   3. b_a = 0.5 * B_a.  Sphere: A = S.  Cylinder: k = 0.5 * ((S_00 + S_11) + S_22) and A_ab = S_ab + (k*u_a)*u_b for a <= b (b is
 *      perpendicular to u, so the solution is the circle's centre in the plane, and A is positive definite).  A c' = b by Cholesky:
 *          l00 = sqrt(A_00)                 l10 = A_01 / l00                         l20 = A_02 / l00
 *          p1  = A_11 - l10*l10             l11 = sqrt(p1)                           l21 = (A_12 - l20*l10) / l11
 *          p2  = A_22 - (l20*l20 + l21*l21) l22 = sqrt(p2)
 *          z0  = b_0 / l00                  z1  = (b_1 - l10*z0) / l11               z2  = (b_2 - (l20*z0 + l21*z1)) / l22
 *          c'2 = z2 / l22                   c'1 = (z1 - l21*c'2) / l11               c'0 = (z0 - (l10*c'1 + l20*c'2)) / l00
 *      R = sqrt(Q / N + ((c'0*c'0 + c'1*c'1) + c'2*c'2)); the centre (the axis point) = m + c'.  The fit is DEGENERATE iff N < 4, or
 *      one of the pivots A_00, p1, p2 is not > 0, or one of c'0, c'1, c'2, R is not finite.
 *   4. The root mean square of sqrt(q') - R over the usable rows, q' = q of SCORE's e about the fitted centre or axis, in float64:
 *      sqrt(sum / N).
 * A degenerate fit gives a model of zeros, a NaN root mean square and the status PCPX_SHAPE_FIT_DEGENERATE (else PCPX_SHAPE_FIT_OK).
 * The radius gate does not apply to fits.  Coplanar points give a huge sphere: the least-squares answer, not an error.  The cylinder
 * fit is linear, in two steps; it is not refined by a non-linear iteration.
 *
 * PCPX_ERR_INVALID, before any device is touched: a NULL points, normals (the RANSAC; the cylinder fit) or rows with a non-zero
 * size; a NULL opt_rows with rows_capacity != 0 or a count; n or rows_capacity >= 2^32 - 1; hypotheses = 0 or >= 2^32 - 1; an unknown
 * kind or flag bit; PCPX_SHAPE_AXIS with a sphere; max_distance negative or NaN; min_radius negative or NaN; max_radius < min_radius
 * or NaN; min_normal_sin, min_normal_cos or min_axis_cos outside [0, 1] or NaN; under the axis flag an axis that is zero or not
 * finite; PCPX_SHAPE_REFIT without a refit array; a non-NULL stream without PCPX_SHAPE_ON_DEVICE; reserved != 0; a NULL params,
 * found or model where it is not optional.
 */
#ifndef PCPX_SHAPES_H
#define PCPX_SHAPES_H

#include "pcpx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCPX_SHAPE_SPHERE 1u
#define PCPX_SHAPE_CYLINDER 2u

#define PCPX_SHAPE_REFIT 1u
#define PCPX_SHAPE_NORMALS 2u   /* the normal gate of SCORE */
#define PCPX_SHAPE_AXIS 4u      /* cylinders only */
#define PCPX_SHAPE_ON_DEVICE 8u

#define PCPX_SHAPE_ORIGIN_FIRST 0xFFFFFFFFu /* origin_row: rows[0] */
#define PCPX_SHAPE_FIT_OK 0u
#define PCPX_SHAPE_FIT_DEGENERATE 1u

typedef struct pcpx_shape_params {
    uint64_t hypotheses;  /* T, 1 .. 2^32 - 2 */
    uint32_t kind;        /* PCPX_SHAPE_SPHERE or PCPX_SHAPE_CYLINDER */
    uint32_t seed;
    uint32_t flags;       /* PCPX_SHAPE_REFIT | PCPX_SHAPE_NORMALS | PCPX_SHAPE_AXIS | PCPX_SHAPE_ON_DEVICE */
    float max_distance;
    float min_radius;
    float max_radius;     /* +inf: no upper bound */
    float min_normal_sin; /* of the two sampled normals */
    float min_normal_cos; /* read under PCPX_SHAPE_NORMALS */
    float axis[3];        /* read under PCPX_SHAPE_AXIS */
    float min_axis_cos;   /* read under PCPX_SHAPE_AXIS */
    uint32_t origin_row;  /* PCPX_SHAPE_ORIGIN_FIRST or a row of points */
    uint32_t reserved;    /* 0 */
} pcpx_shape_params;

/* Host arithmetic only: how a call with `hypotheses` hypotheses and room for `rows_capacity` records (n under a NULL opt_rows) is
 * laid out.  The records are cut into *out_segments segments of *out_segment_rows consecutive records (a multiple of 256; the last
 * segment may be shorter; 0 and 0 when rows_capacity = 0), one wavefront per (64 consecutive hypotheses, segment); segments that
 * begin at or beyond the count do nothing.  *out_scratch_bytes: the device scratch the call takes from the device's pool.  Any
 * output may be NULL.  pcpx_shape_ransac uses exactly this plan. */
int pcpx_shape_plan(uint64_t hypotheses, uint64_t rows_capacity, uint32_t* out_segments, uint64_t* out_segment_rows, uint64_t* out_scratch_bytes);

/* out_found, opt_out_hypothesis, opt_out_score: one uint32_t each; opt_out_inliers: room for rows_capacity (n under a NULL opt_rows)
 * uint32_t, entries [0, *opt_out_inlier_count) are written; opt_out_inlier_count: one uint64_t; opt_out_model, opt_out_refit: 8
 * doubles each. */
int pcpx_shape_ransac(const float* points, uint64_t n, const float* normals, const uint32_t* opt_rows, uint64_t rows_capacity,
                      const uint64_t* opt_rows_count, const pcpx_shape_params* params, int device, void* stream, uint32_t* out_found,
                      uint32_t* opt_out_hypothesis, uint32_t* opt_out_score, uint32_t* opt_out_inliers, uint64_t* opt_out_inlier_count,
                      double* opt_out_model, double* opt_out_refit);

/* kind: PCPX_SHAPE_SPHERE or PCPX_SHAPE_CYLINDER; flags: PCPX_SHAPE_ON_DEVICE or 0.  out_model: 8 doubles; opt_out_rms: one double;
 * opt_out_status: one uint32_t.  (opt_rows not NULL with room for no rows: a list of no rows.) */
int pcpx_shape_fit(const float* points, uint64_t n, const float* opt_normals, const uint32_t* opt_rows, uint64_t rows_capacity,
                   const uint64_t* opt_rows_count, uint32_t kind, uint32_t flags, int device, void* stream, double* out_model, double* opt_out_rms,
                   uint32_t* opt_out_status);

#ifdef __cplusplus
}
#endif
#endif /* PCPX_SHAPES_H */
