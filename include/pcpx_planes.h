/*
 * pcpx_planes.h -- plane detection of libpcpx.so: the plane that most points of a cloud lie on, by a fixed number of three-point
 * hypotheses each scored against all points (RANSAC without early termination); the least-squares plane of a set of points; and the
 * extraction of plane after plane, every round on the points the earlier ones left, as one enqueued loop.
 *
 * A companion of pcpx.h with its conventions: POD arguments, pcpx_status codes, pcpx_last_error().  No pcpx_index is involved: the
 * entry points take a device number (and the _dev forms a stream) like pcpx_register.h.  The _dev forms never synchronise and read
 * nothing back.  Every refusal comes before any device is touched.
 *
 * INPUTS.  `points`: n x 3 float32, row-major and dense.  `opt_normals`: n x 3 float32 or NULL (only the normal gate reads them).
 * `opt_rows`: uint32_t rows of `points`, with room for `rows_capacity` of them (a host value, < 2^32 - 1); the number of rows is
 * C = min(*d_opt_rows_count, rows_capacity) -- one uint64_t on the device, read on the device -- or rows_capacity when that is NULL.
 * A NULL opt_rows (with rows_capacity = 0) means all n rows in order: C = n, rows[k] = k.  The host forms take C as a plain count.
 *
 * RECORDS.  Row k (k < C) is USABLE iff rows[k] < n and its three coordinates are finite and, with the normal gate on
 * (PCPX_PLANE_NORMALS), its normal's three components are finite too.  The origin o is the point of the ORIGIN ROW when that row is
 * usable by the same rule, else (0, 0, 0); the origin row is rows[0] (none when C = 0), or params->origin_row itself -- a row of
 * `points`, whether listed or not -- when that is not PCPX_PLANE_ORIGIN_FIRST.  Row k becomes the record
 *     x_k = points[rows[k]] - o          (float32, one rounding per component)
 * and carries rows[k] and, with the gate, its normal N_k as given.  A row that is not usable, or one of whose differences is not
 * finite, gets NaN as x_k's first component: it is then never an inlier, and a hypothesis that samples it is invalid by the rules
 * below, with no test of its own.
 *
 * SAMPLING, stateless, that of pcpx_register.h.  fmix32 as in pcpx_subsample.h.  For hypothesis h (0 <= h < hypotheses):
 *     w      = fmix32(h XOR seed)
 *     slot_s = floor(fmix32(w + (s + 1) * 0x9E3779B9 mod 2^32) * C / 2^32)        s = 0, 1, 2  (a 64-bit product and a shift)
 * x0, x1, x2 below are the records of slots 0, 1, 2.
 *
 * HYPOTHESIS.  float32, every operation rounded on its own (no FMA), in exactly this order:
 *     a   = x1 - x0                         b = x2 - x0
 *     c   = a x b:  c0 = a1*b2 - a2*b1,  c1 = a2*b0 - a0*b2,  c2 = a0*b1 - a1*b0
 *     lc2 = (c0*c0 + c1*c1) + c2*c2
 *     n   = c / sqrt(lc2)                   (sqrt and division correctly rounded, each component divided by the one root)
 *     m   = (n0*x0_0 + n1*x0_1) + n2*x0_2
 *
 * VALIDITY.  Hypothesis h is valid iff C >= 3, its three slots differ, lc2 > 0 and finite and, with the axis gate (PCPX_PLANE_AXIS:
 * params->axis = A, used as given -- pass a unit vector -- and params->min_axis_cos in [0, 1]),
 *     |(n0*A0 + n1*A1) + n2*A2| >= min_axis_cos        (a NaN comparing false)
 * which keeps the planes perpendicular to A: the ground, with A the vertical.
 *
 * SCORE.  The number of k < C with
 *     e = ((n0*x_k0 + n1*x_k1) + n2*x_k2) - m        and        |e| <= max_distance        (a NaN comparing false)
 * and, with the normal gate, also |(n0*N_k0 + n1*N_k1) + n2*N_k2| >= min_normal_cos.  BEST is the valid hypothesis of largest score,
 * ties going to the lowest h; there is no early termination.  found = 0 when no hypothesis is valid.
 *
 * OUTPUTS, all optional but found: found (0 or 1); the best h; its score; the inliers as rows of `points` (rows[k] of the inlier
 * records k, in record order: ascending under a NULL opt_rows) and their number in one uint64_t; the plane as 4 doubles (n0, n1, n2,
 * d) with n . x + d = 0 in the caller's coordinates: n the float32 values widened and, in float64 without FMA,
 *     d = -(m + ((n0*o0 + n1*o1) + n2*o2));
 * and, with PCPX_PLANE_REFIT, the least-squares plane over the inliers (PLANE FIT over that list of rows) with the sign that makes
 * its normal's product with the hypothesis's n non-negative, or the hypothesis plane itself where fewer than three inliers are
 * usable.  When found = 0: zeros everywhere.  Without PCPX_PLANE_REFIT the refit array is not touched.
 *
 * PLANE FIT.  The plane that minimises the sum of squared distances of the usable rows (rows[j] < n, finite coordinates; normals
 * play no part), over all n rows or a list of them.  Everything is float64: the number of usable rows N and the sums of their
 * coordinates; the centroid c = sum / N; the six terms xx, xy, xz, yy, yz, zz of the scatter, sum (x_a - c_a)*(x_b - c_b); the
 * eigenvector of its smallest eigenvalue by cyclic Jacobi sweeps to convergence, normalised; the sign that makes its component of
 * largest magnitude positive (the lowest index on ties); d = -((n0*c0 + n1*c1) + n2*c2); and from a third pass the root of the mean
 * of e^2, e = (n0*(x0 - c0) + n1*(x1 - c1)) + n2*(x2 - c2).  The sums are formed in a fixed order -- 64 blocks of 256 threads
 * striding over the list, a fixed tree within a block, the blocks' partial sums added in block order, no floating-point atomics --
 * so two calls return the same bits, and since the order depends on the list alone the host form, the _dev form and the RANSAC
 * refit agree to the bit too.  With fewer than three usable rows: zeros and a NaN root mean square.  For a set whose two smallest
 * eigenvalues are equal (a line, a ball) the minimiser is not unique; one of them is returned.
 *
 * EXTRACTION.  pcpx_extract_planes runs up to params->max_planes rounds over all n rows, enqueued whole: no host round trip; a
 * `done` word on the device is read first by every kernel of a later round.  The records are made once, with the origin of row 0
 * (origin_row is not read).  Round r (r = 0, 1, ...):
 *     1. the RANSAC above over the live records -- all of them in round 0 -- with seed_r = fmix32((seed + r) mod 2^32);
 *     2. stops, for good, when found = 0 or the score is below params->min_inliers;
 *     3. otherwise writes label r to the inliers' rows, the plane (and with PCPX_PLANE_REFIT its refit) and the score to entry r;
 *     4. compacts the records that are not inliers, in order, into the other of two buffers: the live records of round r + 1.
 * So round r is pcpx_plane_ransac over the rows still unlabelled, in ascending order, with seed_r and origin_row = 0, bit for bit.
 * Outputs: labels, n uint32_t, PCPX_PLANE_NONE where no plane took the row; the number of planes; planes, refits (max_planes x 4
 * doubles each) and scores (max_planes uint32_t), zeros from the number of planes on.
 *
 * PCPX_ERR_INVALID, before any device is touched: a NULL points, normals-under-the-gate or rows with a non-zero size; a NULL
 * opt_rows with rows_capacity != 0; n or rows_capacity >= 2^32 - 1; hypotheses = 0 or >= 2^32 - 1; max_distance negative or NaN;
 * min_normal_cos (under its gate) or min_axis_cos (under its gate) outside [0, 1] or NaN; under the axis gate an axis that is zero
 * or not finite; PCPX_PLANE_NORMALS without normals; an unknown flag bit; PCPX_PLANE_REFIT without a refit array; a NULL params,
 * found, labels, count or plane where it is not optional; for the extraction max_planes = 0 or above PCPX_PLANES_MAX.
 */
#ifndef PCPX_PLANES_H
#define PCPX_PLANES_H

#include "pcpx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCPX_PLANE_REFIT 1u
#define PCPX_PLANE_NORMALS 2u
#define PCPX_PLANE_AXIS 4u
#define PCPX_PLANE_NONE 0xFFFFFFFFu         /* the label of a row that no plane took */
#define PCPX_PLANE_ORIGIN_FIRST 0xFFFFFFFFu /* origin_row: rows[0] */
#define PCPX_PLANES_MAX 64u                 /* the most rounds of one pcpx_extract_planes call (a round is some twenty launches) */

typedef struct pcpx_plane_params {
    uint64_t hypotheses;  /* T, 1 .. 2^32 - 2 */
    uint32_t seed;
    uint32_t flags;       /* PCPX_PLANE_REFIT | PCPX_PLANE_NORMALS | PCPX_PLANE_AXIS */
    float max_distance;
    float min_normal_cos; /* read under PCPX_PLANE_NORMALS */
    float axis[3];        /* read under PCPX_PLANE_AXIS */
    float min_axis_cos;   /* read under PCPX_PLANE_AXIS */
    uint32_t origin_row;  /* pcpx_plane_ransac only: PCPX_PLANE_ORIGIN_FIRST or a row of points */
    uint32_t min_inliers; /* pcpx_extract_planes only */
    uint32_t max_planes;  /* pcpx_extract_planes only: 1 .. PCPX_PLANES_MAX */
    uint32_t reserved;    /* 0 */
} pcpx_plane_params;

/* Host arithmetic only: how a call with `hypotheses` hypotheses and room for `rows_capacity` records (n under a NULL opt_rows) is
 * laid out.  The records are cut into *out_segments segments of *out_segment_rows consecutive records (a multiple of 256; the last
 * segment may be shorter; 0 and 0 when rows_capacity = 0), one wavefront per (64 consecutive hypotheses, segment); segments that
 * begin at or beyond the device's count do nothing.  flags: only PCPX_PLANE_NORMALS matters (32-byte records instead of 16).
 * max_planes: 0 for pcpx_plane_ransac, else that of pcpx_extract_planes (which keeps a second record buffer).  *out_scratch_bytes:
 * the device scratch the call takes from the device's pool.  Any output may be NULL.  The calls below use exactly this plan. */
int pcpx_plane_plan(uint64_t hypotheses, uint64_t rows_capacity, uint32_t flags, uint32_t max_planes, uint32_t* out_segments,
                    uint64_t* out_segment_rows, uint64_t* out_scratch_bytes);

/* Device arrays on `device` as above; d_out_found, d_opt_out_hypothesis, d_opt_out_score: one uint32_t each; d_opt_out_inliers: room
 * for rows_capacity (n under a NULL d_opt_rows) uint32_t, entries [0, *d_opt_out_inlier_count) are written; d_opt_out_inlier_count:
 * one uint64_t; d_opt_out_plane, d_opt_out_refit: 4 doubles each.  Fully enqueued on `stream`: no read-back and no synchronisation.
 * The scratch stays taken from the device's pool until the stream has passed the call, as in pcpx_register.h. */
int pcpx_plane_ransac_dev(const float* d_points, uint64_t n, const float* d_opt_normals, const uint32_t* d_opt_rows, uint64_t rows_capacity,
                          const uint64_t* d_opt_rows_count, const pcpx_plane_params* params, int device, void* stream, uint32_t* d_out_found,
                          uint32_t* d_opt_out_hypothesis, uint32_t* d_opt_out_score, uint32_t* d_opt_out_inliers,
                          uint64_t* d_opt_out_inlier_count, double* d_opt_out_plane, double* d_opt_out_refit);
/* the same with host arrays and a plain count; opt_out_inliers has room for rows_count (n under a NULL opt_rows) entries,
 * *opt_out_score of which are written */
int pcpx_plane_ransac(const float* points, uint64_t n, const float* opt_normals, const uint32_t* opt_rows, uint64_t rows_count,
                      const pcpx_plane_params* params, int device, uint32_t* out_found, uint32_t* opt_out_hypothesis, uint32_t* opt_out_score,
                      uint32_t* opt_out_inliers, double* opt_out_plane, double* opt_out_refit);

/* d_out_plane: 4 doubles; d_opt_out_rms: one double.  Fully enqueued on `stream`. */
int pcpx_plane_fit_dev(const float* d_points, uint64_t n, const uint32_t* d_opt_rows, uint64_t rows_capacity, const uint64_t* d_opt_rows_count,
                       int device, void* stream, double* d_out_plane, double* d_opt_out_rms);
/* the same with host arrays (opt_rows NULL: all n rows; not NULL with rows_count = 0: a list of no rows) */
int pcpx_plane_fit(const float* points, uint64_t n, const uint32_t* opt_rows, uint64_t rows_count, int device, double* out_plane,
                   double* opt_out_rms);

/* d_out_labels: n uint32_t; d_out_count: one uint32_t; d_opt_out_planes, d_opt_out_refits: max_planes x 4 doubles; d_opt_out_scores:
 * max_planes uint32_t.  Fully enqueued on `stream`. */
int pcpx_extract_planes_dev(const float* d_points, uint64_t n, const float* d_opt_normals, const pcpx_plane_params* params, int device,
                            void* stream, uint32_t* d_out_labels, uint32_t* d_out_count, double* d_opt_out_planes, double* d_opt_out_refits,
                            uint32_t* d_opt_out_scores);
/* the same with host arrays */
int pcpx_extract_planes(const float* points, uint64_t n, const float* opt_normals, const pcpx_plane_params* params, int device,
                        uint32_t* out_labels, uint32_t* out_count, double* opt_out_planes, double* opt_out_refits, uint32_t* opt_out_scores);

#ifdef __cplusplus
}
#endif
#endif /* PCPX_PLANES_H */
