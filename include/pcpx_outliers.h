/*
 * pcpx_outliers.h -- outlier removal of libpcpx.so: the cloud's resolution (the mean over the cloud of the mean distance to the k
 * nearest neighbours), the statistical filter on it (PCL's StatisticalOutlierRemoval, Open3D's remove_statistical_outlier), the
 * radius filter (a sphere must hold at least so many points) and the density filter of the reference's
 * examples/filter_point_cloud_noise_by_density.cpp (the radius filter at a multiple of the resolution) -- each as ONE call that is
 * enqueued from its first kernel to its last: neither the mean, the threshold nor the radius visits the host on the way.
 *
 * A companion of pcpx.h with its conventions: POD arguments, pcpx_status codes, pcpx_last_error(); a rank-local (shard) handle
 * is refused with PCPX_ERR_UNSUPPORTED.  An empty cloud is fine (count 0, stats NaN, NaN, NaN, 0).
 *
 * WHERE THE ARRAYS LIVE.  Every call is declared once and takes `flags`:
 *   PCPX_OUTLIERS_ON_DEVICE   every array argument (stats included) is a device pointer, owing its element type's alignment and no
 *                             more.  Fully enqueued on the handle's stream: no read-back, no synchronisation
 *                             (pcpx_index_synchronize waits for it).  Scratch is the handle's.
 *   0                         host arrays; the call returns when they are written (staged around the same device path).
 *   any other bit             PCPX_ERR_INVALID.
 *
 * THE CONTRACT is exact and does not depend on the tree, the voxel grid, the launch order or the run.
 *   d_i      for an indexed row (a point inside the index's voxel grid) the bits that pcpx_neighbourhoods_self_dev writes as the mean
 *            distance at (k, eps): the neighbours ascending in (d2, index) with the eps-box excluded, the float32 sum of sqrtf(d2)
 *            in that order, divided by the number found; NaN where nothing is found.  k <= 32: the fused epilogue of the kNN kernel,
 *            no rows written.  k > 32 (PCL's default is 50): the multi-pass path, with the rows and their counts in the handle's
 *            scratch -- n_in (k + 1) 4 bytes.
 *   usable   a row is usable iff it is indexed and d_i is finite; m = the number of usable rows.
 *   S1       = sum of (double)d_i over the usable rows, the input rows 0 .. n_in - 1 being the items of the library's one fixed
 *            summation order (an item's thread adds its items ascending, 64 x 256 apart; a block's 256 threads by a tree with
 *            offsets 128 .. 1; the 64 blocks in block order).  An unusable row adds nothing.
 *   mean     = S1 / m.
 *   S2       = sum of e e with e = (double)d_i - mean, a second sum in the same order: one rounding each for e, the product and
 *            the add (no FMA).
 *   std      = sqrt(S2 / (m - 1)) for m >= 2, 0 for m = 1; for m = 0 mean and std are NaN.  The two-pass sample deviation on
 *            purpose: the one-pass sq_sum - sum^2 / n cancels on clouds far from unit scale.
 *   stats    4 doubles {mean, std, cut, usable = (double)m}; cut is the float32 value below, widened.
 * STATISTICAL FILTER.  cut = (float)(mean + (double)std_ratio * std): one rounding for the product, one for the sum, then round
 *   to nearest even.  keep_i = usable_i && d_i <= cut, compared in float32.  m = 0 keeps nothing.  A NaN or infinite std_ratio is
 *   PCPX_ERR_INVALID; a negative one is allowed.
 * RADIUS FILTER.  count_i by the rule of pcpx_range_count_* (d2 <= r * r in float32, centre included, only indexed points
 *   counted); keep_i = indexed_i && count_i >= max(min_neighbours, 1) -- the reference example's
 *   `range_search(ball).size() < at_least -> dropped`.  radius < 0 or NaN is PCPX_ERR_INVALID.
 * DENSITY FILTER.  r = (float)((double)radius_scale * mean) with the mean of the resolution at (k, eps), then the radius filter at
 *   r; cut = r.  (The reference leaves the order of its std::reduce(par) open: any fixed order is within its semantics.)  A NaN r
 *   (m = 0) keeps nothing.  radius_scale < 0 or not finite is PCPX_ERR_INVALID.  The sphere walk reads r from a device word.
 *
 * THE ARRAYS.  keep: n_in rows, every row written, 1 = kept (required: NULL is PCPX_ERR_INVALID).  opt_kept_rows: room for n_in
 * entries; the kept input indices, ascending; only [0, count) are written.  opt_kept_count: one uint64_t.  opt_mean_dist, opt_count:
 * n_in entries, every row written -- for a row outside the voxel grid opt_mean_dist is NaN and opt_count is 0.  k = 0 is
 * PCPX_ERR_INVALID.
 */
#ifndef PCPX_OUTLIERS_H
#define PCPX_OUTLIERS_H

#include "pcpx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCPX_OUTLIERS_ON_DEVICE 1u

/* stats (required): 4 doubles {mean, std, NaN (there is no cut), usable} */
int pcpx_outliers_resolution_self(pcpx_index* idx, uint32_t k, float eps, uint32_t flags, float* opt_mean_dist, double* stats);

int pcpx_outliers_statistical_self(pcpx_index* idx, uint32_t k, float eps, float std_ratio, uint32_t flags, uint8_t* keep,
                                   uint32_t* opt_kept_rows, uint64_t* opt_kept_count, float* opt_mean_dist, double* opt_stats);

/* With opt_count NULL the sphere walk stops a point at the bound (the at-least form); the keep mask is the same by construction. */
int pcpx_outliers_radius_self(pcpx_index* idx, float radius, uint32_t min_neighbours, uint32_t flags, uint8_t* keep,
                              uint32_t* opt_kept_rows, uint64_t* opt_kept_count, uint32_t* opt_count);

int pcpx_outliers_density_self(pcpx_index* idx, uint32_t k, float eps, float radius_scale, uint32_t min_neighbours, uint32_t flags,
                               uint8_t* keep, uint32_t* opt_kept_rows, uint64_t* opt_kept_count, uint32_t* opt_count, double* opt_stats);

#ifdef __cplusplus
}
#endif
#endif /* PCPX_OUTLIERS_H */
