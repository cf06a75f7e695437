/*
 * pcpx_fps.h -- farthest point sampling of libpcpx.so: exactly m points of the indexed cloud that cover it as evenly as a greedy
 * choice can (Gonzalez 1985; Open3D's farthest_point_down_sample, the sampling layer of PointNet++).  Every sample is the point
 * farthest from the samples taken so far.  The index prunes the work: a new sample can only lower the distances in a bucket of
 * leaf slots whose tight box is nearer to it than the bucket's largest distance, so a sample looks at every bucket's box and at
 * the points of a few buckets.
 *
 * A companion of pcpx.h with its conventions: POD arguments, pcpx_status codes, pcpx_last_error(); a rank-local (shard) handle
 * is refused with PCPX_ERR_UNSUPPORTED.  An empty cloud and m = 0 are fine (count 0).
 *
 * WHERE THE ARRAYS LIVE.  The call is declared once and takes params->flags:
 *   PCPX_FPS_ON_DEVICE   every array argument, out_count and opt_out_evaluations included, is a device pointer, owing its element
 *                        type's alignment and no more.  Fully enqueued on the handle's stream: min(m, indexed points) launches and
 *                        a constant few more (one launch in all for a cloud of up to 8192 leaf slots), a number known on the
 *                        host; the stop rule below is applied on the device, so there is no read-back and no synchronisation
 *                        between samples (pcpx_index_synchronize waits for the call).  QUEUE LIMIT: the call returns without waiting only as far as the runtime's queue takes that
 *                        many launches; beyond that the enqueueing thread waits for the device to catch up.  Scratch is the
 *                        handle's.  Under pcpx_profile_begin/end the call is booked as ONE interval of the PCPX_K_RANGE family.
 *   0                    host arrays; the call returns when they are written (staged around the same device path).
 *   any other bit        PCPX_ERR_INVALID.
 *
 * THE CONTRACT is exact and depends on the cloud and the arguments alone: not on the tree, the voxel grid's resolution, the
 * launch order or the run.  All arithmetic is float32, one rounding per operation, no FMA.
 *   setting   I = the indexed rows: the rows inside the index's voxel grid.  A row with a non-finite coordinate is never in I.
 *             d2(i, j) = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)), dx = fl(x_i - x_j): the rule of pcpx_range_count_*.  It is
 *             symmetric, and on I it may be +inf and is never NaN.
 *   start     D_0(i) = +inf for every i in I.  s_0 = params->start if that row is in I; with start = PCPX_FPS_START_LOWEST, the
 *             lowest row of I.  A start < n_in that is not in I selects nothing: count 0, in both forms (the device form cannot
 *             refuse on data).
 *   step      after sample s_t is taken, D_{t+1}(i) = min(D_t(i), d2(i, s_t)), and owner(i) = t whenever d2(i, s_t) < D_t(i):
 *             the comparison is strict, so the EARLIEST sample wins a tie.
 *   next      s_{t+1} = the row of I with the largest D_{t+1}; among equal values the LOWEST input index.
 *   stop      s_{t+1} is taken iff t + 1 < m and D_{t+1}(s_{t+1}) > stop2, stop2 = fl(stop_radius stop_radius).  Otherwise the
 *             selection ends with count = t + 1.  With stop_radius = 0 it ends when every indexed point coincides with a sample:
 *             a duplicate of a sample is never selected, and m larger than the number of distinct points is fine.
 * WHAT IT GUARANTEES.  With stop_radius = r > 0 and count < m: every indexed point has a sample with d2 <= stop2 (a covering),
 * and any two samples have d2 > stop2 (a packing).  In any case out_d2 never increases: D_t(s_t) is the covering radius, squared,
 * of the first t samples.
 *
 * THE ARRAYS.  out_rows: m entries, [0, count) written, the samples in selection order (required when m > 0).  out_count: one
 * uint64_t (required).  opt_out_d2: m floats, [0, count) written, out_d2[t] = D_t(s_t); the first is +inf.  opt_out_min_d2: n_in
 * floats, every row written: D_count(i), +inf for a row not in I or when count is 0.  opt_out_owner: n_in entries, every row
 * written: the ordinal t of the row's owner, PCPX_FPS_NONE for a row not in I or when count is 0.
 * opt_out_evaluations: one uint64_t, a DIAGNOSTIC of how the work was done and NOT part of the contract: the number of d2 values
 * formed over the call.  A sample forms one for every leaf slot of every bucket it updates, the empty slots at the end of the last
 * leaf included; with the switch "fps_prune" = 0 (pcpx_debug_set), and in the one-launch form that a cloud of up to 8192 leaf slots
 * takes ("fps_one_block"), which looks at every slot for every sample, that is 8 ceil(|I| / 8) count.
 *
 * NULL params, NULL out_count, NULL out_rows with m > 0, stop_radius < 0 or NaN, an unknown flag bit, reserved != 0 and a
 * start >= n_in other than PCPX_FPS_START_LOWEST are PCPX_ERR_INVALID, before any device is touched.
 */
#ifndef PCPX_FPS_H
#define PCPX_FPS_H

#include "pcpx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCPX_FPS_ON_DEVICE 1u
#define PCPX_FPS_NONE 0xFFFFFFFFu
#define PCPX_FPS_START_LOWEST 0xFFFFFFFFu

typedef struct pcpx_fps_params {
    uint32_t flags;
    uint32_t start;      /* an input row, or PCPX_FPS_START_LOWEST */
    float stop_radius;   /* 0: no stop before m samples or the last distinct point */
    uint32_t reserved;   /* 0 */
} pcpx_fps_params;

int pcpx_farthest_points_self(pcpx_index* idx, uint64_t m, const pcpx_fps_params* params, uint32_t* out_rows, uint64_t* out_count,
                              float* opt_out_d2, float* opt_out_min_d2, uint32_t* opt_out_owner, uint64_t* opt_out_evaluations);

#ifdef __cplusplus
}
#endif
#endif /* PCPX_FPS_H */
