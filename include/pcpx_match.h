/*
 * pcpx_match.h -- descriptor matching of libpcpx.so: for every row of one set of descriptors the exact nearest and second nearest
 * row of another set, by brute force over all pairs, and the correspondences that pass Lowe's ratio test and the mutual test.
 *
 * A companion of pcpx.h with its conventions: POD arguments, pcpx_status codes, pcpx_last_error().  No pcpx_index is involved: the
 * entry points take a device number (and the _dev forms a stream) like pcpx_hierarchy_simplification_dev.
 *
 * INPUTS.  `src`: m x dims float32.  `tgt`: n x dims float32.  Both row-major and dense.  1 <= dims <= PCPX_MATCH_MAX_DIMS.
 * m, n < 2^32 - 1.  m = 0 or n = 0 is fine.
 *
 * DISTANCE of source row s and target row t.  float32, every operation rounded on its own (no FMA), in bin order:
 *     e_b = s_b - t_b
 *     d2  = ((e_0*e_0 + e_1*e_1) + e_2*e_2) + ...
 * the arithmetic of the kNN kernels and of pcpx_kd_knn_batch, so d2(s, t) and d2(t, s) are the same bits.  A pair whose d2 is NaN
 * is skipped; +inf is an ordinary value.
 *
 * ORDER.  The pairs of one source are ordered by the key (d2 bits, target index) -- d2 is never negative, so its bits order as an
 * unsigned integer -- the total order of pcpx_kd_knn_batch.  BEST is the smallest key, SECOND the smallest key among the other
 * targets (its d2 may equal best's).
 *
 * PCPX_MATCH_SKIP_ZERO_ROWS.  A row all of whose entries are +0 or -0 takes no part, on either side: a descriptor that could not
 * be computed is written as zeros (pcpx_fpfh_self), and zero <-> zero would be a perfect false match.
 *
 * NEAREST.  Per source row: out_idx = best's target index, or PCPX_MATCH_NONE when no target qualifies; opt_out_d2 = best's d2, or
 * +inf; opt_out_second_idx and opt_out_second_d2 = second's, or PCPX_MATCH_NONE and +inf when fewer than two targets qualify.
 * Every row of every array given is written.
 *
 * CORRESPONDENCES.  Source i is kept iff
 *     it has a best j, and
 *     d2_best <= max_ratio_sq * d2_second        (one float32 product, one comparison; a NaN compares false: Lowe's test on squared
 *                                                 distances; max_ratio_sq = 1 is no test, second = +inf passes unless max_ratio_sq = 0)
 *     and, with PCPX_MATCH_MUTUAL, the best SOURCE of target j -- over all sources, by the same rule with the source index as the
 *     tie-break -- is i.
 * The kept (i, j) are written as pairs of uint32_t, ascending i, into an array with room for m pairs; optionally their d2; and
 * their number into one uint64_t.
 *
 * PADDING.  Rows are copied into records of a compiled width W >= dims (pcpx_match_plan reports it), the tail zero.  That is exact:
 * (0 - 0)^2 = +0, and acc + (+0) leaves every bit of a non-negative (or infinite) acc as it was.
 *
 * PCPX_ERR_INVALID: dims = 0 or > PCPX_MATCH_MAX_DIMS; m or n >= 2^32 - 1; a NULL src with m > 0, tgt with n > 0, out_idx or
 * out_pairs with m > 0; an unknown flag bit (PCPX_MATCH_MUTUAL is unknown to the nearest calls); max_ratio_sq outside [0, 1] or
 * NaN; a NULL count in the host form.  All of these are checked before any device is touched.
 */
#ifndef PCPX_MATCH_H
#define PCPX_MATCH_H

#include "pcpx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCPX_MATCH_MAX_DIMS 64
#define PCPX_MATCH_NONE 0xFFFFFFFFu
#define PCPX_MATCH_SKIP_ZERO_ROWS 1u
#define PCPX_MATCH_MUTUAL 2u

/* Host arithmetic only: how a call on m sources, n targets and `dims` columns is laid out.  *out_width: the record width W;
 * *out_segments, *out_segment_rows: the targets are cut into that many segments of that many consecutive rows (the last one may be
 * shorter; 0 and 0 when n = 0), one wavefront per (64 consecutive sources, segment); *out_scratch_bytes: the device scratch that
 * every call of this header takes from the device's pool for these sizes (the records of both sets, the per-segment keys of
 * both directions, the compaction's arrays).  Any output may be NULL.  The calls below use exactly this plan. */
int pcpx_match_plan(uint64_t m, uint64_t n, uint32_t dims, uint32_t* out_width, uint32_t* out_segments, uint64_t* out_segment_rows,
                    uint64_t* out_scratch_bytes);

/* Device arrays on `device`: d_src (m x dims), d_tgt (n x dims), d_out_idx (m uint32_t), d_opt_out_d2, d_opt_out_second_d2 (m
 * floats), d_opt_out_second_idx (m uint32_t).  flags: PCPX_MATCH_SKIP_ZERO_ROWS or 0.  Fully enqueued on `stream`: no read-back and
 * no synchronisation.  The scratch stays taken from the device's pool until the stream has passed the call (looked at by later
 * calls of this header), so calls on different streams do not share it. */
int pcpx_match_nearest_dev(const float* d_src, uint64_t m, const float* d_tgt, uint64_t n, uint32_t dims, uint32_t flags, int device,
                           void* stream, uint32_t* d_out_idx, float* d_opt_out_d2, uint32_t* d_opt_out_second_idx,
                           float* d_opt_out_second_d2);
/* the same with host arrays */
int pcpx_match_nearest(const float* src, uint64_t m, const float* tgt, uint64_t n, uint32_t dims, uint32_t flags, int device,
                       uint32_t* out_idx, float* opt_out_d2, uint32_t* opt_out_second_idx, float* opt_out_second_d2);

/* Device arrays: d_out_pairs (room for m pairs {source, target}), d_opt_out_d2 (room for m floats), d_opt_out_count (one uint64_t):
 * entries [0, count) of the first two are written.  flags: PCPX_MATCH_SKIP_ZERO_ROWS | PCPX_MATCH_MUTUAL.  Fully enqueued on
 * `stream`, as the call above: the count stays on the device. */
int pcpx_match_correspondences_dev(const float* d_src, uint64_t m, const float* d_tgt, uint64_t n, uint32_t dims, float max_ratio_sq,
                                   uint32_t flags, int device, void* stream, uint32_t* d_out_pairs, float* d_opt_out_d2,
                                   uint64_t* d_opt_out_count);
/* the same with host arrays; *out_count pairs are written */
int pcpx_match_correspondences(const float* src, uint64_t m, const float* tgt, uint64_t n, uint32_t dims, float max_ratio_sq, uint32_t flags,
                               int device, uint32_t* out_pairs, float* opt_out_d2, uint64_t* out_count);

#ifdef __cplusplus
}
#endif
#endif /* PCPX_MATCH_H */
