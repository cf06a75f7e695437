/*
 * pcpx_objects.h -- objects from labels of libpcpx.so: what follows every call that ends in a label per row (pcpx_cluster_self,
 * pcpx_segment_self, pcpx_extract_planes, the `owner` outputs of pcpx_voxel_grid and pcpx_subsample_self).  The rows of every label
 * (PCL's std::vector<PointIndices>), its size, centroid, covariance, axis-aligned box and oriented box, and the
 * setMinClusterSize / setMaxClusterSize filter, with every bit of the result defined.
 *
 * A companion of pcpx.h with its conventions: POD arguments, pcpx_status codes, pcpx_last_error().  No pcpx_index is involved: the
 * entry point takes a device number and a stream like pcpx_voxel.h.  Every refusal comes before any device is touched.  The result
 * depends on the arguments alone: not on the launch order, not on the run.
 *
 * WHERE THE ARRAYS LIVE.  The call is declared once and params->flags says where its arrays are:
 *   PCPX_OBJECTS_ON_DEVICE   every array argument is a device pointer on `device`, owing its element type's alignment and no more.
 *                            Fully enqueued on `stream`: no read-back and no synchronisation.  The scratch stays taken from the
 *                            device's pool until the stream has passed the call, as in pcpx_voxel.h.
 *   without it               host arrays, staged around the same device path; the call returns when they are written.  `stream`
 *                            must be NULL.
 *   PCPX_OBJECTS_SKIP        rows whose label is params->none_label are not members (below).
 *   any other bit            PCPX_ERR_INVALID.
 *
 * INPUTS.  `points`: n x 3 float32, row-major and dense.  `labels`: n uint32_t.  n < 2^32 - 4096, the limit of pcpx_voxel.h.
 *
 * MEMBER.  A row is a member iff its three coordinates are finite and, under PCPX_OBJECTS_SKIP, its label != none_label.
 * PCPX_CLUSTER_NOISE, PCPX_VOXEL_NONE, PCPX_SUBSAMPLE_NONE and the "unlabelled" value of the segment and plane calls all go in
 * none_label.  Without the flag every label value is a label, 0xFFFFFFFF included.  The rows that are not members are counted in
 * the optional output `skipped`.
 *
 * SEGMENTS.  The distinct labels among the members, in ASCENDING LABEL order; within a segment the members r_0 < r_1 < ... <
 * r_(c-1) in ascending row order (one stable sort of label << 32 | row on its upper half gives this order).  A segment of c
 * members is an OBJECT iff min_size <= c and (max_size == 0 or c <= max_size).  The objects are numbered 0 .. S - 1 in label
 * order; S is one uint64_t and always written.
 *
 * SUMS.  Every sum below is float64 with no FMA, in a FIXED 64-ARY TREE over the members in member order:
 *     level 0   chunk j holds the terms [64 j, min(64 j + 64, c)):  P0_j = (...((x_(64 j) + x_(64 j + 1)) + ...)  in order, starting
 *               from its first term, not from zero
 *     level l   P(l)_j = (...((P(l-1)_(64 j) + P(l-1)_(64 j + 1)) + ...) over the at most 64 partial sums of the level below, in order
 *     T         the one sum that is left when a level has one chunk (for c <= 64: the plain sequential sum)
 * No thread adds more than 64 terms in a row, whatever share of the cloud one segment holds: with labels, one segment holding 40 %
 * of a 10 M-point scan is the normal case.  This bound is why the order differs from pcpx_voxel.h, whose two levels let one thread
 * add 64 + ceil(c / 64) terms in a row (6 * 10^4 of them for such a segment).  For c <= 4096 the two orders are the same.
 *
 * CENTROID.  T_a the tree sum of double(p_a) over the members; m_a = T_a / double(c), output as float64 (float32 would lose the
 * offsets of a georeferenced cloud).
 *
 * COVARIANCE.  d_a = double(p_a) - m_a; the six products d_a * d_b, each rounded on its own, summed in the same tree and divided by
 * double(c), in the order xx, xy, xz, yy, yz, zz.
 *
 * AABB.  Per axis the minimum and the maximum of the members' float32 coordinates, compared as the ordered integers of the bit
 * patterns (as pcpx_voxel.h's origin: -0 is below +0, the result is one defined bit pattern): lo x, y, z, then hi x, y, z.
 *
 * ORIENTED BOX.  The eigenvectors of the covariance by cyclic Jacobi sweeps in float64, one thread per object (they are NOT defined
 * to the bit: compare them by what they span).  The axes are ordered by descending eigenvalue, the first of equal ones first.  e0
 * and e1 are normalised and signed so that their component of largest magnitude is positive (the lowest index on ties); e2 = e0 x e1,
 * each component two products and one subtraction (e2x = e0y e1z - e0z e1y, e2y = e0z e1x - e0x e1z, e2z = e0x e1y - e0y e1x).  A
 * covariance with a term that is not finite gets the identity axes (no finite float32 input gives one: the squares of float32
 * differences do not overflow float64).  GIVEN THE AXES, everything else is defined to the bit, float64, no FMA:
 *     t_k    = ((d_x e_kx + d_y e_ky) + d_z e_kz) + 0.0            per member (the last addition makes a zero +0)
 *     lo_k   = the minimum, hi_k = the maximum of t_k over the members (they commute: any order gives the same bits)
 *     half_k = (hi_k - lo_k) / 2
 *     c_k    = (lo_k + hi_k) / 2
 *     centre_a = ((m_a + c_0 e_0a) + c_1 e_1a) + c_2 e_2a
 * One object's 15 doubles: centre 3, the axes 9 row-major (e0, e1, e2), half 3.
 *
 * OUTPUTS, all optional but the count.  The per-object arrays have room for `capacity` objects (out_offsets for capacity + 1
 * entries), object o at entry o; the per-row arrays have n entries.
 *     out_labels         S uint32_t, ascending
 *     out_counts         S uint32_t, c
 *     out_first_row      S uint32_t, r_0
 *     out_offsets        S + 1 uint32_t: offsets[o] = the members of the objects before o (CSR)
 *     out_rows           n uint32_t: the member rows grouped by object, object o's at [offsets[o], offsets[o + 1]) in ascending row
 *                        order; [0, offsets[S]) is written
 *     out_centroid       S x 3 float64
 *     out_cov            S x 6 float64
 *     out_aabb           S x 6 float32
 *     out_obb            S x 15 float64
 *     out_object_of_row  n uint32_t: the object of every row, PCPX_OBJECTS_NONE for a row that is not a member and for a member of a
 *                        segment that is not an object; written for all n rows whatever the capacity
 *     out_skipped        one uint64_t
 * CAPACITY as in pcpx_voxel_grid.  The host form sets *out_count always; when capacity < S it returns PCPX_ERR_CAPACITY and writes
 * nothing else.  The device form writes the first min(S, capacity) objects of every per-object output, offsets[0 .. min(S, capacity)]
 * and the rows of those objects, [0, offsets[min(S, capacity)]); the caller compares the count with its capacity.
 * n = 0 and "no member" are valid: S = 0, offsets[0] = 0, skipped = n.
 *
 * PCPX_ERR_INVALID, before any device is touched: a NULL points or labels with n > 0; a NULL params or count; min_size == 0;
 * max_size nonzero and below min_size; an unknown flag bit; reserved != 0; n >= 2^32 - 4096; a non-NULL stream without
 * PCPX_OBJECTS_ON_DEVICE.
 */
#ifndef PCPX_OBJECTS_H
#define PCPX_OBJECTS_H

#include "pcpx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCPX_OBJECTS_ON_DEVICE 1u      /* every array is a device pointer; enqueued on `stream` */
#define PCPX_OBJECTS_SKIP 2u           /* rows labelled params->none_label are not members */
#define PCPX_OBJECTS_NONE 0xFFFFFFFFu  /* the object of a row that is in none */
#define PCPX_OBJECTS_CHUNK 64u         /* the tree's fan-in */

typedef struct pcpx_objects_params {
    uint32_t flags;      /* PCPX_OBJECTS_ON_DEVICE | PCPX_OBJECTS_SKIP */
    uint32_t none_label; /* read under PCPX_OBJECTS_SKIP */
    uint32_t min_size;   /* at least 1 */
    uint32_t max_size;   /* 0: no upper bound */
    uint32_t reserved;   /* 0 */
} pcpx_objects_params;

/* Host arithmetic only: the device scratch that a call over n rows with room for `capacity` objects takes from the device's pool
 * (the sort's workspace is part of it: *opt_out_sort_bytes).  The capacity counts up to n.  Either output may be NULL.  The call
 * below uses exactly this plan. */
int pcpx_objects_plan(uint64_t n, uint64_t capacity, uint64_t* opt_out_sort_bytes, uint64_t* opt_out_scratch_bytes);

int pcpx_label_objects(const float* points, const uint32_t* labels, uint64_t n, const pcpx_objects_params* params, uint64_t capacity,
                       int device, void* stream, uint64_t* out_count, uint32_t* opt_out_labels, uint32_t* opt_out_counts,
                       uint32_t* opt_out_first_row, uint32_t* opt_out_offsets, uint32_t* opt_out_rows, double* opt_out_centroid,
                       double* opt_out_cov, float* opt_out_aabb, double* opt_out_obb, uint32_t* opt_out_object_of_row,
                       uint64_t* opt_out_skipped);

#ifdef __cplusplus
}
#endif
#endif /* PCPX_OBJECTS_H */
