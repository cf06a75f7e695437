/*
 * pcpx_voxel.h -- voxel-grid downsampling of libpcpx.so: the points of every occupied cell of a regular grid replaced by their
 * centroid (PCL's VoxelGrid, Open3D's voxel_down_sample), attributes averaged with them, every bit of the result defined.
 *
 * A companion of pcpx.h with its conventions: POD arguments, pcpx_status codes, pcpx_last_error().  No pcpx_index is involved: the
 * entry points take a device number (and the _dev form a stream) like pcpx_planes.h.  The _dev form never synchronises and reads
 * nothing back.  Every refusal comes before any device is touched.  The result depends on the arguments alone: not on the launch
 * order, not on the run.
 *
 * INPUTS.  `points`: n x 3 float32, row-major and dense, n < 2^32 - 4096.  `opt_attrs`: n x A float32 with A = params->attr_columns
 * in 0 .. PCPX_VOXEL_ATTRS_MAX (colours, normals, intensities), or NULL with A = 0.  A row is USABLE iff its three coordinates are
 * finite; attributes play no part in that.
 *
 * ORIGIN.  With PCPX_VOXEL_ORIGIN, params->origin as given.  Without it, per axis the minimum over the usable rows, compared as the
 * ordered integers of the bit patterns (so -0 is below +0, and the result is one defined bit pattern); (0, 0, 0) with no usable
 * row.  The origin used is an optional output of 3 floats.
 *
 * CELL.  Per axis a, in float32, every operation rounded on its own:
 *     t = p_a - o_a
 *     q = t / leaf_a          (a correctly rounded division, not a multiplication by a reciprocal: a point at exactly o + k * leaf
 *                              with k * leaf representable is in cell k)
 *     c_a = floor(q)
 * The row is INDEXED iff it is usable and 0 <= q_a < 2^21 on every axis, as float comparisons: an inf from the subtraction, or a
 * negative cell under an explicit origin, drops the row, and nothing else does.  key = c_z * 2^42 + c_y * 2^21 + c_x.  The number
 * of rows that are not indexed is the optional output `dropped`.
 *
 * VOXELS.  The distinct keys of the indexed rows in ASCENDING KEY order; V is their number, one uint64_t, always written.
 *
 * SUMS.  For voxel v with members r_0 < r_1 < ... < r_(c-1) (ascending input row) and each column (x, y, z, then each attribute),
 * everything float64 with no FMA:
 *     chunk j holds members [64 j, min(64 j + 64, c))
 *     S_j = (...((double(x_(64 j)) + double(x_(64 j + 1))) + ...)          in member order
 *     T   = S_0, then T = T + S_j for j = 1, 2, ... in order
 *     out = float(T / double(c))                                          one rounding to float32
 * For c <= 64 this is the plain sequential sum.  A NaN or inf attribute propagates as IEEE 754 says (a NaN result is a NaN; which
 * NaN is not defined).  The two levels are part of the contract so that no thread adds more than 64 + ceil(c / 64) terms in a row,
 * whatever share of the cloud one voxel holds.
 *
 * OUTPUTS, all optional but the count, each with room for `capacity` voxels, voxel v at entry v:
 *     out_xyz     V x 3 float32, the centroids
 *     out_attrs   V x A float32, the attribute means
 *     out_counts  V uint32_t, c
 *     out_keys    V uint64_t
 *     out_rows    V uint32_t: the member nearest the float32 centroid, the one of smallest (bits(d2) << 32 | row) with
 *                 d2 = (dx*dx + dy*dy) + dz*dz in float32, dx = p_x - centroid_x, every operation rounded on its own -- the subset
 *                 form, for callers who must keep measured points
 *     out_owner   n uint32_t: an indexed row's voxel v, PCPX_VOXEL_NONE otherwise; written for all n rows whatever the capacity
 * The host form sets *out_count always; when out_xyz is NULL or capacity < V it returns PCPX_ERR_CAPACITY and writes nothing else
 * (pcpx_hierarchy_simplification's sizing call).  The _dev form writes the first min(V, capacity) voxels of every per-voxel output;
 * the caller compares the count with its capacity.  n = 0 is valid: V = 0 and nothing else is written.
 *
 * PCPX_ERR_INVALID, before any device is touched: a NULL points with n > 0; a NULL params or count; a leaf that is <= 0, NaN or
 * inf; a non-finite origin under its flag; attr_columns above PCPX_VOXEL_ATTRS_MAX, or above 0 with NULL attrs (whatever n), or an
 * attrs output without attrs; an unknown flag bit; reserved != 0; n >= 2^32 - 4096.
 */
#ifndef PCPX_VOXEL_H
#define PCPX_VOXEL_H

#include "pcpx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCPX_VOXEL_ORIGIN 1u            /* params->origin is the grid's origin */
#define PCPX_VOXEL_NONE 0xFFFFFFFFu     /* the owner of a row that is not indexed */
#define PCPX_VOXEL_ATTRS_MAX 16u
#define PCPX_VOXEL_CELLS_PER_AXIS 2097152u /* 2^21 */

typedef struct pcpx_voxel_params {
    float leaf[3];         /* the cell's edges, each finite and > 0 */
    float origin[3];       /* read under PCPX_VOXEL_ORIGIN */
    uint32_t flags;        /* PCPX_VOXEL_ORIGIN */
    uint32_t attr_columns; /* A, 0 .. PCPX_VOXEL_ATTRS_MAX */
    uint32_t reserved;     /* 0 */
} pcpx_voxel_params;

/* Host arithmetic only: the device scratch that a call over n rows with room for `capacity` voxels takes from the device's pool
 * (the sort's workspace is part of it: *opt_out_sort_bytes).  The capacity counts up to n; the host form's is its own when out_xyz
 * is given, else 0.  Either output may be NULL.  The calls below use exactly this plan. */
int pcpx_voxel_plan(uint64_t n, uint64_t capacity, uint64_t* opt_out_sort_bytes, uint64_t* opt_out_scratch_bytes);

/* Device arrays on `device` as above; d_out_count, d_opt_out_dropped: one uint64_t each; d_opt_out_origin: 3 floats.  Fully enqueued
 * on `stream`: no read-back and no synchronisation.  The scratch stays taken from the device's pool until the stream has passed the
 * call, as in pcpx_register.h. */
int pcpx_voxel_grid_dev(const float* d_points, uint64_t n, const float* d_opt_attrs, const pcpx_voxel_params* params, uint64_t capacity,
                        int device, void* stream, uint64_t* d_out_count, float* d_opt_out_xyz, float* d_opt_out_attrs,
                        uint32_t* d_opt_out_counts, uint64_t* d_opt_out_keys, uint32_t* d_opt_out_rows, uint32_t* d_opt_out_owner,
                        uint64_t* d_opt_out_dropped, float* d_opt_out_origin);
/* the same with host arrays */
int pcpx_voxel_grid(const float* points, uint64_t n, const float* opt_attrs, const pcpx_voxel_params* params, uint64_t capacity, int device,
                    uint64_t* out_count, float* opt_out_xyz, float* opt_out_attrs, uint32_t* opt_out_counts, uint64_t* opt_out_keys,
                    uint32_t* opt_out_rows, uint32_t* opt_out_owner, uint64_t* opt_out_dropped, float* opt_out_origin);

#ifdef __cplusplus
}
#endif
#endif /* PCPX_VOXEL_H */
