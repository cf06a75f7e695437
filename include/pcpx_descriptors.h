/*
 * pcpx_descriptors.h -- descriptors of libpcpx.so: the Fast Point Feature Histogram (Rusu, Blodow, Beetz 2009) of the indexed
 * cloud's points, or of a subset of them, over a radius, in two walks of the index and without materialising the neighbour lists.
 *
 * A companion of pcpx.h with its conventions: POD arguments, pcpx_status codes, pcpx_last_error(); a rank-local (shard) handle
 * is refused with PCPX_ERR_UNSUPPORTED.
 *
 * INPUTS.  `normals`: three float32 per input row, used as given (orientation is the caller's business: the histograms of a
 * surface depend on which way its normals point).  `rows`: m DISTINCT input indices to describe (m = 0: nobody), or NULL with
 * m = 0 for every input row.
 *
 * SPHERE.  j is in i's sphere iff d2 <= r*r by the rule of pcpx_range_count_* (d = p_j - p_i, float32, three roundings, no FMA);
 * only points inside the index's voxel grid are in any sphere.  A PAIR (i, j) is a j in i's sphere with j != i.
 *
 * PAIR FEATURE of (i, j).  Every line is one float32 statement, every operation rounded on its own (no FMA), evaluated left to
 * right with the brackets as written; sqrt and / are the correctly rounded ones.  p, n: coordinates and normal.
 *     dx = xj - xi;  dy = yj - yi;  dz = zj - zi
 *     d2 = (dx*dx + dy*dy) + dz*dz                              skip the pair if d2 == 0
 *     ai = (nix*dx + niy*dy) + niz*dz
 *     aj = (njx*dx + njy*dy) + njz*dz
 *     if |ai| < |aj|:  s = j, t = i, (ex, ey, ez) = (-dx, -dy, -dz), a = -aj       (the source is the end whose normal makes the
 *     else:            s = i, t = j, (ex, ey, ez) = ( dx,  dy,  dz), a =  ai        smaller angle with the line; a NaN compares false)
 *     f3 = a / sqrt(d2)
 *     vx = ey*nsz - ez*nsy;  vy = ez*nsx - ex*nsz;  vz = ex*nsy - ey*nsx           (v_raw = e x n_s)
 *     vv = (vx*vx + vy*vy) + vz*vz                              skip the pair if vv == 0
 *     vl = sqrt(vv)
 *     f2 = ((vx*ntx + vy*nty) + vz*ntz) / vl
 *     wx = nsy*vz - nsz*vy;  wy = nsz*vx - nsx*vz;  wz = nsx*vy - nsy*vx           (n_s x v_raw)
 *     y  = (wx*ntx + wy*nty) + wz*ntz                           (theta = atan2(y, x): both carry the factor |v_raw|)
 *     x  = ((nsx*ntx + nsy*nty) + nsz*ntz) * vl
 *     skip the pair if f3, f2, x or y is NaN
 * Two square roots and two divisions per pair.  Non-unit normals are not an error: the features are then whatever these lines give.
 *
 * BINS, 11 per feature.
 *     b3 = trunc(min(max((f3 + 1) * 5.5, 0), 10))               (= clamp(floor(11 (f3 + 1) / 2), 0, 10); 5.5 t and 11 t / 2 round alike)
 *     b2 likewise from f2
 *     b1 = 5 + k if y >= 0 (so for -0 too), 5 - k otherwise, with k = #{i in 0..4 : PCPX_FPFH_COS[i] * |y| - PCPX_FPFH_SIN[i] * x >= 0}
 *          (two products and one difference, each rounded): the place of theta among 11 equal sectors of [-pi, pi] without a
 *          transcendental -- theta >= k pi / 11 iff sin(theta - k pi / 11) >= 0.  x = y = 0 gives k = 5.
 *
 * SPFH.  count_i[33], integers, over i's pairs that are not skipped: feature 1 in bins 0-10, feature 2 in 11-21, feature 3 in
 * 22-32; pairs_i their number; spfh_i[b] = (100 * (float)count_i[b]) / (float)pairs_i, and 0 when pairs_i = 0.  Integer counts make
 * this exact and independent of the order of the walk.
 *
 * FPFH.  T_i[b] = sum over j in i's sphere with d2 > 0 of spfh_j[b] * (1 / d2): weight one over the squared distance, the centre
 * and its exact copies left out.  Each block of 11 bins is scaled to sum 100: fpfh_i[b] = T_i[b] * (100 / S), S the block's sum in
 * bin order; all 0 when S = 0.  The order of the sum over j is not part of the contract; float32 throughout.
 *
 * A row outside the voxel grid, or an entry of `rows` that is >= n_in, gets 33 zeros (and pairs = 0).  Radius 0 gives zeros.
 *
 * radius < 0 or NaN, NULL normals, a NULL fpfh array, rows NULL with m > 0 or flags != 0 are PCPX_ERR_INVALID.  An empty cloud is
 * fine.
 */
#ifndef PCPX_DESCRIPTORS_H
#define PCPX_DESCRIPTORS_H

#include "pcpx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCPX_FPFH_BINS 11
#define PCPX_FPFH_SIZE 33

/* float32(cos, sin)(k pi / 11) for k = 1, 3, 5, 7, 9, the sector edges of theta (exact float32 values, written in hexadecimal):
 * PCPX_FPFH_COS[i] and PCPX_FPFH_SIN[i] above are element i of   static const float c[5] = PCPX_FPFH_COS_INIT;   and its like. */
#define PCPX_FPFH_COS_INIT {0x1.eb42aap-1f, 0x1.4f49e8p-1f, 0x1.2375f6p-3f, -0x1.a9628ep-2f, -0x1.aeb8c8p-1f}
#define PCPX_FPFH_SIN_INIT {0x1.207e8p-2f, 0x1.82f19cp-1f, 0x1.fac9ep-1f, 0x1.d1bb48p-1f, 0x1.14ceep-1f}

/* Device arrays: d_normals (n_in x 3 floats); d_opt_rows (m distinct input indices; NULL, with m = 0: every row); d_fpfh (m x 33
 * floats, n_in x 33 without d_opt_rows; every row written); d_opt_spfh (n_in x 33 floats) and d_opt_pairs (n_in uint32_t), by
 * input row -- with d_opt_rows they are defined for the points that some described row's sphere holds and zero elsewhere.  Fully
 * enqueued on the handle's stream: no read-back and no synchronisation (pcpx_index_synchronize waits for it).  Scratch is the
 * handle's: 132 bytes per leaf slot for the SPFH records and 12 for the normal records, and with d_opt_rows 4 per input row and 5
 * per leaf slot more.  Under pcpx_profile_begin/end the call is booked as ONE interval of the PCPX_K_RANGE family. */
int pcpx_fpfh_self_dev(pcpx_index* idx, const float* d_normals, float radius, const uint32_t* d_opt_rows, uint64_t m, uint32_t flags,
                       float* d_fpfh, float* d_opt_spfh, uint32_t* d_opt_pairs);
/* the same with host arrays */
int pcpx_fpfh_self(pcpx_index* idx, const float* normals, float radius, const uint32_t* opt_rows, uint64_t m, uint32_t flags, float* fpfh,
                   float* opt_spfh, uint32_t* opt_pairs);

#ifdef __cplusplus
}
#endif
#endif /* PCPX_DESCRIPTORS_H */
