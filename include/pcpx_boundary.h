/*
 * pcpx_boundary.h -- boundary points of libpcpx.so: which points of a sampled surface lie on its border -- the rim of an open scan,
 * the edge of a hole, the outline of a plane that pcpx_extract_planes found -- by the angle criterion (PCL's BoundaryEstimation;
 * Bendels, Schnabel and Klein 2006 for hole detection): a point is on the border iff the directions to its neighbours, projected
 * into its tangent plane, leave a large empty angle.  One walk of the index, without materialising the neighbour lists: a
 * point's state is ONE 64-bit word, the set of the 64 sectors of 5.625 degrees in which some neighbour lies.
 *
 * A companion of pcpx.h with its conventions: POD arguments, pcpx_status codes, pcpx_last_error(); a rank-local (shard) handle
 * is refused with PCPX_ERR_UNSUPPORTED.  An empty cloud is fine (count 0).
 *
 * WHERE THE ARRAYS LIVE.  The call is declared once and takes `flags`:
 *   PCPX_BOUNDARY_ON_DEVICE   every array argument (the normals included) is a device pointer, owing its element type's alignment
 *                             and no more.  Fully enqueued on the handle's stream: no read-back, no synchronisation
 *                             (pcpx_index_synchronize waits for it).  Scratch is the handle's.  Under pcpx_profile_begin/end the
 *                             call is booked as ONE interval of the PCPX_K_RANGE family.
 *   0                         host arrays; the call returns when they are written (staged around the same device path).
 *   any other bit             PCPX_ERR_INVALID.
 *
 * THE CONTRACT is exact and does not depend on the tree, the voxel grid, the launch order or the run: the mask is an OR over the
 * neighbours, which commutes.  All arithmetic is float32, one rounding per operation, no FMA, denormals preserved.
 *   sphere   j is in i's sphere iff d2 <= r*r by the rule of pcpx_range_count_* (d = p_j - p_i, three roundings); only points
 *            inside the index's voxel grid are in any sphere; the centre is in its own sphere.  count_i = the points in the sphere.
 *   frame    n = normals[i] as given (n_in x 3 floats; a non-unit normal is not an error).  has_frame_i iff the three components
 *            are finite and not all zero.  With ax, ay, az = |n|:
 *                ax <= ay && ax <= az:  u = (0, -nz, ny)
 *                else ay <= az:         u = (-nz, 0, nx)
 *                else:                  u = (-ny, nx, 0)
 *            and v = n x u, each component two products and one subtraction (vx = ny uz - nz uy, vy = nz ux - nx uz,
 *            vz = nx uy - ny ux).  Nothing is normalised: a sector depends only on the direction of (a, b), and for a unit normal u
 *            and v are equally long.  (For a normal of length L, v is L times as long as u: the angles are those of the tangent
 *            plane stretched by L along v.  Pass unit normals.)
 *   partner  a = (dx ux + dy uy) + dz uz, b = (dx vx + dy vy) + dz vz.  A partner with a == 0 && b == 0 -- the centre, an exact
 *            duplicate, a point on the normal's line -- has no direction: it is counted and sets no sector.
 *   sector   of (a, b), 64 sectors of 5.625 degrees: swap = |b| > |a|, x = swap ? |b| : |a|, y = swap ? |a| : |b| (the larger
 *            and the smaller magnitude); sub = the number of k in 1 .. 7 with y >= T_k x (the product rounded), T_k the float32
 *            nearest to tan(k pi / 32), listed below; q = swap ? 15 - sub : sub;
 *                a >= 0, b >= 0:  s = q            a <  0, b >= 0:  s = 31 - q
 *                a <  0, b <  0:  s = 32 + q       a >= 0, b <  0:  s = 63 - q
 *            the signs by `<`, so -0 is >= 0.  (T_k x does not decrease with k, so three steps of a binary search give the same
 *            sub as seven compares.)  A point whose (a, b) rounds across a sector border is assigned as computed.
 *   sectors  sectors_i = the OR of 1 << s over the partners that have a direction.
 *   gap      G_i = the longest cyclic run of zero bits of sectors_i: 64 for the mask 0, 0 for the full mask.  start_i = the lowest
 *            s with bit s clear, bit (s - 1) mod 64 set and a run of G_i zero bits from s on; 0 for the mask 0 and for G_i = 0.
 *   keep     keep_i = indexed_i && has_frame_i && count_i >= max(min_neighbours, 1) && G_i >= gap_sectors.
 * WHAT IT MEANS.  If theta is the largest empty angle between the directions of a point's neighbours in its tangent plane, then
 * G 5.625 degrees <= theta < (G + 2) 5.625 degrees: an empty angle covers every sector strictly inside it and at most a part of
 * the two at its ends.  So gap_sectors = 16 keeps no point whose largest empty angle is below 90 degrees (PCL's default threshold)
 * and every point whose largest empty angle is at least 101.25 degrees.
 *
 * THE ARRAYS.  normals: n_in x 3 floats (required).  keep: n_in rows, every row written, 1 = kept (required).  opt_kept_rows: room
 * for n_in entries; the kept input indices, ascending; only [0, count) are written.  opt_kept_count: one uint64_t.  opt_gap: n_in x 2
 * bytes {G, start}; opt_count: n_in entries; opt_sectors: n_in 64-bit masks -- every row of them written: a row outside the voxel
 * grid gets keep 0, gap {255, 255}, count 0, sectors 0; an indexed row without a frame keep 0, gap {255, 255}, sectors 0 and its
 * true count.
 *
 * radius < 0 or NaN, gap_sectors outside 1 .. 64, a NULL normals or keep array and an unknown flag bit are PCPX_ERR_INVALID.
 */
#ifndef PCPX_BOUNDARY_H
#define PCPX_BOUNDARY_H

#include "pcpx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCPX_BOUNDARY_ON_DEVICE 1u
#define PCPX_BOUNDARY_SECTORS 64u

/* T_k = the float32 nearest to tan(k pi / 32), k = 1 .. 7 (hexadecimal floats: every bit is part of the contract) */
#define PCPX_BOUNDARY_TANS                                                                                                         \
    {                                                                                                                               \
        0x1.936bb8p-4f, 0x1.975f5ep-3f, 0x1.36a084p-2f, 0x1.a8279ap-2f, 0x1.11ab72p-1f, 0x1.561b82p-1f, 0x1.a43002p-1f             \
    }

int pcpx_boundary_self(pcpx_index* idx, const float* normals, float radius, uint32_t gap_sectors, uint32_t min_neighbours, uint32_t flags,
                       uint8_t* keep, uint32_t* opt_kept_rows, uint64_t* opt_kept_count, uint8_t* opt_gap /* n_in x 2 */, uint32_t* opt_count,
                       uint64_t* opt_sectors);

#ifdef __cplusplus
}
#endif
#endif /* PCPX_BOUNDARY_H */
