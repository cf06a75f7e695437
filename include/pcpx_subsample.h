/*
 * pcpx_subsample.h -- Poisson-disk subsampling of libpcpx.so: the subsample of the indexed cloud in which no two points are within
 * `radius` of each other and every dropped point has a kept point within `radius` ("spatial subsampling", minimum-distance
 * thinning), in a few walks of the index and without materialising the neighbour lists.
 *
 * A companion of pcpx.h with its conventions: POD arguments, pcpx_status codes, pcpx_last_error(); a rank-local (shard) handle
 * is refused with PCPX_ERR_UNSUPPORTED.
 *
 * The contract is exact and does not depend on the tree, the voxel grid, the launch order or the run:
 *   - edge: i ~ j iff j is in i's sphere by the rule of pcpx_range_count_*: d2 <= r*r (d = p_j - p_i, float32, three roundings,
 *     no FMA); only points inside the index's voxel grid are in any sphere.  The rule is symmetric.
 *   - priority: key(i) = fmix32(i XOR seed), i the input index, fmix32 the 32-bit finaliser of MurmurHash3
 *     (x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16, modulo 2^32): a bijection on 32-bit words, so
 *     the keys are distinct and the order is strict.
 *   - kept set: the one set K with: an indexed point i is in K iff no j in K has j ~ i and key(j) < key(i) -- what the sequential
 *     greedy loop gives that visits the points in ascending key and keeps a point iff no kept point is in its sphere.  So no two
 *     kept points are within r of each other, and every indexed dropped point has a kept point within r.
 *   - a point outside the voxel grid is dropped.  radius 0 keeps one point of every set of exact duplicates, the one of smallest
 *     key: a de-duplication call.  radius > 1 is the geometric answer.
 *   - owner (optional): a kept point owns itself; an indexed dropped point belongs to the kept point in its sphere of smallest
 *     (d2 bits, input index); a point outside the grid has PCPX_SUBSAMPLE_NONE.  Use: averaging colours or normals onto the sample.
 * Another `seed` gives another sample.  "First in input order wins" is NOT offered: the chain of decisions is then as long as the
 * scan line (a 200 000-point helix in input order decides two points per round; under the hashed key it ends in eight or nine).
 *
 * radius < 0 or NaN, flags != 0 or a NULL keep array are PCPX_ERR_INVALID.  An empty cloud is fine (count 0, no rounds).
 */
#ifndef PCPX_SUBSAMPLE_H
#define PCPX_SUBSAMPLE_H

#include "pcpx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCPX_SUBSAMPLE_NONE 0xFFFFFFFFu
/* The call launches rounds until every point is decided and reads a 4-byte counter back after every PCPX_SUBSAMPLE_ROUND_BATCH of
 * them: the number of round launches it reports is a multiple of this (the launches over a cloud that is decided already return
 * after one load per group).  Under pcpx_profile_begin/end the whole call -- rounds, owners, rows, scan -- is booked as ONE
 * interval of the PCPX_K_RANGE family. */
#define PCPX_SUBSAMPLE_ROUND_BATCH 4u

/* Device arrays: d_keep (required; n_in rows, 1 = kept); d_opt_owner (n_in rows); d_opt_kept_rows (room for n_in entries: the
 * kept input indices, ascending); d_opt_kept_count (one uint64_t).  *opt_rounds is a HOST word: the round launches issued.
 * On the handle's stream; scratch is the handle's (4 bytes per point).  Unlike the other _dev entry points this one SYNCHRONISES
 * the handle's stream between rounds (the number of rounds is data dependent, as the levels of pcpx_hierarchy_simplification_dev
 * are); what follows the last round is enqueued and pcpx_index_synchronize waits for it. */
int pcpx_subsample_self_dev(pcpx_index* idx, float radius, uint32_t seed, uint32_t flags, uint8_t* d_keep, uint32_t* d_opt_owner,
                            uint32_t* d_opt_kept_rows, uint64_t* d_opt_kept_count, uint32_t* opt_rounds);
/* the same with host arrays; kept_rows[0 .. *opt_kept_count) are written */
int pcpx_subsample_self(pcpx_index* idx, float radius, uint32_t seed, uint32_t flags, uint8_t* keep, uint32_t* opt_owner,
                        uint32_t* opt_kept_rows, uint64_t* opt_kept_count, uint32_t* opt_rounds);

#ifdef __cplusplus
}
#endif
#endif /* PCPX_SUBSAMPLE_H */
