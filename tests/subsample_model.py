"""A numpy restatement of the subsampling contract of include/pcpx_subsample.h, from an edge list.  numpy only:
no GPU, no package import.  Edges come from cluster_model.brute_edges / edges_from_lists: (src, dst) ordered pairs, both directions
of every pair present (pairs (i, i) may be present and are ignored).

    fmix32(x)                          -> the 32-bit finaliser of MurmurHash3, elementwise
    keys(n, seed)                      -> key(i) = fmix32(i ^ seed) for i < n
    greedy(n, src, dst, seed[, ids])      -> keep (bool): the literal sequential loop in ascending key
    rounds_form(n, src, dst, seed[, ids]) -> (keep, rounds): the synchronous round form
    owners(n, src, dst, d2, keep)      -> the kept point of smallest (d2 bits, index) in every point's sphere; itself if kept

The contract: i is kept iff no kept j ~ i has key(j) < key(i)."""
import numpy as np

NONE = np.uint32(0xFFFFFFFF)
M32 = np.uint64(0xFFFFFFFF)


def fmix32(x):
    x = np.asarray(x).astype(np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & M32
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & M32
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def keys(n, seed=0, ids=None):
    """ids: the input index of every vertex (None: vertex v is input row v) -- a graph over the indexed subset of a cloud keeps the
    keys of the rows it came from"""
    ids = np.arange(n, dtype=np.uint64) if ids is None else np.asarray(ids).astype(np.uint64)
    return fmix32(ids ^ np.uint64(int(seed) & 0xFFFFFFFF))


def _earlier(n, src, dst, seed, ids=None):
    """the pairs (i, j) with key(j) < key(i), grouped by i: (key, i of every pair, j of every pair, first pair of every i)"""
    key = keys(n, seed, ids)
    src = np.asarray(src, np.int64)
    dst = np.asarray(dst, np.int64)
    take = key[dst] < key[src]
    src, dst = src[take], dst[take]
    order = np.argsort(src, kind="stable")
    src, dst = src[order], dst[order]
    start = np.searchsorted(src, np.arange(n + 1))
    return key, src, dst, start


def greedy(n, src, dst, seed=0, ids=None):
    """Visit the points in ascending key; keep a point iff no kept point is in its sphere."""
    key, _, dst, start = _earlier(n, src, dst, seed, ids)
    keep = np.zeros(n, bool)
    for i in np.argsort(key, kind="stable").tolist():
        keep[i] = not keep[dst[start[i]:start[i + 1]]].any()  # (only earlier-visited partners can be kept by now: the others are not needed)
    return keep


def rounds_form(n, src, dst, seed=0, ids=None):
    """Every round reads the states as they were when it began: an undecided point with a kept partner of smaller key is dropped;
    else, with an undecided one, it waits; else it is kept.  Returns (keep, the rounds in which something was undecided)."""
    UNDECIDED, KEPT, DROPPED = 0, 1, 2
    _, src, dst, _ = _earlier(n, src, dst, seed, ids)
    state = np.full(n, UNDECIDED, np.int8)
    rounds = 0
    while (state == UNDECIDED).any():
        rounds += 1
        live = state[src] == UNDECIDED
        src, dst = src[live], dst[live]
        sees_kept = np.zeros(n, bool)
        sees_kept[src[state[dst] == KEPT]] = True
        sees_undecided = np.zeros(n, bool)
        sees_undecided[src[state[dst] == UNDECIDED]] = True
        undecided = state == UNDECIDED
        state[undecided & sees_kept] = DROPPED
        state[undecided & ~sees_kept & ~sees_undecided] = KEPT
    return state == KEPT, rounds


def owners(n, src, dst, d2, keep):
    """owner[i] = i for a kept point, else the kept j in i's sphere of smallest (bits of the float32 d2 of the pair, j); NONE where
    there is none.  d2: the squared distance of every pair, float32, as the walk forms it."""
    src = np.asarray(src, np.int64)
    dst = np.asarray(dst, np.int64)
    bits = np.ascontiguousarray(d2, np.float32).view(np.uint32).astype(np.uint64)
    take = keep[dst] & ~keep[src]
    word = (bits[take] << np.uint64(32)) | dst[take].astype(np.uint64)
    best = np.full(n, np.iinfo(np.uint64).max, np.uint64)
    np.minimum.at(best, src[take], word)
    out = (best & M32).astype(np.uint32)
    out[best == np.iinfo(np.uint64).max] = NONE
    out[keep] = np.nonzero(keep)[0].astype(np.uint32)
    return out


def pair_d2(pts, src, dst):
    """(dx*dx + dy*dy) + dz*dz of every pair, d = p_dst - p_src, in float32 (three roundings, no fused multiply-add)"""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    d = pts[np.asarray(dst, np.int64)] - pts[np.asarray(src, np.int64)]
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
