"""The contract of include/pcpx_match.h restated in numpy: the float32 distance summed in column order on m x n arrays, the keys
(d2 bits, index) as uint64, best and second, the ratio test, the mutual test and the zero rows.  Slow and plain on purpose: the GPU
tests compare the library with this bit for bit."""
import numpy as np

F = np.float32
NONE = np.uint32(0xFFFFFFFF)
PAD = np.uint64(0xFFFFFFFFFFFFFFFF)
SKIP_ZERO_ROWS, MUTUAL = 1, 2


def d2_matrix(src, tgt):
    """m x n float32: d2 = ((e0*e0 + e1*e1) + e2*e2) + ..., e_b = s_b - t_b, every operation rounded to float32"""
    s, t = np.asarray(src, F), np.asarray(tgt, F)
    with np.errstate(all="ignore"):
        acc = None
        for b in range(s.shape[1]):
            e = s[:, b][:, None] - t[:, b][None, :]
            p = e * e
            acc = p if acc is None else acc + p
    assert acc.dtype == F
    return acc


def zero_rows(a):
    """rows all of whose entries are +0 or -0"""
    return ~(np.asarray(a, F) != 0).any(axis=1)


def keys(src, tgt, skip_zero_rows=False):
    """m x n uint64: d2 bits << 32 | target index; PAD for a pair that is skipped (NaN d2; a zero row on either side with the flag)"""
    s, t = np.asarray(src, F), np.asarray(tgt, F)
    d2 = d2_matrix(s, t)
    k = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(t.shape[0], dtype=np.uint64)[None, :]
    skip = np.isnan(d2)
    if skip_zero_rows:
        skip = skip | zero_rows(s)[:, None] | zero_rows(t)[None, :]
    k[skip] = PAD
    return k


def _unpack(k):
    idx = (k & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    d2 = (k >> np.uint64(32)).astype(np.uint32).view(F).copy()
    d2[k == PAD] = np.inf
    return idx, d2


def two_smallest(k):
    """(idx, d2, second_idx, second_d2) per row of a key matrix: its two smallest keys; NONE / +inf where there is none"""
    k = np.concatenate([k, np.full((k.shape[0], 2), PAD, np.uint64)], axis=1)
    k = np.sort(k, axis=1)[:, :2]
    return _unpack(k[:, 0]) + _unpack(k[:, 1])


def nearest(src, tgt, skip_zero_rows=False):
    """(idx, d2, second_idx, second_d2) per source row"""
    s, t = np.asarray(src, F), np.asarray(tgt, F)
    m, n = s.shape[0], t.shape[0]
    if n == 0:
        return two_smallest(np.empty((m, 0), np.uint64))
    step = max(1, 4_000_000 // n)  # (source rows at a time: the m x n arrays stay small)
    parts = [two_smallest(keys(s[a:a + step], t, skip_zero_rows)) for a in range(0, m, step)] or [two_smallest(np.empty((0, 0), np.uint64))]
    return tuple(np.concatenate(c) for c in zip(*parts))


def keep_pairs(fwd, back_idx, max_ratio_sq=1.0):
    """(pairs uint32 (K, 2) ascending i, d2 float32 (K,)) from fwd = nearest(src, tgt) and back_idx = nearest(tgt, src)[0] (None: no
    mutual test): source i is kept iff it has a best j, d2_best <= max_ratio_sq * d2_second (one float32 product, a NaN compares
    false) and, with the mutual test, the best source of target j is i"""
    i1, d1, _i2, d2 = fwd
    with np.errstate(all="ignore"):
        keep = (i1 != NONE) & (d1 <= F(max_ratio_sq) * d2)
    if back_idx is not None and len(back_idx):
        j = np.where(i1 != NONE, i1, 0).astype(np.int64)
        keep &= back_idx[j] == np.arange(len(i1), dtype=np.uint32)
    rows = np.nonzero(keep)[0]
    return np.stack([rows.astype(np.uint32), i1[rows]], axis=1).reshape(-1, 2), d1[rows]


def correspondences(src, tgt, max_ratio_sq=1.0, flags=0):
    """the kept (source, target) pairs and their d2: keep_pairs of the two directions"""
    skip = bool(flags & SKIP_ZERO_ROWS)
    return keep_pairs(nearest(src, tgt, skip), nearest(tgt, src, skip)[0] if flags & MUTUAL else None, max_ratio_sq)


def merge_chunks(parts, offsets):
    """best and second over target chunks matched by separate calls: parts = [(idx, d2, second_idx, second_d2)] per chunk, offsets =
    the chunks' first target rows.  The same (idx, d2, second_idx, second_d2) as one call on all the targets gives."""
    cols = []
    for (i1, d1, i2, d2), off in zip(parts, offsets):
        for i, d in ((i1, d1), (i2, d2)):
            k = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (i.astype(np.uint64) + np.uint64(off))
            k[i == NONE] = PAD
            cols.append(k)
    k = np.sort(np.stack(cols + [np.full_like(cols[0], PAD)] * 2, axis=1), axis=1)[:, :2]
    return _unpack(k[:, 0]) + _unpack(k[:, 1])
