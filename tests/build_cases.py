"""The clouds and key sets of tests/test_gpu_build_order.py, seeded and made once.  tests/test_build_order_cpu.py asserts, from the
host's sort words, that every cloud has the property it was made for (tests/build_model.py restates the build's rules).

A case is a Case(points, grid, ...): grid None means the index makes its grid from the cloud's box."""
import functools
from collections import namedtuple

import numpy as np

import build_model as M

UNIT = np.array([0, 0, 0, 1, 1, 1], np.float32)
SIZES = (0, 1, 2, 7, 8, 9, 32, 33, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097)
KNOT_LENGTHS = (2, 16, 63, 64, 65, 66, 200)
STRADDLERS = (16, 64, 65)
END_RUN = 40  # length of the runs at the first and at the last indexed position

Case = namedtuple("Case", "points grid knots redo note")  # knots: Knot tuples (runs cloud only); redo: is the first build meant to repeat itself
Knot = namedtuple("Knot", "length kind role key40")       # kind: 'distinct' / 'copies'; role: 'plain' / 'straddle' / 'first' / 'last'


def uniform(n, seed):
    return np.random.default_rng(seed).random((n, 3), dtype=np.float32)


def _key40(points, grid=UNIT):
    """Bits [40, 64) of the points' sort words: the top-digit bucket and the 24-bit cell (they do not depend on the index bits)."""
    return (M.words_of(points, grid)[1] >> np.uint64(40)).astype(np.int64)


def _in_cell(rng, cell, count, copies):
    """`count` points well inside cell (ix, iy, iz) of the unit grid's 256^3 cells: distinct ones, or one point `count` times."""
    p = ((np.asarray(cell, np.float64) + 0.125 + 0.75 * rng.random((1 if copies else count, 3))) / 256.0).astype(np.float32)
    return np.repeat(p, count, axis=0) if copies else p


@functools.lru_cache(maxsize=None)
def runs_cloud(with_knots=True):
    """20 000 uniform points in the explicit unit grid and knots of L points inside one 24-bit cell each (a run of L words for the
    leaf kernel): every L of KNOT_LENGTHS with distinct coordinates and as exact copies; one more of each L of STRADDLERS moved, by
    filler points that sort before it, across a multiple of the leaf kernel's 1024 positions; one run at position 0 and one at
    the last.  No point lies in the last top-digit bucket, which always takes every pass: the last run is an early bucket's too.
    The knots of 66 and 200 are alone in their buckets, the only ones the build has to repeat itself for.
    with_knots=False: the base alone (the same grid, no run of any length to speak of)."""
    rng = np.random.default_rng(20260)
    base = rng.random((20600, 3), dtype=np.float32)
    kb = _key40(base)
    base, kb = base[(kb >> 16) != 255][:20000], kb[(kb >> 16) != 255][:20000]
    assert len(base) == 20000
    if not with_knots:
        return Case(base[rng.permutation(len(base))], UNIT, (), False, "base of the runs cloud")
    first_cell, last_cell = (base[np.argmin(kb)] * 256).astype(np.int64), (base[np.argmax(kb)] * 256).astype(np.int64)
    taken_buckets = {int(kb.min() >> 16), int(kb.max() >> 16)}
    used = set()

    def pick(ok_bucket):
        while True:
            cell = rng.integers(0, 256, 3)
            k = int(_key40(((cell + 0.5) / 256.0).astype(np.float32)[None, :])[0])
            if k not in used and (k >> 16) != 255 and ok_bucket(k >> 16):
                used.add(k)
                return cell, k

    knots, parts = [], []

    def add(length, kind, role, cell, k):
        pts = _in_cell(rng, cell, length, kind == "copies")
        assert (_key40(pts) == k).all()
        knots.append(Knot(length, kind, role, k))
        parts.append(pts)

    long_buckets = set()
    for length in KNOT_LENGTHS:  # the long ones first: each alone in a bucket of its own
        if length > M.FIN_RUN_MAX:
            for kind in ("distinct", "copies"):
                cell, k = pick(lambda b: b not in taken_buckets and b not in long_buckets)
                long_buckets.add(k >> 16)
                add(length, kind, "plain", cell, k)
    for length in KNOT_LENGTHS:
        if length <= M.FIN_RUN_MAX:
            for kind in ("distinct", "copies"):
                cell, k = pick(lambda b: b not in long_buckets)
                add(length, kind, "plain", cell, k)
    for length, (b0, b1) in zip(STRADDLERS, ((40, 60), (120, 140), (200, 220))):  # far apart along the curve: room for the fillers
        cell, k = pick(lambda b: b0 <= b < b1 and b not in long_buckets)
        add(length, "distinct", "straddle", cell, k)
    for role, cell in (("first", first_cell), ("last", last_cell)):
        k = int(_key40(((cell + 0.5) / 256.0).astype(np.float32)[None, :])[0])
        assert k == (kb.min() if role == "first" else kb.max()) and k not in used
        used.add(k)
        add(END_RUN, "distinct", role, cell, k)
    base = base[~np.isin(kb, list(used))]  # a knot has its cell to itself
    cloud = np.concatenate([base] + parts)
    # fillers: uniform points that sort after the first run, before the last, in no knot's cell and in no long knot's bucket
    pool = rng.random((150000, 3), dtype=np.float32)
    kp = _key40(pool)
    keep = (kp > kb.min()) & (kp < kb.max()) & ~np.isin(kp, list(used)) & ~np.isin(kp >> 16, list(long_buckets))
    pool, kp = pool[keep], kp[keep]
    after = int(kb.min())
    for knot in sorted((k for k in knots if k.role == "straddle"), key=lambda k: k.key40):
        start = int((_key40(cloud) < knot.key40).sum())
        need = (_straddle_start(knot.length) - start) % M.FINISH_TILE
        mine = np.nonzero((kp > after) & (kp < knot.key40))[0][:need]
        assert len(mine) == need
        cloud = np.concatenate([cloud, pool[mine]])
        pool, kp = np.delete(pool, mine, axis=0), np.delete(kp, mine)
        after = knot.key40
    assert len(cloud) <= 30000
    return Case(cloud[rng.permutation(len(cloud))], UNIT, tuple(knots), True, "runs")


def _straddle_start(length):
    """Where a run of `length` starts to lie half before and half after a multiple of the leaf kernel's tile."""
    return M.FINISH_TILE - length // 2


@functools.lru_cache(maxsize=None)
def size_cloud(n):
    return Case(uniform(n, 100 + n), None, (), False, "uniform, n = %d" % n)


@functools.lru_cache(maxsize=None)
def bucket_cloud(kind):
    rng = np.random.default_rng(77)
    if kind == "thin":      # every top-digit bucket holds a few dozen words
        return Case(uniform(8192, 1), UNIT, (), False, kind)
    if kind == "one":       # a cube of 1/8 of the grid's extent, aligned: nine key bits fixed, one bucket
        return Case((np.array([3, 5, 2], np.float32) + uniform(5000, 2) * np.float32(0.999)) / np.float32(8), UNIT, (), False, kind)
    if kind == "coincident":  # 5 000 copies of one point: their 16-bit cell is fuller than a bucket that stops early may have
        p = np.concatenate([uniform(2000, 3), np.repeat(np.array([[0.3, 0.6, 0.2]], np.float32), 5000, axis=0)])
        return Case(p[rng.permutation(len(p))], UNIT, (), False, kind)
    if kind == "outside":   # points outside the grid on every side, rows with NaN, +inf and -inf
        p = np.concatenate([uniform(3000, 4), uniform(200, 5) + rng.choice([-1.5, 1.5], (200, 3)).astype(np.float32), uniform(60, 6)])
        bad = np.array([np.nan, np.inf, -np.inf], np.float32)
        for j in range(60):
            p[3200 + j, j % 3] = bad[(j // 3) % 3]
        p[3259] = np.nan
        return Case(p[rng.permutation(len(p))], UNIT, (), False, kind)
    if kind == "single":    # exactly one point inside
        p = uniform(50, 7) + np.float32(2)
        p[17] = (0.25, 0.5, 0.75)
        return Case(p, UNIT, (), False, kind)
    if kind == "none":      # no point inside
        return Case(uniform(50, 8) + np.float32(2), UNIT, (), False, kind)
    raise KeyError(kind)


BUCKET_KINDS = ("thin", "one", "coincident", "outside", "single", "none")
TINY_HINT_N = 100


@functools.lru_cache(maxsize=None)
def large_cloud():
    """300 000 points inside one 16-bit cell of the explicit unit grid (a cube of 1/64 of its extent, aligned: 18 key bits fixed):
    the plan sends the bucket through every pass, and its two lowest passes have 74 tiles -- more than the grid a handle gives
    them whose build before was the tiny one (2 * low_pass_tiles + 64 blocks)."""
    p = (np.array([21, 40, 9], np.float32) + uniform(300_000, 9) * np.float32(0.999)) / np.float32(64)
    return Case(p, UNIT, (), False, "large")


@functools.lru_cache(maxsize=None)
def tiny_cloud():
    return Case(uniform(TINY_HINT_N, 10) * np.float32(0.5), UNIT, (), False, "tiny")


# ---- the plain sort ----
SORT_SIZES = (0, 1, 63, 64, 65, 4095, 4096, 4097, 8191, 8192, 8193, 70_001)
SORT_FIRST_BITS = tuple(range(0, 57, 8))
SORT_REFUSED_BITS = (57, 60)
PER_BUCKET = (4095, 4096, 4097)


def _low(rng, n, first_bit):
    """Random bits below first_bit: what tells a stable sort from another one."""
    return rng.integers(0, 1 << 63, n, dtype=np.uint64) & np.uint64((1 << first_bit) - 1)


def sort_key_sets(n, first_bit, seed=0):
    """(name, keys) for every kind of key set of n words."""
    rng = np.random.default_rng(1000 * first_bit + n + seed)
    r64 = lambda: rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    top = np.uint64(0xFF) << np.uint64(56)
    hi_mask = ~np.uint64((1 << first_bit) - 1)
    yield "equal", (np.uint64(0x5A3C96E1D2B4F078) & hi_mask) | _low(rng, n, first_bit)
    yield "one bucket", (r64() & ~top) | (np.uint64(0xA7) << np.uint64(56))
    yield "first and last bucket", (r64() & ~top) | (rng.integers(0, 2, n, dtype=np.uint64) * top)
    s = np.sort(r64())
    yield "sorted", s
    yield "reversed", s[::-1].copy()
    for byte in range(8):
        const = np.uint64(0x5A3C96E1D2B4F078) & ~(np.uint64(0xFF) << np.uint64(8 * byte))
        yield "byte %d" % byte, const | (rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(8 * byte))
    yield "random", r64()


def per_bucket_keys(per, first_bit):
    """All 256 top-digit buckets with exactly `per` words each, shuffled."""
    rng = np.random.default_rng(per + first_bit)
    n = 256 * per
    k = rng.integers(0, 1 << 56, n, dtype=np.uint64) | (np.repeat(np.arange(256, dtype=np.uint64), per) << np.uint64(56))
    return k[rng.permutation(n)]


def sorted_reference(keys, first_bit):
    return keys[np.argsort(keys >> np.uint64(first_bit), kind="stable")]
