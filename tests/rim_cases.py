"""The clouds, radii, rules and rows of tests/test_rim_cpu.py and tests/test_gpu_rim.py: every fixed-radius operation on lattices, where
points and leaf boxes lie EXACTLY at the radius ("The rim").  numpy only: no GPU, no package import.

The contract (include/pcpx.h, conventions; sphere.hpp:27-35) is a closed ball: d = p - q per axis, (dx dx + dy dy) + dz dz in float32
with no fused multiply-add, inside iff that is <= fl(r r).  On a dyadic lattice all of it is exact, so the contract is integer
arithmetic: with g the integer sites (p = offset + S g),

    inside  iff  |g_i - g_j|^2 <= K,    K = floor(fl(r r) / S^2)

and that -- integers, not one more float32 restatement -- is the reference here.

    CLOUDS   full9      all 9^3 = 729 sites
             thin12     a seeded 60 % of the 12^3 sites, 1 037 points: not symmetric, and the removed sites are outside centres
             thin12far  thin12 moved by (64, -32, 16): still exact in float32
             (rows in a seeded permutation of the sites)
    RADII    s          fl(r r) = s^2 exactly, K = 1:           a `<` for the `<=` loses the six nearest sites
             sqrt2_s    fl(sqrt 2) s, fl(r r) = 1.9999999 s^2, K = 1:  fl(sqrt(2 s^2)) <= r holds, so a rule on distances lets the 12 face diagonals in
             sqrt3_s    fl(sqrt 3) s, fl(r r) = 3 s^2 exactly though r^2 = 2.9999999 s^2, K = 3:  an r^2 formed in double, or a `<`, loses the 8 corners
             3s         K = 9:  a `<` loses the (3, 0, 0) and (2, 2, 1) shells; long lists
    RULES    contract, and three wrong ones: strict (d2 < fl(r r)), exact (d2 <= r^2 in rationals), distance (fl(sqrt d2) <= r)

`bound(radius, rule)` is the largest integer squared distance a rule lets in; every radius is separated from the contract by at
least one wrong rule (tests/test_rim_cpu.py).  A model that takes an edge list gets the integer edges of a rule; a model that takes
(points, radius) gets, for a wrong rule, `EQUIVALENT[bound]`: a radius with no lattice distance between its square and that bound.

A ROW is an operation: `model(case, rule)` gives what it must return under a rule, as a dict of arrays; `exact` names the outputs
that the GPU test compares bit for bit with the contract's and that a wrong rule must change on at least one (cloud, radius);
`fixed` names those compared exactly that no sphere rule can change (the smooth mask of a curvature gate).  Seeded inputs, built
once, never changed."""
import collections
import fractions
import functools

import numpy as np

import boundary_model as BoM
import cluster_model as CM
import fpfh_model as PM
import fps_model as FM
import icp_model as IM
import keypoints_model as KM
import mls_model as MM
import outliers_model as OM
import segment_model as GM
import subsample_model as UM

F = np.float32
S = 2.0 ** -3
NONE = np.uint32(0xFFFFFFFF)
CLOUDS = ("full9", "thin12", "thin12far")
FAR_SHIFT = np.array([64.0, -32.0, 16.0])
THIN_KEPT = 1037  # 60 % of 12^3
SEEDS = {"full9": 909, "thin12": 1212, "thin12far": 1212}
RADII = ("s", "sqrt2_s", "sqrt3_s", "3s")
RULES = ("contract", "strict", "exact", "distance")
WRONG = RULES[1:]
EQUIVALENT = {0: 0.5, 2: 1.5, 8: 2.9}  # wrong bound -> radius / S
D2_MAX = 64  # integers looked at by `bound`


def radius(name):
    """the float32 radius of a name"""
    return {"s": F(S), "sqrt2_s": np.sqrt(F(2)) * F(S), "sqrt3_s": np.sqrt(F(3)) * F(S), "3s": F(3) * F(S)}[name]


def holds(m, r, rule):
    """does `rule` let the integer squared distance m (d2 = m S^2, exact in float32) into a sphere of the float32 radius r"""
    r = F(r)
    d2 = F(m) * F(S * S)
    if rule == "contract":
        return bool(d2 <= r * r)
    if rule == "strict":
        return bool(d2 < r * r)
    if rule == "exact":
        return fractions.Fraction(m) * fractions.Fraction(S) ** 2 <= fractions.Fraction(float(r)) ** 2
    if rule == "distance":
        return bool(np.sqrt(d2) <= r)
    raise ValueError(rule)


@functools.lru_cache(maxsize=None)
def _bound(r, rule):
    ok = [holds(m, r, rule) for m in range(D2_MAX)]
    k = ok.index(False) - 1 if False in ok else D2_MAX - 1
    assert all(ok[:k + 1]) and not any(ok[k + 1:])  # (monotone)
    return k


def bound(r, rule="contract"):
    """the largest integer m the rule lets in (-1: none), for a radius by name or by value"""
    return _bound(float(radius(r)) if isinstance(r, str) else float(F(r)), rule)


def rule_radius(name, rule):
    """what a (points, radius) model gets for a rule: the radius itself where the rule agrees with the contract there"""
    k = bound(name, rule)
    return float(radius(name)) if k == bound(name) else float(F(EQUIVALENT[k]) * F(S))


def interior_count(k):
    """the sites within integer squared distance k of a site, itself included, in a full lattice"""
    a = np.arange(-8, 9)
    x, y, z = np.meshgrid(a, a, a, indexing="ij")
    return int((x * x + y * y + z * z <= k).sum())


# ---- clouds -----------------------------------------------------------------------------------------------------------------------------
def _grid(lo, hi):
    a = np.arange(lo, hi)
    return np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3).astype(np.int64)


def _thin():
    """(kept, removed) sites of the 12^3 lattice"""
    take = np.zeros(12 ** 3, bool)
    take[np.random.default_rng(SEEDS["thin12"]).permutation(12 ** 3)[:THIN_KEPT]] = True
    g = _grid(0, 12)
    return g[take], g[~take]


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def sites(cloud):
    """the integer sites of a cloud's rows (n, 3) int64"""
    g = _grid(0, 9) if cloud == "full9" else _thin()[0]
    return _frozen(g[np.random.default_rng(SEEDS[cloud] + 1).permutation(len(g))])


@functools.lru_cache(maxsize=None)
def absent(cloud):
    """integer sites that hold no point: one step outside the hull for full9, the removed sites of thin12"""
    if cloud == "full9":
        g = _grid(-1, 10)
        g = g[((g < 0) | (g > 8)).any(1)]
    else:
        g = _thin()[1]
    return _frozen(g[np.random.default_rng(SEEDS[cloud] + 2).permutation(len(g))])


@functools.lru_cache(maxsize=None)
def source_sites(cloud):
    """the source of nearest_posed: the absent sites and the three shells outside the hull -- the nearest point of a site 3 steps
    outside a face is at exactly 3 S, that of a site outside an edge or a corner at sqrt 2 S or sqrt 3 S, and ties several ways"""
    size = 9 if cloud == "full9" else 12
    g = _grid(-3, size + 3)
    g = g[((g < 0) | (g >= size)).any(1)]
    g = g[np.random.default_rng(SEEDS[cloud] + 4).permutation(len(g))]
    return _frozen(g if cloud == "full9" else np.concatenate([absent(cloud), g]))  # (full9's absent sites are its first shell)


def offset(cloud):
    return FAR_SHIFT if cloud.endswith("far") else np.zeros(3)


def at(cloud, g):
    """the float32 points of integer sites, exact (asserted)"""
    p64 = offset(cloud) + np.asarray(g, np.float64) * S
    p = p64.astype(F)
    assert np.array_equal(p.astype(np.float64), p64), "a coordinate is not exact in float32"
    return _frozen(p)


@functools.lru_cache(maxsize=None)
def points(cloud):
    return at(cloud, sites(cloud))


def d2_int(a, b):
    """|a_i - b_j|^2 of integer sites, (len(a), len(b)) int64"""
    d = a[:, None, :] - b[None, :, :]
    return (d * d).sum(-1)


@functools.lru_cache(maxsize=None)
def _self_d2(cloud):
    return _frozen(d2_int(sites(cloud), sites(cloud)))


@functools.lru_cache(maxsize=None)
def edges(cloud, k):
    """(src, dst, counts): every ordered pair of rows with integer squared distance <= k, (i, i) included, by (src, dst)"""
    src, dst = np.nonzero(_self_d2(cloud) <= k)
    return _frozen(src.astype(np.int64)), _frozen(dst.astype(np.int64)), _frozen(np.bincount(src, minlength=len(sites(cloud))).astype(np.uint32))


def lists_of(inside):
    """CSR (offsets uint64, indices uint32 ascending in every list) of a boolean (centres, points) matrix"""
    src, dst = np.nonzero(inside)
    off = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=inside.shape[0]))]).astype(np.uint64)
    return off, dst.astype(np.uint32)


def sorted_lists(off, idx):
    """each list of a CSR pair ascending (the batch forms' lists are in unspecified order)"""
    out = np.asarray(idx).copy()
    for a, b in zip(off[:-1].astype(np.int64), off[1:].astype(np.int64)):
        out[a:b] = np.sort(out[a:b])
    return out


# ---- the seeded inputs of a cloud ---------------------------------------------------------------------------------------------------------
BATCH_OWN = 3  # the batch forms' centres: the absent sites and every third point of the cloud
# segment's threshold by radius: uniform directions are compatible with probability 1 - min_cos, so a sphere holds one or two compatible
# partners at every radius and the segments hang on single pairs -- with a laxer one the 3s graph is one component under any rule
MIN_COS = {"s": 0.75, "sqrt2_s": 0.75, "sqrt3_s": 0.94, "3s": 0.985}
MAX_CURVATURE, MIN_SIZE = 0.5, 3
SUBSAMPLE_SEED = 5
MIN_SCORE, MAXIMA_MIN_NEIGHBOURS = 0.25, 2
ISS_GAMMA, ISS_MIN_NEIGHBOURS = 0.975, 5
# the salient radius that goes with a non-maximum radius (never sqrt3_s: on full9 no neighbourhood of that radius passes the strict
# ratio tests, every one has two equal eigenvalues)
ISS_SALIENT = {"s": "3s", "sqrt2_s": "3s", "sqrt3_s": "3s", "3s": "s"}
GAUSS_H = float(F(1.5) * F(S))  # MLS's width, the same at every radius
STEP = np.array([[1, 0, 0, S], [0, 1, 0, 0], [0, 0, 1, -S], [0, 0, 0, 1]], np.float64)  # one lattice step along x and back along z
POSES = {"identity": None, "step": STEP}
STEP_SITES = np.array([1, 0, -1], np.int64)
FPFH_SUBSET = 5  # every fifth row, descending


@functools.lru_cache(maxsize=None)
def inputs(cloud):
    n = len(sites(cloud))
    rng = np.random.default_rng(SEEDS[cloud] + 3)
    v = rng.normal(size=(n, 3))  # unit normals, uniform over the upper hemisphere ...
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v[v[:, 2] < 0] *= -1.0
    v[rng.uniform(size=n) < 0.3] *= -1.0  # ... with a share flipped: |n_i . n_j| must not care, the pair features must
    centres = np.concatenate([absent(cloud), sites(cloud)[::BATCH_OWN]])
    d = {"normals": v.astype(F), "flat": np.tile(np.array([0, 0, 1], F), (n, 1)),
         "score": (np.floor(rng.uniform(0, 16, n)) / 16).astype(F), "curvature": rng.uniform(0, 1, n).astype(F),
         "rows": np.arange(n - 1, -1, -FPFH_SUBSET).astype(np.uint32),
         "centre_sites": centres, "centres": at(cloud, centres).copy(),
         "radius_of": rng.integers(0, len(RADII), len(centres)),  # the mixed radii: one of the four per sphere
         "source": at(cloud, source_sites(cloud)).copy()}
    return {k: _frozen(a) for k, a in d.items()}


def mixed_names(cloud, rname):
    """the radius name of every batch sphere: the seeded mix, turned by the case's radius so that every case has another"""
    return [RADII[(int(j) + RADII.index(rname)) % len(RADII)] for j in inputs(cloud)["radius_of"]]


def mixed_radii(cloud, rname):
    return np.array([radius(name) for name in mixed_names(cloud, rname)], F)


class Case:
    """a cloud and a radius: the points, the radius as float32 and as a Python float, and what a rule makes of them"""

    def __init__(self, cloud, rname):
        self.cloud, self.rname = cloud, rname
        self.g, self.pts, self.I = sites(cloud), points(cloud), inputs(cloud)
        self.n, self.r = len(self.g), float(radius(rname))

    def __repr__(self):
        return "%s/%s" % (self.cloud, self.rname)

    def bound(self, rule="contract"):
        return bound(self.rname, rule)

    def radius(self, rule="contract"):
        return rule_radius(self.rname, rule)

    def edges(self, rule="contract"):
        return edges(self.cloud, self.bound(rule))

    def counts(self, rule="contract"):
        return self.edges(rule)[2]

    def sets(self, rule="contract"):
        """the rows inside every row's sphere, ascending"""
        src, dst, cnt = self.edges(rule)
        return np.split(dst, np.cumsum(cnt.astype(np.int64))[:-1])

    def batch_inside(self, rule="contract"):
        """(centres, points) bool: the mixed-radii spheres"""
        k = np.array([bound(name, rule) for name in mixed_names(self.cloud, self.rname)], np.int64)
        return d2_int(self.I["centre_sites"], self.g) <= k[:, None]

    def batch_sets(self, rule="contract"):
        return [np.nonzero(row)[0] for row in self.batch_inside(rule)]

    def absent_counts(self, rule="contract"):
        return (d2_int(absent(self.cloud), self.g) <= self.bound(rule)).sum(1).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def case(cloud, rname):
    return Case(cloud, rname)


def all_cases():
    return [(cloud, rname) for cloud in CLOUDS for rname in RADII]


def rim_share(c):
    """the pairs at exactly the contract's bound as a share of all pairs inside, the pairs (i, i) among them"""
    d = _self_d2(c.cloud)
    k = c.bound()
    return float((d == k).sum()) / float((d <= k).sum())


# ---- the rows -----------------------------------------------------------------------------------------------------------------------------
def outlier_bounds(c):
    """min_neighbours of the two radius_outliers calls: the interior count (keeping hinges on a full shell) and the median count"""
    return interior_count(c.bound()), int(np.median(c.counts()))


def _counts(c, rule):
    cnt = c.counts(rule)
    out = {"self": cnt, "absent": c.absent_counts(rule)}
    for name, at_least in zip(("keep_interior", "keep_median"), outlier_bounds(c)):
        keep, mcnt = OM.radius(c.pts, None, c.radius(rule), at_least)
        assert np.array_equal(mcnt, cnt)  # (outliers_model is float32: tied to the integers here)
        out[name] = keep
    return out


def _lists(c, rule):
    off, idx = lists_of(_self_d2(c.cloud) <= c.bound(rule))
    boff, bidx = lists_of(c.batch_inside(rule))
    return {"offsets": off, "idx": idx, "batch_offsets": boff, "batch_idx": bidx}


def _set_counts(c, rule):
    return {"counts_self": c.counts(rule), "counts_batch": c.batch_inside(rule).sum(1).astype(np.uint32)}


# (name, compact): min_pts 1 and 7, and "sparse" -- a min_pts by radius at which so few points of thin12 are core that their components
# hang on single pairs at exactly r: with the counts right, k_cluster_hook's compare alone and k_cluster_border's alone decide labels
# (tests/test_rim_cpu.py::test_each_kernel_of_a_row_has_teeth; at min_pts 7 the core graph at sqrt 3 s and 3 s is connected without them)
CLUSTER_FORMS = (("m1", True), ("m1", False), ("m7", True), ("m7", False), ("sparse", False))
SPARSE_MIN_PTS = {"s": 5, "sqrt2_s": 5, "sqrt3_s": 19, "3s": 80}


def cluster_min_pts(name, rname):
    return {"m1": 1, "m7": 7, "sparse": SPARSE_MIN_PTS[rname]}[name]


def cluster_tag(name, compact):
    return "_%s_%s" % (name, "compact" if compact else "plain")


def without_rim(c, from_mask, to_mask):
    """the contract's edges less those at exactly the bound that lead from a row of from_mask to one of to_mask: what ONE kernel with
    a `<` for its `<=` sees while the others see the contract's"""
    src, dst, cnt = c.edges()
    keep = ~((_self_d2(c.cloud)[src, dst] == c.bound()) & from_mask[src] & to_mask[dst])
    return src[keep], dst[keep], cnt


def _cluster(c, rule):
    src, dst, cnt = c.edges(rule)
    out = {"counts": cnt}
    for name, compact in CLUSTER_FORMS:
        lab, core, count = CM.cluster(c.n, src, dst, cnt, cluster_min_pts(name, c.rname), compact=compact, symmetric=True)
        tag = cluster_tag(name, compact)
        out["labels" + tag], out["count" + tag] = lab, np.array([count], np.uint64)
        if name != "m1":  # (at min_pts 1 every point is core under any rule: the GPU test asserts that much)
            out["core" + tag] = core.astype(np.uint8)
    return out


def _segment(c, rule):
    e = c.edges(rule)
    lab, _smooth, count = GM.segment_cloud(c.pts, c.I["normals"], c.radius(rule), MIN_COS[c.rname], edges=e)
    glab, gsmooth, gcount = GM.segment_cloud(c.pts, c.I["normals"], c.radius(rule), MIN_COS[c.rname], curvature=c.I["curvature"], edges=e,
                                             max_curvature=MAX_CURVATURE, min_size=MIN_SIZE)
    return {"labels": lab, "count": np.array([count], np.uint64), "gated_labels": glab, "gated_count": np.array([gcount], np.uint64),
            "gated_smooth": gsmooth.astype(np.uint8)}


def _subsample(c, rule):
    src, dst, _cnt = c.edges(rule)
    keep, _rounds = UM.rounds_form(c.n, src, dst, SUBSAMPLE_SEED)
    return {"keep": keep.astype(np.uint8), "owner": UM.owners(c.n, src, dst, UM.pair_d2(c.pts, src, dst), keep)}


def _local_maxima(c, rule):
    keep = KM.local_maxima_cloud(c.pts, c.I["score"], c.radius(rule), MIN_SCORE, MAXIMA_MIN_NEIGHBOURS, edges=c.edges(rule))
    return {"keep": keep.astype(np.uint8)}


def iss_radii(c):
    """(salient, non-maximum): the latter is the case's radius, both from the table"""
    return float(radius(ISS_SALIENT[c.rname])), c.r


def _iss(c, rule):
    """the float64 saliency of the rule's salient spheres and its maxima over the rule's non-maximum spheres (the GPU test takes the
    device's own eigenvalues through keypoints_model.iss_score instead, as tests/test_gpu_keypoints.py does)"""
    salient = edges(c.cloud, bound(ISS_SALIENT[c.rname], rule))
    sal = KM.iss_saliency_f64(c.pts, None, ISS_GAMMA, ISS_GAMMA, edges=salient)
    keep = KM.local_maxima_cloud(c.pts, sal, c.radius(rule), min_neighbours=ISS_MIN_NEIGHBOURS, edges=c.edges(rule))
    return {"passes": (~np.isnan(sal)).astype(np.uint8), "keep": keep.astype(np.uint8)}


def fpfh_rows(c, rule="contract", rows=None):
    """fpfh_model's SPFH and pair counts of `rows` (default: all)"""
    rows = np.arange(c.n) if rows is None else rows
    spfh, pairs = PM.spfh(c.pts, c.I["normals"], rows, c.radius(rule))
    return {"spfh": spfh, "pairs": pairs}


def _fpfh_teeth(c, rule):
    return fpfh_rows(c, rule, c.I["rows"].astype(np.int64))  # (the subset: the model is a loop over rows)


def _nearest(c, rule):
    """by integers: the lowest row among the nearest sites within the bound -- and icp_model says the same"""
    out = {}
    for name, pose in POSES.items():
        d = d2_int(source_sites(c.cloud) + (STEP_SITES if name == "step" else 0), c.g)
        d = np.where(d <= c.bound(rule), d, np.iinfo(np.int64).max)
        j = np.argmin(d, 1)  # (the first of equal minima)
        best = d[np.arange(len(j)), j]
        has = best != np.iinfo(np.int64).max
        partner = np.where(has, j, NONE).astype(np.uint32)
        d2 = np.where(has, best * (S * S), np.inf).astype(F)
        mp, md = IM.nearest_posed(c.pts, c.I["source"], pose, c.radius(rule))
        assert np.array_equal(mp, partner) and np.array_equal(md, d2)
        out["partner_" + name], out["d2_" + name] = partner, d2
    return out


MLS_TEETH_ROWS = 7


def mls_rows(c, rule="contract", rows=None):
    """mls_model's rows at order 2 (they carry the plane's result too)"""
    centres = c.pts if rows is None else c.pts[rows]
    return MM.project_cloud(c.pts, centres, c.radius(rule), GAUSS_H)


def mls_tie(m):
    """A row of mls_rows whose two smallest eigenvalues tie: a symmetric lattice neighbourhood (all of full9's interior), whose normal
    is ANY vector of a plane or of space.  The quadric's frame and with it its pivots follow that choice -- of the 84 such rows on
    full9's edges at sqrt 3 S numpy's eigenvector gives fit 2 on 69 and fit 1 on 15 -- so the contract fixes the count there, fit >= 1,
    and nothing else.  Fewer than 6 points never form a system: those rows are not meant."""
    return m.count >= 6 and not m.gap > 2.0 ** -20 * m.evals[2]


def _mls(c, rule):
    """counts of every sampled row; fit words where the contract's row is no tie (255 elsewhere: not compared)"""
    at = np.arange(0, c.n, MLS_TEETH_ROWS)
    tie = np.array([mls_tie(m) for m in mls_rows(c, "contract", at)])
    rows = mls_rows(c, rule, at)
    fit = np.where(tie, 255, np.array([m.fit for m in rows])).astype(np.uint8)
    return {"counts": np.array([m.count for m in rows], np.uint32), "fit_order1": np.minimum(fit, np.where(tie, 255, 1)).astype(np.uint8),
            "fit_order2": fit}


BOUNDARY_NAMES = ("keep", "gap", "count", "sectors")
BOUNDARY_NORMALS = ("normals", "flat")  # seeded ones, and (0, 0, 1): lattice directions exactly on sector borders


def _boundary(c, rule):
    out = {}
    for which in BOUNDARY_NORMALS:
        got = BoM.boundary(c.pts, c.I[which], c.radius(rule))
        out.update({"%s_%s" % (name, which): np.ascontiguousarray(a) for name, a in zip(BOUNDARY_NAMES, got)})
    return out


Row = collections.namedtuple("Row", "model exact fixed")
ROWS = {
    "counts": Row(_counts, ("self", "absent", "keep_interior", "keep_median"), ()),
    "lists": Row(_lists, ("offsets", "idx", "batch_offsets", "batch_idx"), ()),
    "neighbourhoods": Row(_set_counts, ("counts_self", "counts_batch"), ()),
    "features": Row(_set_counts, ("counts_self", "counts_batch"), ()),
    "cluster": Row(_cluster, ("counts",) + tuple(k + cluster_tag(m, cp) for m, cp in CLUSTER_FORMS
                                                 for k in (("labels", "count") if m == "m1" else ("labels", "count", "core"))), ()),
    "segment": Row(_segment, ("labels", "count", "gated_labels", "gated_count"), ("gated_smooth",)),
    "subsample": Row(_subsample, ("keep", "owner"), ()),
    "local_maxima": Row(_local_maxima, ("keep",), ()),
    "iss": Row(_iss, ("passes", "keep"), ()),
    "fpfh": Row(_fpfh_teeth, ("spfh", "pairs"), ()),
    "nearest_posed": Row(_nearest, tuple(k + "_" + p for p in POSES for k in ("partner", "d2")), ()),
    "mls": Row(_mls, ("counts", "fit_order1", "fit_order2"), ()),
    "boundary": Row(_boundary, tuple("%s_%s" % (k, w) for w in BOUNDARY_NORMALS for k in BOUNDARY_NAMES), ()),
}
MIXED = ("lists", "neighbourhoods", "features")  # rows with a mixed-radii batch form: every wrong rule changes some sphere of it


def differing_rules(row, rname):
    """the wrong rules under which a row's model must answer differently at a radius"""
    return [rule for rule in WRONG if row in MIXED or bound(rname, rule) != bound(rname)]


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    view = {4: np.uint32, 8: np.uint64}.get(a.dtype.itemsize) if a.dtype.kind == "f" else None
    return np.array_equal(a.view(view), b.view(view)) if view else np.array_equal(a, b)


# ---- farthest points ------------------------------------------------------------------------------------------------------------------------
FPS_CLOUD, FPS_START = "full9", 0
FPS_STOP = float(F(2) * F(S))  # the selection goes on while D > 4 S^2 and ends at D == 4 S^2


@functools.lru_cache(maxsize=None)
def fps_case():
    """(points, m, the model's result)"""
    pts = points(FPS_CLOUD)
    return pts, len(pts), FM.fps(pts, len(pts), start=FPS_START, stop_radius=FPS_STOP)
