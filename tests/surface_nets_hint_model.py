"""A restatement of the reference's hint-seeded surface nets (include/pcp/algorithm/surface_nets.hpp:653-1119, the overload
with a hint point) for the tests, on a field given at the grid's corners, with the divergences the library documents
(DESIGN.md section 15):
  - cubes are keyed by (i, j, k) and cubes outside the grid are never active (the reference walks linear indices across
    faces and evaluates f outside the grid);
  - the hint cube is floor((p - o) / d) in float32 (the reference truncates, which is the same for values >= 0);
  - if the first search pops POP_CAP cubes without meeting the queue bound or an active cube, the seed is the active cube
    nearest the hint cube in Manhattan distance, the smallest cube index on a tie.
The first search is the literal queue: visited marked on pop, duplicates pushed, `size == queue_max` checked before every
pop.  The second search runs over active grid cubes through their bipolar edges.  Vertices are computed with the
reference's arithmetic and returned with their cubes, in the reference's (search) order.

It is a test model, not a code path of the library."""
from collections import deque

import numpy as np

import surface_nets_model as M

F = np.float32
POP_CAP = 1 << 20
CORNERS, EDGES = M.CORNERS, M.EDGES
# adjacent_cubes_of_edges (surface_nets.hpp:853-866)
EDGE_CUBES = [((0, -1, 0), (0, -1, -1), (0, 0, -1)), ((1, 0, 0), (1, 0, -1), (0, 0, -1)), ((0, 1, 0), (0, 1, -1), (0, 0, -1)),
              ((-1, 0, 0), (-1, 0, -1), (0, 0, -1)), ((0, -1, 0), (0, -1, 1), (0, 0, 1)), ((1, 0, 0), (1, 0, 1), (0, 0, 1)),
              ((0, 1, 0), (0, 1, 1), (0, 0, 1)), ((-1, 0, 0), (-1, 0, 1), (0, 0, 1)), ((-1, 0, 0), (-1, -1, 0), (0, -1, 0)),
              ((1, 0, 0), (1, -1, 0), (0, -1, 0)), ((1, 0, 0), (1, 1, 0), (0, 1, 0)), ((-1, 0, 0), (-1, 1, 0), (0, 1, 0))]
NEIGHBOURS6 = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]


def _g(grid, name):
    return grid[name] if isinstance(grid, dict) else getattr(grid, name)


def search_order(queue_max, pop_cap=POP_CAP):
    """The first search on an unbounded lattice with nothing active: (offsets of the distinct cubes in first-pop order,
    bounded).  bounded: the queue held exactly queue_max cubes before some pop, and the offsets end there."""
    q = deque([(0, 0, 0)])
    visited, order = set(), []
    for _ in range(pop_cap):
        if len(q) == queue_max:
            return order, True
        c = q.popleft()
        if c not in visited:
            visited.add(c)
            order.append(c)
        for d in NEIGHBOURS6:
            n = (c[0] + d[0], c[1] + d[1], c[2] + d[2])
            if n not in visited:
                q.append(n)
    return order, False


def hint_cube(hint, grid):
    return tuple(int(np.floor((F(hint[a]) - F(_g(grid, n))) / F(_g(grid, "d" + n)))) for a, n in enumerate("xyz"))


class _Field:
    def __init__(self, field, grid, isovalue):
        self.sx, self.sy, self.sz = int(_g(grid, "sx")), int(_g(grid, "sy")), int(_g(grid, "sz"))
        self.Fd = np.ascontiguousarray(field, F).reshape(self.sz + 1, self.sy + 1, self.sx + 1)
        self.iso = F(isovalue)
        self.grid = grid
        pos = self.Fd >= self.iso
        s = [pos[dk:dk + self.sz, dj:dj + self.sy, di:di + self.sx] for (di, dj, dk) in CORNERS]
        act = np.zeros_like(s[0])
        for q in range(1, 8):
            act |= s[q] != s[0]
        self.active = act  # (sz, sy, sx)

    def inside(self, c):
        return 0 <= c[0] < self.sx and 0 <= c[1] < self.sy and 0 <= c[2] < self.sz

    def is_active(self, c):
        return self.inside(c) and bool(self.active[c[2], c[1], c[0]])

    def values(self, c):
        i, j, k = c
        return [self.Fd[k + dk, j + dj, i + di] for (di, dj, dk) in CORNERS]

    def lin(self, c):
        return c[0] + c[1] * self.sx + c[2] * self.sx * self.sy


def find_seed(fm, hint, queue_max, pop_cap=POP_CAP):
    """The seed cube (i, j, k), or None for the whole-grid fallback / no active cube."""
    h = hint_cube(hint, fm.grid)
    q = deque([h])
    visited = set()
    for _ in range(pop_cap):
        if len(q) == queue_max:
            return None
        c = q.popleft()
        visited.add(c)
        if fm.is_active(c):
            return c
        for d in NEIGHBOURS6:
            n = (c[0] + d[0], c[1] + d[1], c[2] + d[2])
            if n not in visited:
                q.append(n)
    kk, jj, ii = np.nonzero(fm.active)
    if len(ii) == 0:
        return None
    dist = np.abs(ii - h[0]) + np.abs(jj - h[1]) + np.abs(kk - h[2])
    lin = ii + jj * fm.sx + kk * fm.sx * fm.sy
    best = np.lexsort((lin, dist))[0]
    return (int(ii[best]), int(jj[best]), int(kk[best]))


def _vertex(fm, c):
    """surface_nets.hpp:930-1017 for one cube, float32."""
    s = fm.values(c)
    iso = fm.iso
    i, j, k = (F(v) for v in c)
    p = [(i, j, k), (i + F(1), j, k), (i + F(1), j + F(1), k), (i, j + F(1), k), (i, j, k + F(1)), (i + F(1), j, k + F(1)),
         (i + F(1), j + F(1), k + F(1)), (i, j + F(1), k + F(1))]
    acc = [F(0), F(0), F(0)]
    n = 0
    for a, b in EDGES:
        if (s[a] >= iso) == (s[b] >= iso):
            continue
        t = (iso - s[a]) / (s[b] - s[a])
        for ax in range(3):
            acc[ax] = F(acc[ax] + F(p[a][ax] + F(t * F(p[b][ax] - p[a][ax]))))
        n += 1
    g = fm.grid
    o = [F(_g(g, "x")), F(_g(g, "y")), F(_g(g, "z"))]
    d = [F(_g(g, "dx")), F(_g(g, "dy")), F(_g(g, "dz"))]
    sd = [F(fm.sx), F(fm.sy), F(fm.sz)]
    out = []
    for ax in range(3):
        mn = F(o[ax] + F(0) * d[ax])
        mx = F(o[ax] + sd[ax] * d[ax])
        cen = F(acc[ax] / F(n))
        out.append(F(mn + F(F(F(mx - mn) * F(cen - F(0))) / F(sd[ax] - F(0)))))
    return out


def surface_nets_hint(field, grid, hint, isovalue=0.0, queue_max=32768, pop_cap=POP_CAP):
    """(vertices (V,3) float32, triangles (T,3) uint32, cubes (V,) linear cube index of every vertex, seed linear index or
    None).  None as seed: the whole-grid mesh (surface_nets_model.surface_nets) with every active cube."""
    fm = _Field(field, grid, isovalue)
    if min(fm.sx, fm.sy, fm.sz) == 0:
        return np.zeros((0, 3), F), np.zeros((0, 3), np.uint32), np.zeros(0, np.int64), None
    seed = find_seed(fm, hint, queue_max, pop_cap)
    if seed is None:
        v, t = M.surface_nets(field, grid, isovalue)
        kk, jj, ii = np.nonzero(fm.active)
        return v, t, (ii + jj * fm.sx + kk * fm.sx * fm.sy).astype(np.int64), None
    iso = fm.iso
    comp = {}
    verts, cubes = [], []
    q = deque([seed])
    with np.errstate(all="ignore"):
        while q:
            c = q.popleft()
            if c in comp:
                continue
            s = fm.values(c)
            for e, (a, b) in enumerate(EDGES):
                if (s[a] >= iso) == (s[b] >= iso):
                    continue
                for d in EDGE_CUBES[e]:
                    n = (c[0] + d[0], c[1] + d[1], c[2] + d[2])
                    if fm.inside(n) and n not in comp:
                        q.append(n)
            comp[c] = len(verts)
            verts.append(_vertex(fm, c))
            cubes.append(fm.lin(c))
        tris = []
        for c, v0 in comp.items():  # surface_nets.hpp:1036-1115, the quad rule over the component map
            i, j, k = c
            if i == 0 or j == 0 or k == 0:
                continue
            nb = [(i - 1, j, k), (i - 1, j - 1, k), (i, j - 1, k), (i, j - 1, k - 1), (i, j, k - 1), (i - 1, j, k - 1)]
            Fd = fm.Fd
            edge = [(Fd[k, j, i], Fd[k + 1, j, i]), (Fd[k, j + 1, i], Fd[k, j, i]), (Fd[k, j, i], Fd[k, j, i + 1])]
            for qi, quad in enumerate(((0, 1, 2), (0, 5, 4), (2, 3, 4))):
                if any(nb[x] not in comp for x in quad):
                    continue
                nv = [comp[nb[x]] for x in quad]
                order = (0, 1, 2) if edge[qi][1] > edge[qi][0] else (2, 1, 0)
                v1, v2, v3 = nv[order[0]], nv[order[1]], nv[order[2]]
                tris.append((v0, v1, v2))
                tris.append((v0, v2, v3))
    return (np.asarray(verts, F).reshape(-1, 3), np.asarray(tris, np.uint32).reshape(-1, 3), np.asarray(cubes, np.int64),
            fm.lin(seed))


def canonical(vertices, triangles, cubes):
    """A mesh keyed by cube: vertices sorted by cube, triangles as cube triples grouped by their first cube (stable, so each
    cube's quads keep their order).  The library's output is already in this order."""
    order = np.argsort(cubes, kind="stable")
    tc = cubes[triangles.astype(np.int64)] if len(triangles) else np.zeros((0, 3), np.int64)
    torder = np.argsort(tc[:, 0], kind="stable") if len(tc) else np.zeros(0, np.int64)
    return vertices[order], cubes[order], tc[torder]


def active_cubes(field, grid, isovalue=0.0):
    """Linear indices of the active cubes, ascending (the vertex order of the whole-grid mesh)."""
    fm = _Field(field, grid, isovalue)
    kk, jj, ii = np.nonzero(fm.active)
    return (ii + jj * fm.sx + kk * fm.sx * fm.sy).astype(np.int64)


def restrict(vertices, triangles, cubes, keep):
    """The whole-grid mesh (vertices in ascending cube order `cubes`) restricted to the cubes where `keep` (per vertex) holds:
    those vertices, and the quads -- consecutive triangle pairs -- whose four cubes are all kept, indices remapped."""
    keep = np.asarray(keep, bool)
    remap = np.full(len(vertices), -1, np.int64)
    remap[keep] = np.arange(int(keep.sum()))
    t = triangles.astype(np.int64).reshape(-1, 2, 3)
    pair_ok = keep[t].reshape(len(t), -1).all(1)
    kept = t[pair_ok].reshape(-1, 3)
    return vertices[keep], remap[kept].astype(np.uint32), cubes[keep]
