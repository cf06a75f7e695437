"""A numpy restatement of the reference's naive surface nets (include/pcp/algorithm/surface_nets.hpp:357-650, the overload
that marches over the whole grid) for the tests: every grid cube once, the reference's arithmetic in float32, its output
order canonicalised by cube index (vertices by ascending i + j*sx + k*sx*sy, triangles by (cube, quad 0..2, triangle 0..1)).

It is a test model, not a code path of the library."""
import numpy as np

F = np.float32
# corner q of a cube at offset CORNERS[q] (get_voxel_corner_grid_positions) and the reference's edges table
CORNERS = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
EDGES = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]
NO_VERTEX = np.uint32(0xFFFFFFFF)


def _g(grid, name):
    return grid[name] if isinstance(grid, dict) else getattr(grid, name)


def _corner_values(Fd, k0, k1, sx, sy):
    """The 8 corner values of the cubes of slab k0 <= k < k1, each (k1-k0, sy, sx)."""
    return [Fd[k0 + dk:k1 + dk, dj:dj + sy, di:di + sx] for (di, dj, dk) in CORNERS]


def surface_nets(field, grid, isovalue=0.0, slab=32):
    """(vertices (V,3) float32, triangles (T,3) uint32)."""
    sx, sy, sz = int(_g(grid, "sx")), int(_g(grid, "sy")), int(_g(grid, "sz"))
    if sx == 0 or sy == 0 or sz == 0:
        return np.zeros((0, 3), F), np.zeros((0, 3), np.uint32)
    gx, gy, gz = F(_g(grid, "x")), F(_g(grid, "y")), F(_g(grid, "z"))
    dx, dy, dz = F(_g(grid, "dx")), F(_g(grid, "dy")), F(_g(grid, "dz"))
    iso = F(isovalue)
    Fd = np.ascontiguousarray(field, F).reshape(sz + 1, sy + 1, sx + 1)
    ncubes = sx * sy * sz
    cmap = np.full(ncubes, NO_VERTEX, np.uint32)
    # mesh_aabb = {get_world_point_of(0,0,0), get_world_point_of(sx,sy,sz)}
    mn = [gx + F(0) * dx, gy + F(0) * dy, gz + F(0) * dz]
    mx = [gx + F(sx) * dx, gy + F(sy) * dy, gz + F(sz) * dz]
    sdim = [F(sx), F(sy), F(sz)]
    verts, nv = [], 0
    with np.errstate(all="ignore"):
        for k0 in range(0, sz, slab):
            k1 = min(sz, k0 + slab)
            s = _corner_values(Fd, k0, k1, sx, sy)
            pos = [v >= iso for v in s]
            active = np.zeros_like(pos[0])
            for q in range(1, 8):
                active |= pos[q] != pos[0]
            kk, jj, ii = np.nonzero(active)
            kk = kk + k0
            lin = ii + jj * sx + kk * (sx * sy)  # nonzero returns C order: ascending linear index
            cmap[lin] = np.arange(nv, nv + len(lin), dtype=np.uint32)
            nv += len(lin)
            sv = [v[active] for v in s]
            pv = [v[active] for v in pos]
            fi, fj, fk = ii.astype(F), jj.astype(F), kk.astype(F)
            base = [(fi, fj, fk), (fi + F(1), fj, fk), (fi + F(1), fj + F(1), fk), (fi, fj + F(1), fk),
                    (fi, fj, fk + F(1)), (fi + F(1), fj, fk + F(1)), (fi + F(1), fj + F(1), fk + F(1)), (fi, fj + F(1), fk + F(1))]
            acc = [np.zeros(len(lin), F) for _ in range(3)]
            n = np.zeros(len(lin), np.int64)
            for a, b in EDGES:
                bip = pv[a] != pv[b]
                t = (iso - sv[a]) / (sv[b] - sv[a])
                for ax in range(3):
                    q = base[a][ax] + t * (base[b][ax] - base[a][ax])
                    acc[ax] = np.where(bip, acc[ax] + q, acc[ax])
                n += bip
            fn = n.astype(F)
            c = [acc[ax] / fn for ax in range(3)]
            verts.append(np.stack([mn[ax] + (mx[ax] - mn[ax]) * (c[ax] - F(0)) / (sdim[ax] - F(0)) for ax in range(3)], axis=1).astype(F))
        vertices = np.concatenate(verts) if verts else np.zeros((0, 3), F)
        # triangles: active cubes with i, j, k >= 1, three quads over the neighbour table of surface_nets.hpp:549-586
        act = np.nonzero(cmap != NO_VERTEX)[0]
        tris = []
        for lo in range(0, len(act), 1 << 22):
            c = act[lo:lo + (1 << 22)].astype(np.int64)
            i, j, k = c % sx, (c // sx) % sy, c // (sx * sy)
            keep = (i > 0) & (j > 0) & (k > 0)
            c, i, j, k = c[keep], i[keep], j[keep], k[keep]
            sxy = sx * sy
            nb = [cmap[c - 1], cmap[c - 1 - sx], cmap[c - sx], cmap[c - sx - sxy], cmap[c - sxy], cmap[c - 1 - sxy]]
            quads = [(0, 1, 2), (0, 5, 4), (2, 3, 4)]
            s0 = Fd[k, j, i]
            e = [(s0, Fd[k + 1, j, i]), (Fd[k, j + 1, i], s0), (s0, Fd[k, j, i + 1])]
            v0 = cmap[c]
            out = np.zeros((len(c), 3, 2, 3), np.uint32)
            valid = np.zeros((len(c), 3), bool)
            for qi, (a, b, d) in enumerate(quads):
                na, nb_, nd = nb[a], nb[b], nb[d]
                valid[:, qi] = (na != NO_VERTEX) & (nb_ != NO_VERTEX) & (nd != NO_VERTEX)
                fwd = e[qi][1] > e[qi][0]
                v1 = np.where(fwd, na, nd)
                v2 = nb_
                v3 = np.where(fwd, nd, na)
                out[:, qi, 0] = np.stack([v0, v1, v2], 1)
                out[:, qi, 1] = np.stack([v0, v2, v3], 1)
            tris.append(out[np.repeat(valid[:, :, None], 2, axis=2)].reshape(-1, 3))
        triangles = np.concatenate(tris) if tris else np.zeros((0, 3), np.uint32)
    return vertices, triangles.astype(np.uint32)


def grid_dict(x, y, z, dx, dy, dz, sx, sy, sz):
    return dict(x=F(x), y=F(y), z=F(z), dx=F(dx), dy=F(dy), dz=F(dz), sx=int(sx), sy=int(sy), sz=int(sz))


def regular_grid_containing(mn, mx, dims):
    """regular_grid3d.hpp:63-90 in float32, quirk included (every axis moves back by dx)."""
    mn = np.asarray(mn, F)
    mx = np.asarray(mx, F)
    dx = (mx[0] - mn[0]) / F(dims[0])
    dy = (mx[1] - mn[1]) / F(dims[1])
    dz = (mx[2] - mn[2]) / F(dims[2])
    return grid_dict(mn[0] - dx, mn[1] - dx, mn[2] - dx, dx, dy, dz, dims[0] + 2, dims[1] + 2, dims[2] + 2)


def corner_positions(grid):
    """World positions of every corner in field order, as get_world_point_of."""
    sx, sy, sz = int(_g(grid, "sx")), int(_g(grid, "sy")), int(_g(grid, "sz"))
    x = F(_g(grid, "x")) + np.arange(sx + 1).astype(F) * F(_g(grid, "dx"))
    y = F(_g(grid, "y")) + np.arange(sy + 1).astype(F) * F(_g(grid, "dy"))
    z = F(_g(grid, "z")) + np.arange(sz + 1).astype(F) * F(_g(grid, "dz"))
    zz, yy, xx = np.meshgrid(z, y, x, indexing="ij")
    return np.stack([xx.ravel(), yy.ravel(), zz.ravel()], 1).astype(F)


def sphere_field(grid, r=1.0, c=(0.0, 0.0, 0.0)):
    p = corner_positions(grid) - np.asarray(c, F)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return (np.sqrt(x * x + y * y + z * z) - F(r)).astype(F)
