// pcpx_isosurface.hip -- tangent-plane surface reconstruction: the signed-distance field at the corners of a regular grid and
// naive surface nets over it (include/pcp/algorithm/surface_nets.hpp:357-650 of the reference, the overload that marches
// over the whole grid).
//
// Field: every grid corner is a kNN query (k = 1) through the index's query path; a small kernel turns the nearest point's
// tangent plane into dot(c - o, n).  Corners are enumerated in 4x4x4 bricks, so the queries handed to the query sort arrive
// spatially coherent.
//
// Surface nets, three passes with device scans and no atomics, so the output order is fixed:
//   1. one thread per cube: active flag (some edge bipolar);  exclusive scan -> vertex index of every active cube, in
//      ascending linear cube index i + j*sx + k*sx*sy;
//   2. one thread per cube: dense cube -> vertex map (UINT32_MAX = inactive), list of active cubes, vertex position;
//   3. one thread per active cube: triangle count;  scan;  the same thread again: the triangles, in (cube, quad 0..2,
//      triangle 0..1) order.
// The vertex arithmetic is the reference's operation for operation; the build's -ffp-contract=off keeps it unfused.
//
// Hint-seeded surface nets (:653-1119 of the reference): the same passes restricted to one connected
// component of the active cubes, found by a table-driven seed search and union-find labelling.
#include "pcpx_internal.h"
#include "pcpx_scan.h"
#include "pcpx_unionfind.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <deque>
#include <map>
#include <unordered_set>

namespace pcpx {

namespace {

constexpr int SN_BLOCK = 256;
constexpr u32 SN_MAX_BLOCKS = 8192;  // grid-stride beyond this: 256 CUs x 32 blocks of 256 threads cover the card many times over
constexpr u32 NO_VERTEX = 0xFFFFFFFFu;

u32 blocks_for(u64 n)
{
    const u64 b = (n + SN_BLOCK - 1) / SN_BLOCK;
    return static_cast<u32>(b < SN_MAX_BLOCKS ? (b > 0 ? b : 1) : SN_MAX_BLOCKS);
}

struct GridDev {
    float x, y, z, dx, dy, dz;
    u32 sx, sy, sz;  // cubes per axis; sx*sy*sz < 2^32
};

__device__ __forceinline__ u64 corner_at(const GridDev& g, u32 i, u32 j, u32 k)
{
    return static_cast<u64>(i) + static_cast<u64>(g.sx + 1) * (static_cast<u64>(j) + static_cast<u64>(g.sy + 1) * k);
}

// get_world_point_of (surface_nets.hpp:31-41)
__device__ __forceinline__ float3 world_of(const GridDev& g, u32 i, u32 j, u32 k)
{
    return make_float3(g.x + static_cast<float>(i) * g.dx, g.y + static_cast<float>(j) * g.dy, g.z + static_cast<float>(k) * g.dz);
}

// ---- tangent-plane distance field ---------------------------------------------------------------------------------------

struct Bricks {
    u32 bx, by, bz;  // bricks per axis over the (sx+1) x (sy+1) x (sz+1) corners
};

// corner of brick-order query p (clamped into the grid for the padding of partial bricks; `inside` tells which)
__device__ __forceinline__ void brick_corner(const GridDev& g, const Bricks& b, u64 p, u32& i, u32& j, u32& k, bool& inside)
{
    const u64 brick = p >> 6;
    const u32 r = static_cast<u32>(p & 63u);
    const u64 bxy = static_cast<u64>(b.bx) * b.by;
    i = static_cast<u32>(brick % b.bx) * 4u + (r & 3u);
    j = static_cast<u32>((brick / b.bx) % b.by) * 4u + ((r >> 2) & 3u);
    k = static_cast<u32>(brick / bxy) * 4u + (r >> 4);
    inside = i <= g.sx && j <= g.sy && k <= g.sz;
    i = i <= g.sx ? i : g.sx;
    j = j <= g.sy ? j : g.sy;
    k = k <= g.sz ? k : g.sz;
}

__global__ __launch_bounds__(SN_BLOCK) void k_sdf_queries(GridDev g, Bricks b, u64 nq, float* __restrict__ q)
{
    for (u64 p = static_cast<u64>(blockIdx.x) * SN_BLOCK + threadIdx.x; p < nq; p += static_cast<u64>(gridDim.x) * SN_BLOCK) {
        u32 i, j, k;
        bool inside;
        brick_corner(g, b, p, i, j, k, inside);
        const float3 c = world_of(g, i, j, k);
        q[3 * p] = c.x;
        q[3 * p + 1] = c.y;
        q[3 * p + 2] = c.z;
    }
}

// field[corner] = inner_product(c - o, n) of the nearest point's plane (common/norm.hpp:34: n.x * op.x + ..., left to right);
// NaN where no point is outside the eps-box of the corner (the reference would dereference an empty neighbour list)
__global__ __launch_bounds__(SN_BLOCK) void k_sdf_eval(GridDev g, Bricks b, u64 nq, const u32* __restrict__ nn, const u32* __restrict__ cnt,
                                                       const float* __restrict__ centroids, const float* __restrict__ normals,
                                                       float* __restrict__ field)
{
    for (u64 p = static_cast<u64>(blockIdx.x) * SN_BLOCK + threadIdx.x; p < nq; p += static_cast<u64>(gridDim.x) * SN_BLOCK) {
        u32 i, j, k;
        bool inside;
        brick_corner(g, b, p, i, j, k, inside);
        if (!inside) continue;
        float v = __builtin_nanf("");
        if (cnt[p] > 0) {
            const u64 o = nn[p];
            const float3 c = world_of(g, i, j, k);
            const float opx = c.x - centroids[3 * o], opy = c.y - centroids[3 * o + 1], opz = c.z - centroids[3 * o + 2];
            const float xx = normals[3 * o] * opx, yy = normals[3 * o + 1] * opy, zz = normals[3 * o + 2] * opz;
            v = xx + yy + zz;
        }
        field[corner_at(g, i, j, k)] = v;
    }
}

// ---- surface nets -------------------------------------------------------------------------------------------------------

// the reference's `edges` table (surface_nets.hpp:453-465) over the corner order of get_voxel_corner_grid_positions
__constant__ unsigned char c_edges[12][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 0}, {4, 5}, {5, 6}, {6, 7}, {7, 4}, {0, 4}, {1, 5}, {2, 6}, {3, 7}};

__device__ __forceinline__ void cube_of(const GridDev& g, u32 c, u32& i, u32& j, u32& k)
{
    i = c % g.sx;
    j = (c / g.sx) % g.sy;
    k = c / (g.sx * g.sy);
}

__device__ __forceinline__ void cube_corners(const GridDev& g, const float* __restrict__ f, u32 i, u32 j, u32 k, float s[8])
{
    const u64 X = g.sx + 1u, XY = X * (g.sy + 1u);
    const u64 c0 = corner_at(g, i, j, k);
    s[0] = f[c0];
    s[1] = f[c0 + 1];
    s[2] = f[c0 + 1 + X];
    s[3] = f[c0 + X];
    s[4] = f[c0 + XY];
    s[5] = f[c0 + 1 + XY];
    s[6] = f[c0 + 1 + X + XY];
    s[7] = f[c0 + X + XY];
}

// active iff some edge is bipolar; the 12 edges connect all 8 corners, so: iff the corners are not all on one side
__device__ __forceinline__ bool cube_active(const float s[8], float iso)
{
    const bool p0 = s[0] >= iso;
    bool mixed = false;
#pragma unroll
    for (int q = 1; q < 8; ++q) mixed |= (s[q] >= iso) != p0;
    return mixed;
}

__global__ __launch_bounds__(SN_BLOCK) void k_sn_flags(GridDev g, u32 ncubes, const float* __restrict__ field, float iso,
                                                       u32* __restrict__ flag)
{
    for (u64 c64 = static_cast<u64>(blockIdx.x) * SN_BLOCK + threadIdx.x; c64 < ncubes; c64 += static_cast<u64>(gridDim.x) * SN_BLOCK) {
        const u32 c = static_cast<u32>(c64);
        u32 i, j, k;
        cube_of(g, c, i, j, k);
        float s[8];
        cube_corners(g, field, i, j, k, s);
        flag[c] = cube_active(s, iso) ? 1u : 0u;
    }
}

// the mesh vertex of an active cube (surface_nets.hpp:467-519): centroid of the edge crossings in grid coordinates, then
// mapped into mesh_aabb
__device__ __forceinline__ float3 cube_vertex(const GridDev& g, u32 i, u32 j, u32 k, const float s[8], float iso)
{
    const float fi = static_cast<float>(i), fj = static_cast<float>(j), fk = static_cast<float>(k);
    const float fi1 = fi + 1.f, fj1 = fj + 1.f, fk1 = fk + 1.f;
    const float px[8] = {fi, fi1, fi1, fi, fi, fi1, fi1, fi};
    const float py[8] = {fj, fj, fj1, fj1, fj, fj, fj1, fj1};
    const float pz[8] = {fk, fk, fk, fk, fk1, fk1, fk1, fk1};
    float sx = 0.f, sy = 0.f, sz = 0.f;
    int n = 0;
#pragma unroll
    for (int e = 0; e < 12; ++e) {
        const int a = c_edges[e][0], b = c_edges[e][1];
        if ((s[a] >= iso) == (s[b] >= iso)) continue;
        const float t = (iso - s[a]) / (s[b] - s[a]);
        // p1 + t * (p2 - p1), then accumulated from point_type{} (vector3d_queries.hpp:79-99)
        sx = sx + (px[a] + t * (px[b] - px[a]));
        sy = sy + (py[a] + t * (py[b] - py[a]));
        sz = sz + (pz[a] + t * (pz[b] - pz[a]));
        ++n;
    }
    const float fn = static_cast<float>(n);
    const float cx = sx / fn, cy = sy / fn, cz = sz / fn;
    // mesh_aabb = {get_world_point_of(0, 0, 0), get_world_point_of(sx, sy, sz)}
    const float minx = g.x + 0.f * g.dx, miny = g.y + 0.f * g.dy, minz = g.z + 0.f * g.dz;
    const float maxx = g.x + static_cast<float>(g.sx) * g.dx, maxy = g.y + static_cast<float>(g.sy) * g.dy,
                maxz = g.z + static_cast<float>(g.sz) * g.dz;
    return make_float3(minx + (maxx - minx) * (cx - 0.f) / (static_cast<float>(g.sx) - 0.f),
                       miny + (maxy - miny) * (cy - 0.f) / (static_cast<float>(g.sy) - 0.f),
                       minz + (maxz - minz) * (cz - 0.f) / (static_cast<float>(g.sz) - 0.f));
}

// vofs: the exclusive scan of the flags (ncubes + 1 entries); an active cube c has vofs[c + 1] != vofs[c]
__global__ __launch_bounds__(SN_BLOCK) void k_sn_vertices(GridDev g, u32 ncubes, const float* __restrict__ field, float iso,
                                                          const u32* __restrict__ vofs, u32* __restrict__ map, u32* __restrict__ active,
                                                          float* __restrict__ out_xyz)
{
    for (u64 c64 = static_cast<u64>(blockIdx.x) * SN_BLOCK + threadIdx.x; c64 < ncubes; c64 += static_cast<u64>(gridDim.x) * SN_BLOCK) {
        const u32 c = static_cast<u32>(c64);
        const u32 v = vofs[c];
        const bool on = vofs[c + 1] != v;
        map[c] = on ? v : NO_VERTEX;
        if (!on) continue;
        active[v] = c;
        if (!out_xyz) continue;
        u32 i, j, k;
        cube_of(g, c, i, j, k);
        float s[8];
        cube_corners(g, field, i, j, k, s);
        const float3 p = cube_vertex(g, i, j, k, s, iso);
        out_xyz[3ull * v] = p.x;
        out_xyz[3ull * v + 1] = p.y;
        out_xyz[3ull * v + 2] = p.z;
    }
}

// neighbours of cube (i, j, k) in the reference's order (surface_nets.hpp:549-556) and the three quads over them (:586)
__device__ __forceinline__ void quad_vertices(const GridDev& g, const u32* __restrict__ map, u32 i, u32 j, u32 k, u32 nv[3][3])
{
    const u32 sx = g.sx, sxy = g.sx * g.sy;
    const u32 c = i + j * sx + k * sxy;
    const u32 n0 = map[c - 1], n1 = map[c - 1 - sx], n2 = map[c - sx], n3 = map[c - sx - sxy], n4 = map[c - sxy], n5 = map[c - 1 - sxy];
    nv[0][0] = n0, nv[0][1] = n1, nv[0][2] = n2;
    nv[1][0] = n0, nv[1][1] = n5, nv[1][2] = n4;
    nv[2][0] = n2, nv[2][1] = n3, nv[2][2] = n4;
}

__global__ __launch_bounds__(SN_BLOCK) void k_sn_tri_count(GridDev g, u32 nvert, const u32* __restrict__ active, const u32* __restrict__ map,
                                                           u64* __restrict__ tcnt)
{
    for (u64 v64 = static_cast<u64>(blockIdx.x) * SN_BLOCK + threadIdx.x; v64 < nvert; v64 += static_cast<u64>(gridDim.x) * SN_BLOCK) {
        const u32 v = static_cast<u32>(v64);
        u32 i, j, k;
        cube_of(g, active[v], i, j, k);
        u64 t = 0;
        if (i > 0 && j > 0 && k > 0) {
            u32 nv[3][3];
            quad_vertices(g, map, i, j, k, nv);
#pragma unroll
            for (int q = 0; q < 3; ++q) t += (nv[q][0] != NO_VERTEX && nv[q][1] != NO_VERTEX && nv[q][2] != NO_VERTEX) ? 2u : 0u;
        }
        tcnt[v] = t;
    }
}

__global__ __launch_bounds__(SN_BLOCK) void k_sn_triangles(GridDev g, u32 nvert, const float* __restrict__ field, const u32* __restrict__ active,
                                                           const u32* __restrict__ map, const u64* __restrict__ tofs, u32* __restrict__ out_tri)
{
    for (u64 v64 = static_cast<u64>(blockIdx.x) * SN_BLOCK + threadIdx.x; v64 < nvert; v64 += static_cast<u64>(gridDim.x) * SN_BLOCK) {
        const u32 v = static_cast<u32>(v64);
        u64 t = tofs[v64];
        if (tofs[v64 + 1] == t) continue;
        u32 i, j, k;
        cube_of(g, active[v], i, j, k);
        u32 nv[3][3];
        quad_vertices(g, map, i, j, k, nv);
        // the directed edges (0,4), (3,0), (0,1) of the cube (surface_nets.hpp:558-584)
        const float s0 = field[corner_at(g, i, j, k)], s4 = field[corner_at(g, i, j, k + 1)], s3 = field[corner_at(g, i, j + 1, k)],
                    s1 = field[corner_at(g, i + 1, j, k)];
        const float e0[3] = {s0, s3, s0}, e1[3] = {s4, s0, s1};
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            if (nv[q][0] == NO_VERTEX || nv[q][1] == NO_VERTEX || nv[q][2] == NO_VERTEX) continue;
            const bool fwd = e1[q] > e0[q];
            const u32 v1 = fwd ? nv[q][0] : nv[q][2], v2 = nv[q][1], v3 = fwd ? nv[q][2] : nv[q][0];
            u32* o = out_tri + 3 * t;
            o[0] = v, o[1] = v1, o[2] = v2;
            o[3] = v, o[4] = v2, o[5] = v3;
            t += 2;
        }
    }
}

// ---- hint-seeded surface nets: the seed, the components of the active cubes, the restriction -------------------------------

// the reference's adjacent_cubes_of_edges (surface_nets.hpp:853-866): the three other cubes around edge e of a cube
__constant__ signed char c_edge_cubes[12][3][3] = {
    {{0, -1, 0}, {0, -1, -1}, {0, 0, -1}}, {{1, 0, 0}, {1, 0, -1}, {0, 0, -1}},  {{0, 1, 0}, {0, 1, -1}, {0, 0, -1}},
    {{-1, 0, 0}, {-1, 0, -1}, {0, 0, -1}}, {{0, -1, 0}, {0, -1, 1}, {0, 0, 1}},  {{1, 0, 0}, {1, 0, 1}, {0, 0, 1}},
    {{0, 1, 0}, {0, 1, 1}, {0, 0, 1}},     {{-1, 0, 0}, {-1, 0, 1}, {0, 0, 1}},  {{-1, 0, 0}, {-1, -1, 0}, {0, -1, 0}},
    {{1, 0, 0}, {1, -1, 0}, {0, -1, 0}},   {{1, 0, 0}, {1, 1, 0}, {0, 1, 0}},    {{-1, 0, 0}, {-1, 1, 0}, {0, 1, 0}},
};

// the seed: the first table entry (offsets from the hint cube h, in the reference's first-pop order) that is an active cube of
// the grid.  One block; each thread stops at its own first hit, so the block minimum of the ranks is the first hit overall.
// seed[0] = its cube, or UINT64_MAX.
__global__ __launch_bounds__(SN_BLOCK) void k_hint_seed(GridDev g, const int* __restrict__ offsets, u32 n, long long hx, long long hy,
                                                        long long hz, const u32* __restrict__ map, unsigned long long* __restrict__ seed)
{
    __shared__ u32 best[SN_BLOCK];
    u32 mine = NO_VERTEX;
    for (u32 r = threadIdx.x; r < n; r += SN_BLOCK) {
        const long long i = hx + offsets[3 * r], j = hy + offsets[3 * r + 1], k = hz + offsets[3 * r + 2];
        if (i < 0 || j < 0 || k < 0 || i >= g.sx || j >= g.sy || k >= g.sz) continue;
        const u32 c = static_cast<u32>(i) + static_cast<u32>(j) * g.sx + static_cast<u32>(k) * (g.sx * g.sy);
        if (map[c] != NO_VERTEX) {
            mine = r;
            break;
        }
    }
    best[threadIdx.x] = mine;
    __syncthreads();
    for (int w = SN_BLOCK / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) best[threadIdx.x] = min(best[threadIdx.x], best[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const u32 r = best[0];
    if (r == NO_VERTEX) {
        seed[0] = ~0ull;
        return;
    }
    const u32 i = static_cast<u32>(hx + offsets[3 * r]), j = static_cast<u32>(hy + offsets[3 * r + 1]), k = static_cast<u32>(hz + offsets[3 * r + 2]);
    seed[0] = i + j * g.sx + k * (g.sx * g.sy);
}

// without a bound and with no table entry active: seed[1] = min over the active cubes of (Manhattan distance to the hint cube
// clamped into the grid) << 32 | cube -- the nearest to the hint cube itself, as the offset from the clamp is the same for every
// cube.  Does nothing when k_hint_seed found a seed (seed[0], written by the launch before).  One atomic per block.
__global__ __launch_bounds__(SN_BLOCK) void k_hint_nearest(GridDev g, u32 nvert, const u32* __restrict__ active, u32 cx, u32 cy, u32 cz,
                                                           unsigned long long* __restrict__ seed)
{
    __shared__ unsigned long long best[SN_BLOCK];
    unsigned long long mine = ~0ull;
    if (seed[0] == ~0ull) {
        for (u64 v = static_cast<u64>(blockIdx.x) * SN_BLOCK + threadIdx.x; v < nvert; v += static_cast<u64>(gridDim.x) * SN_BLOCK) {
            const u32 c = active[v];
            u32 i, j, k;
            cube_of(g, c, i, j, k);
            const u64 d = static_cast<u64>(i > cx ? i - cx : cx - i) + (j > cy ? j - cy : cy - j) + (k > cz ? k - cz : cz - k);
            mine = min(mine, static_cast<unsigned long long>(d << 32 | c));
        }
    }
    best[threadIdx.x] = mine;
    __syncthreads();
    for (int w = SN_BLOCK / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) best[threadIdx.x] = min(best[threadIdx.x], best[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0 && best[0] != ~0ull) atomicMin(seed + 1, best[0]);
}

// Connected components of the active cubes (two are adjacent iff they share a bipolar edge) by the union-find of
// pcpx_unionfind.h over active ranks: the final label of a component is its smallest active rank.
__global__ __launch_bounds__(SN_BLOCK) void k_cc_init(u32 nvert, u32* __restrict__ parent)
{
    for (u64 v = static_cast<u64>(blockIdx.x) * SN_BLOCK + threadIdx.x; v < nvert; v += static_cast<u64>(gridDim.x) * SN_BLOCK)
        parent[v] = static_cast<u32>(v);
}

// one thread per active cube: the in-grid cubes around its bipolar edges that come later in cube order (the earlier ones
// hook this pair from their side), each once -- a face neighbour shares four edges -- then a union with each
__global__ __launch_bounds__(SN_BLOCK) void k_cc_hook(GridDev g, u32 nvert, const float* __restrict__ field, float iso,
                                                      const u32* __restrict__ active, const u32* __restrict__ map, u32* parent)
{
    for (u64 v64 = static_cast<u64>(blockIdx.x) * SN_BLOCK + threadIdx.x; v64 < nvert; v64 += static_cast<u64>(gridDim.x) * SN_BLOCK) {
        const u32 v = static_cast<u32>(v64), c = active[v];
        u32 i, j, k;
        cube_of(g, c, i, j, k);
        float s[8];
        cube_corners(g, field, i, j, k, s);
        // bit (di+1) + 3(dj+1) + 9(dk+1) of the 3x3x3 block around the cube; bits 14..26 are the later cubes
        u32 around = 0;
        for (int e = 0; e < 12; ++e) {
            if ((s[c_edges[e][0]] >= iso) == (s[c_edges[e][1]] >= iso)) continue;
            for (int q = 0; q < 3; ++q)
                around |= 1u << ((c_edge_cubes[e][q][0] + 1) + 3 * (c_edge_cubes[e][q][1] + 1) + 9 * (c_edge_cubes[e][q][2] + 1));
        }
        around &= ~((1u << 14) - 1);
        while (around) {
            const int b = __builtin_ctz(around);
            around &= around - 1;
            const int di = b % 3 - 1, dj = (b / 3) % 3 - 1, dk = b / 9 - 1;
            if ((di < 0 && i == 0) || (dj < 0 && j == 0) || (di > 0 && i + 1 == g.sx) || (dj > 0 && j + 1 == g.sy) || (dk > 0 && k + 1 == g.sz))
                continue;  // (outside the grid; dk >= 0 here)
            const u32 u = map[(i + di) + (j + dj) * g.sx + (k + dk) * (g.sx * g.sy)];  // (a cube on a bipolar edge is active)
            if (u == NO_VERTEX) continue;
            (void)uf_unite(parent, v, u);
        }
    }
}

// parent[v] = the root of v, in a launch after the hooks: the roots are fixed.  The climb only READS (uf_find): a halving store
// that straddled thread x's own store of its root would put a non-root back into parent[x], and k_cc_restrict compares the
// words as roots.  With reads only, the one store to parent[v] in this launch is its root (pcpx_unionfind.h).
__global__ __launch_bounds__(SN_BLOCK) void k_cc_flatten(u32 nvert, u32* parent)
{
    for (u64 v = static_cast<u64>(blockIdx.x) * SN_BLOCK + threadIdx.x; v < nvert; v += static_cast<u64>(gridDim.x) * SN_BLOCK) {
        const u32 r = uf_find(parent, static_cast<u32>(v));
        __hip_atomic_store(parent + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// flag[c] = cube c is active and in the seed's component (label = the seed's root rank)
__global__ __launch_bounds__(SN_BLOCK) void k_cc_restrict(u32 ncubes, const u32* __restrict__ map, const u32* __restrict__ label, u32 seed_cube,
                                                          u32* __restrict__ flag)
{
    const u32 want = label[map[seed_cube]];
    for (u64 c = static_cast<u64>(blockIdx.x) * SN_BLOCK + threadIdx.x; c < ncubes; c += static_cast<u64>(gridDim.x) * SN_BLOCK) {
        const u32 m = map[c];
        flag[c] = m != NO_VERTEX && label[m] == want ? 1u : 0u;
    }
}

int grid_to_dev(const pcpx_grid3d& g, GridDev& d, u64& ncubes)
{
    ncubes = 0;
    if (g.sx == 0 || g.sy == 0 || g.sz == 0) return PCPX_OK;
    const u64 lim = 0xFFFFFFFFull;
    if (g.sx >= lim || g.sy >= lim || g.sz >= lim || g.sx * g.sy >= lim || g.sx * g.sy * g.sz >= lim) {
        set_error("pcpx: grid of %llu x %llu x %llu cubes: sx * sy * sz must be below 2^32", static_cast<unsigned long long>(g.sx),
                  static_cast<unsigned long long>(g.sy), static_cast<unsigned long long>(g.sz));
        return PCPX_ERR_INVALID;
    }
    d = GridDev{g.x, g.y, g.z, g.dx, g.dy, g.dz, static_cast<u32>(g.sx), static_cast<u32>(g.sy), static_cast<u32>(g.sz)};
    ncubes = g.sx * g.sy * g.sz;
    return PCPX_OK;
}

}  // namespace

int check_surface_grid(const pcpx_grid3d& grid)
{
    GridDev g{};
    u64 ncubes = 0;
    return grid_to_dev(grid, g, ncubes);
}

// events of a timed call, destroyed on every return
struct Events {
    hipEvent_t e[6] = {};
    int n = 0;
    int create(int count)
    {
        for (; n < count; ++n) PCPX_HIP(hipEventCreate(&e[n]));
        return PCPX_OK;
    }
    ~Events()
    {
        for (int q = 0; q < n; ++q) (void)hipEventDestroy(e[q]);
    }
};

// pass 1: flags, scanned in place into vertex offsets (ncubes + 1 entries); the number of active cubes in *nv.  ev_scanned (may
// be null) is recorded after the scan, ahead of the count's read-back.
int active_offsets(const GridDev& g, u64 ncubes, const float* d_field, float iso, hipStream_t s, u32* vofs, u32* sums, hipEvent_t ev_scanned,
                   u64* nv)
{
    PCPX_HIP(hipMemsetAsync(vofs + ncubes, 0, sizeof(u32), s));
    k_sn_flags<<<blocks_for(ncubes), SN_BLOCK, 0, s>>>(g, static_cast<u32>(ncubes), d_field, iso, vofs);
    PCPX_HIP(hipGetLastError());
    const int st = exclusive_scan_in_place<u32>(vofs, ncubes + 1, sums, s);
    if (st != PCPX_OK) return st;
    if (ev_scanned) PCPX_HIP(hipEventRecord(ev_scanned, s));
    u32 nv32 = 0;
    PCPX_HIP(hipMemcpyAsync(&nv32, vofs + ncubes, sizeof(u32), hipMemcpyDeviceToHost, s));
    PCPX_HIP(hipStreamSynchronize(s));
    *nv = nv32;
    return PCPX_OK;
}

// passes 2 and 3 over the cubes that `vofs` selects (nv of them): the map, the list, the vertices and the triangles, with the
// capacity protocol of surface_nets_device.  ev_vertices / ev_end (may be null) are recorded after the vertices and at the end.
int mesh_selected(const GridDev& g, u64 ncubes, const float* d_field, float iso, hipStream_t s, DevPool& pool, const u32* vofs, u32* map,
                  u64 nv, float* d_out_xyz, u64 vertex_capacity, u32* d_out_tri, u64 triangle_capacity, u64* out_nt, hipEvent_t ev_vertices,
                  hipEvent_t ev_end)
{
    int st;
    const u32 nc = static_cast<u32>(ncubes), nv32 = static_cast<u32>(nv);
    // pass 2: the map, the active cubes, and the vertices if they fit
    DevBuf active(pool), tofs(pool), tsums(pool);
    const u64 tiles_v = scan_tiles(nv + 1);
    if ((st = active.alloc(nv * sizeof(u32))) != PCPX_OK || (st = tofs.alloc((nv + 1) * sizeof(u64))) != PCPX_OK ||
        (st = tsums.alloc(std::max<u64>(tiles_v, 64) * sizeof(u64))) != PCPX_OK)
        return st;
    const bool write_vertices = d_out_xyz && nv <= vertex_capacity;
    k_sn_vertices<<<blocks_for(ncubes), SN_BLOCK, 0, s>>>(g, nc, d_field, iso, vofs, map, active.as<u32>(), write_vertices ? d_out_xyz : nullptr);
    PCPX_HIP(hipGetLastError());
    if (ev_vertices) PCPX_HIP(hipEventRecord(ev_vertices, s));
    // pass 3: triangle counts of the active cubes, scanned; then the triangles if they fit
    u64 nt = 0;
    if (nv > 0) {
        PCPX_HIP(hipMemsetAsync(tofs.as<u64>() + nv, 0, sizeof(u64), s));
        k_sn_tri_count<<<blocks_for(nv), SN_BLOCK, 0, s>>>(g, nv32, active.as<u32>(), map, tofs.as<u64>());
        PCPX_HIP(hipGetLastError());
        if ((st = exclusive_scan_in_place<u64>(tofs.as<u64>(), nv + 1, tsums.as<u64>(), s)) != PCPX_OK) return st;
        PCPX_HIP(hipMemcpyAsync(&nt, tofs.as<u64>() + nv, sizeof(u64), hipMemcpyDeviceToHost, s));
        PCPX_HIP(hipStreamSynchronize(s));
    }
    *out_nt = nt;
    const bool write_triangles = d_out_tri && nt <= triangle_capacity;
    if (nt > 0 && write_triangles) {
        k_sn_triangles<<<blocks_for(nv), SN_BLOCK, 0, s>>>(g, nv32, d_field, active.as<u32>(), map, tofs.as<u64>(), d_out_tri);
        PCPX_HIP(hipGetLastError());
    }
    if (ev_end) {
        PCPX_HIP(hipEventRecord(ev_end, s));
        PCPX_HIP(hipEventSynchronize(ev_end));
    }
    // the scratch goes back to the pool on return: nothing that reads it may still be queued
    PCPX_HIP(hipStreamSynchronize(s));
    if ((nv > 0 && !write_vertices) || (nt > 0 && !write_triangles)) {
        set_error("pcpx_surface_nets: the mesh has %llu vertices and %llu triangles", static_cast<unsigned long long>(nv),
                  static_cast<unsigned long long>(nt));
        return PCPX_ERR_CAPACITY;
    }
    return PCPX_OK;
}

int surface_nets_device(const float* d_field, const pcpx_grid3d& grid, float iso, hipStream_t s, DevPool& pool, float* d_out_xyz,
                        u64 vertex_capacity, u32* d_out_tri, u64 triangle_capacity, u64* out_nv, u64* out_nt, SurfaceNetsTimes* times)
{
    *out_nv = 0;
    *out_nt = 0;
    GridDev g{};
    u64 ncubes = 0;
    int st = grid_to_dev(grid, g, ncubes);
    if (st != PCPX_OK || ncubes == 0) return st;
    if (!d_field) {
        set_error("pcpx_surface_nets_dev: null field");
        return PCPX_ERR_INVALID;
    }
    Events ev;
    if (times && (st = ev.create(4)) != PCPX_OK) return st;
    DevBuf vofs(pool), sums(pool), map(pool);
    const u64 tiles_c = scan_tiles(ncubes + 1);
    if ((st = vofs.alloc((ncubes + 1) * sizeof(u32))) != PCPX_OK || (st = map.alloc(ncubes * sizeof(u32))) != PCPX_OK ||
        (st = sums.alloc(std::max<u64>(tiles_c, 64) * sizeof(u64))) != PCPX_OK)
        return st;
    if (times) PCPX_HIP(hipEventRecord(ev.e[0], s));
    if ((st = active_offsets(g, ncubes, d_field, iso, s, vofs.as<u32>(), sums.as<u32>(), ev.e[1], out_nv)) != PCPX_OK) return st;
    st = mesh_selected(g, ncubes, d_field, iso, s, pool, vofs.as<u32>(), map.as<u32>(), *out_nv, d_out_xyz, vertex_capacity, d_out_tri,
                       triangle_capacity, out_nt, ev.e[2], ev.e[3]);
    if (times && (st == PCPX_OK || st == PCPX_ERR_CAPACITY)) {
        PCPX_HIP(hipEventElapsedTime(&times->flags_ms, ev.e[0], ev.e[1]));
        PCPX_HIP(hipEventElapsedTime(&times->vertices_ms, ev.e[1], ev.e[2]));
        PCPX_HIP(hipEventElapsedTime(&times->triangles_ms, ev.e[2], ev.e[3]));
    }
    return st;
}

// ---- hint-seeded surface nets (surface_nets.hpp:653-1119 of the reference; the contract is DESIGN.md section 15) ------------

namespace {

constexpr u64 HINT_POP_CAP = 1ull << 20;  // pops of the simulated queue after which the search counts as unbounded

struct SearchOrder {
    std::vector<int> offsets;  // 3 per cube, in first-pop order
    bool bounded = false;
};

// The reference's first search (surface_nets.hpp:773-842) on an unbounded lattice with no active cube: pop, mark visited, push
// the six neighbours not yet visited (+x, -x, +y, -y, +z, -z), duplicates and all; before every pop, stop if the queue holds
// exactly queue_max cubes.  Returns the distinct cubes popped before the stop, or before HINT_POP_CAP pops (unbounded).
SearchOrder simulate_search(u64 queue_max)
{
    constexpr int B = 21;  // offsets stay within +-HINT_POP_CAP: 21 bits per axis, biased
    const auto key = [](long long i, long long j, long long k) {
        return (static_cast<u64>(i + (1 << 20)) << (2 * B)) | (static_cast<u64>(j + (1 << 20)) << B) | static_cast<u64>(k + (1 << 20));
    };
    SearchOrder out;
    std::deque<std::array<int, 3>> queue;
    std::unordered_set<u64> visited;
    queue.push_back({0, 0, 0});
    for (u64 pops = 0; pops < HINT_POP_CAP; ++pops) {
        if (queue.size() == queue_max) {
            out.bounded = true;
            break;
        }
        const std::array<int, 3> c = queue.front();
        queue.pop_front();
        if (visited.insert(key(c[0], c[1], c[2])).second) out.offsets.insert(out.offsets.end(), c.begin(), c.end());
        const std::array<int, 3> nb[6] = {{c[0] + 1, c[1], c[2]}, {c[0] - 1, c[1], c[2]}, {c[0], c[1] + 1, c[2]},
                                          {c[0], c[1] - 1, c[2]}, {c[0], c[1], c[2] + 1}, {c[0], c[1], c[2] - 1}};
        for (const auto& n : nb)
            if (!visited.count(key(n[0], n[1], n[2]))) queue.push_back(n);
    }
    return out;
}

// the table of queue_max, simulated once per process and value
const SearchOrder& search_order(u64 queue_max)
{
    static std::mutex mu;
    static std::map<u64, SearchOrder> tables;
    std::lock_guard<std::mutex> lock(mu);
    auto it = tables.find(queue_max);
    if (it == tables.end()) it = tables.emplace(queue_max, simulate_search(queue_max)).first;
    return it->second;
}

int surface_nets_hint_device(const float* d_field, const pcpx_grid3d& grid, float iso, const float hint[3], u64 queue_max, hipStream_t s,
                             DevPool& pool, float* d_out_xyz, u64 vertex_capacity, u32* d_out_tri, u64 triangle_capacity, u64* out_nv,
                             u64* out_nt, u64* out_seed, float* phase_ms, u32* rounds)
{
    *out_nv = 0;
    *out_nt = 0;
    *out_seed = UINT64_MAX;
    if (rounds) *rounds = 0;
    if (!std::isfinite(hint[0]) || !std::isfinite(hint[1]) || !std::isfinite(hint[2])) {
        set_error("pcpx_surface_nets_hint: the hint is not finite");
        return PCPX_ERR_INVALID;
    }
    GridDev g{};
    u64 ncubes = 0;
    int st = grid_to_dev(grid, g, ncubes);
    if (st != PCPX_OK || ncubes == 0) return st;
    if (!d_field) {
        set_error("pcpx_surface_nets_hint_dev: null field");
        return PCPX_ERR_INVALID;
    }
    // the hint cube: (p - o) / d per axis in float as get_grid_point_of, truncated -- floored, so negative values are defined too;
    // clamped far beyond the reach of any table so that the offsets below cannot overflow
    long long h[3];
    const float o[3] = {grid.x, grid.y, grid.z}, d[3] = {grid.dx, grid.dy, grid.dz};
    const u32 sz[3] = {g.sx, g.sy, g.sz};
    u32 hc[3];
    for (int a = 0; a < 3; ++a) {
        const float q = (hint[a] - o[a]) / d[a];
        if (std::isnan(q)) {
            set_error("pcpx_surface_nets_hint: the hint's grid coordinate is NaN (a zero voxel size)");
            return PCPX_ERR_INVALID;
        }
        const double lim = 1099511627776.0;  // 2^40
        h[a] = static_cast<long long>(std::min(lim, std::max(-lim, std::floor(static_cast<double>(q)))));
        hc[a] = static_cast<u32>(std::min<long long>(std::max<long long>(h[a], 0), sz[a] - 1));
    }
    const SearchOrder& order = search_order(queue_max);
    const u64 table = order.offsets.size() / 3;

    Events ev;
    if (phase_ms && (st = ev.create(6)) != PCPX_OK) return st;
    const auto mark = [&](int q) -> int {
        if (phase_ms) PCPX_HIP(hipEventRecord(ev.e[q], s));
        return PCPX_OK;
    };
    DevBuf vofs(pool), sums(pool), map(pool), active(pool), parent(pool), seed(pool), offs(pool);
    const u64 tiles_c = scan_tiles(ncubes + 1);
    if ((st = vofs.alloc((ncubes + 1) * sizeof(u32))) != PCPX_OK || (st = map.alloc(ncubes * sizeof(u32))) != PCPX_OK ||
        (st = sums.alloc(std::max<u64>(tiles_c, 64) * sizeof(u64))) != PCPX_OK || (st = seed.alloc(2 * sizeof(u64))) != PCPX_OK ||
        (st = offs.alloc(std::max<u64>(table, 1) * 3 * sizeof(int))) != PCPX_OK)
        return st;
    // phase 1: the active cubes -- offsets, then the dense cube -> active rank map and the list
    if ((st = mark(0)) != PCPX_OK) return st;
    u64 nv = 0;
    if ((st = active_offsets(g, ncubes, d_field, iso, s, vofs.as<u32>(), sums.as<u32>(), nullptr, &nv)) != PCPX_OK) return st;
    if ((st = active.alloc(std::max<u64>(nv, 1) * sizeof(u32))) != PCPX_OK || (st = parent.alloc(std::max<u64>(nv, 1) * sizeof(u32))) != PCPX_OK)
        return st;
    k_sn_vertices<<<blocks_for(ncubes), SN_BLOCK, 0, s>>>(g, static_cast<u32>(ncubes), d_field, iso, vofs.as<u32>(), map.as<u32>(),
                                                          active.as<u32>(), nullptr);
    PCPX_HIP(hipGetLastError());
    if ((st = mark(1)) != PCPX_OK) return st;
    // phase 2: the seed
    u64 found[2] = {UINT64_MAX, UINT64_MAX};
    if (nv > 0) {
        PCPX_HIP(hipMemsetAsync(seed.p, 0xFF, 2 * sizeof(u64), s));
        if (table > 0) {
            if ((st = upload_pageable(offs.p, order.offsets.data(), table * 3 * sizeof(int), s)) != PCPX_OK) return st;
            k_hint_seed<<<1, SN_BLOCK, 0, s>>>(g, offs.as<int>(), static_cast<u32>(table), h[0], h[1], h[2], map.as<u32>(),
                                               seed.as<unsigned long long>());
            PCPX_HIP(hipGetLastError());
        }
        if (!order.bounded) {
            k_hint_nearest<<<blocks_for(nv), SN_BLOCK, 0, s>>>(g, static_cast<u32>(nv), active.as<u32>(), hc[0], hc[1], hc[2],
                                                               seed.as<unsigned long long>());
            PCPX_HIP(hipGetLastError());
        }
        PCPX_HIP(hipMemcpyAsync(found, seed.p, sizeof(found), hipMemcpyDeviceToHost, s));
        PCPX_HIP(hipStreamSynchronize(s));
    }
    const u64 seed_cube = found[0] != UINT64_MAX ? found[0] : (found[1] != UINT64_MAX ? (found[1] & 0xFFFFFFFFull) : UINT64_MAX);
    *out_seed = seed_cube;
    if ((st = mark(2)) != PCPX_OK) return st;
    // phase 3: the components, and phase 4: the restriction to the seed's (no seed: the whole grid, vofs as it stands)
    u64 nsel = nv;
    if (seed_cube != UINT64_MAX) {
        const u32 nv32 = static_cast<u32>(nv);
        k_cc_init<<<blocks_for(nv), SN_BLOCK, 0, s>>>(nv32, parent.as<u32>());
        k_cc_hook<<<blocks_for(nv), SN_BLOCK, 0, s>>>(g, nv32, d_field, iso, active.as<u32>(), map.as<u32>(), parent.as<u32>());
        k_cc_flatten<<<blocks_for(nv), SN_BLOCK, 0, s>>>(nv32, parent.as<u32>());
        PCPX_HIP(hipGetLastError());
        if (rounds) *rounds = 1;  // union-find: one hook launch, whatever the component's diameter
        if ((st = mark(3)) != PCPX_OK) return st;
        PCPX_HIP(hipMemsetAsync(vofs.as<u32>() + ncubes, 0, sizeof(u32), s));
        k_cc_restrict<<<blocks_for(ncubes), SN_BLOCK, 0, s>>>(static_cast<u32>(ncubes), map.as<u32>(), parent.as<u32>(),
                                                              static_cast<u32>(seed_cube), vofs.as<u32>());
        PCPX_HIP(hipGetLastError());
        if ((st = exclusive_scan_in_place<u32>(vofs.as<u32>(), ncubes + 1, sums.as<u32>(), s)) != PCPX_OK) return st;
        u32 n32 = 0;
        PCPX_HIP(hipMemcpyAsync(&n32, vofs.as<u32>() + ncubes, sizeof(u32), hipMemcpyDeviceToHost, s));
        PCPX_HIP(hipStreamSynchronize(s));
        nsel = n32;
    } else if ((st = mark(3)) != PCPX_OK) {
        return st;
    }
    *out_nv = nsel;
    // phases 4 (the vertices) and 5 (the triangles): the whole-grid passes over the selected cubes
    st = mesh_selected(g, ncubes, d_field, iso, s, pool, vofs.as<u32>(), map.as<u32>(), nsel, d_out_xyz, vertex_capacity, d_out_tri,
                       triangle_capacity, out_nt, phase_ms ? ev.e[4] : nullptr, phase_ms ? ev.e[5] : nullptr);
    if (phase_ms && (st == PCPX_OK || st == PCPX_ERR_CAPACITY))
        for (int q = 0; q < 5; ++q) PCPX_HIP(hipEventElapsedTime(&phase_ms[q], ev.e[q], ev.e[q + 1]));
    return st;
}

int surface_nets_search_order(u64 queue_max, int* out, u64 capacity, u64* out_count, int* out_bounded)
{
    const SearchOrder& order = search_order(queue_max);
    *out_count = order.offsets.size() / 3;
    *out_bounded = order.bounded ? 1 : 0;
    if (*out_count == 0) return PCPX_OK;
    if (!out || capacity < *out_count) {
        set_error("pcpx_surface_nets_search_order: the table has %llu entries", static_cast<unsigned long long>(*out_count));
        return PCPX_ERR_CAPACITY;
    }
    std::copy(order.offsets.begin(), order.offsets.end(), out);
    return PCPX_OK;
}

}  // namespace

int tangent_plane_sdf_device(Index& ix, const float* d_centroids, const float* d_normals, const pcpx_grid3d& grid, float eps, float* d_field)
{
    GridDev g{};
    u64 ncubes = 0;
    int st = grid_to_dev(grid, g, ncubes);
    if (st != PCPX_OK) return st;
    // (a grid with no cube along some axis still has corners: the field is defined there too)
    g.x = grid.x, g.y = grid.y, g.z = grid.z, g.dx = grid.dx, g.dy = grid.dy, g.dz = grid.dz;
    g.sx = static_cast<u32>(grid.sx), g.sy = static_cast<u32>(grid.sy), g.sz = static_cast<u32>(grid.sz);
    const Bricks b{static_cast<u32>((grid.sx + 1 + 3) / 4), static_cast<u32>((grid.sy + 1 + 3) / 4), static_cast<u32>((grid.sz + 1 + 3) / 4)};
    const u64 nq = static_cast<u64>(b.bx) * b.by * b.bz * 64;
    if (nq >= 0xFFFFFFFEull) {
        set_error("pcpx_tangent_plane_sdf_dev: %llu corner queries (4x4x4 bricks) do not fit 32-bit rows", static_cast<unsigned long long>(nq));
        return PCPX_ERR_UNSUPPORTED;
    }
    if (ix.n == 0) {
        set_error("pcpx_tangent_plane_sdf_dev: the index holds no points");
        return PCPX_ERR_INVALID;
    }
    hipStream_t s = ix.stream;
    DevBuf q(ix.pool), nn(ix.pool), cnt(ix.pool);
    if ((st = q.alloc(nq * 3 * sizeof(float))) != PCPX_OK || (st = nn.alloc(nq * sizeof(u32))) != PCPX_OK ||
        (st = cnt.alloc(nq * sizeof(u32))) != PCPX_OK)
        return st;
    k_sdf_queries<<<blocks_for(nq), SN_BLOCK, 0, s>>>(g, b, nq, q.as<float>());
    PCPX_HIP(hipGetLastError());
    QueryView qv;
    if ((st = prepare_queries(ix, q.as<float>(), nq, qv)) != PCPX_OK) return st;
    KnnOutputs o;
    o.idx = nn.as<u32>();
    o.cnt = cnt.as<u32>();
    if ((st = launch_knn(ix, qv, false, 0, (nq + GROUP - 1) / GROUP, 1, eps, o)) != PCPX_OK) return st;
    k_sdf_eval<<<blocks_for(nq), SN_BLOCK, 0, s>>>(g, b, nq, nn.as<u32>(), cnt.as<u32>(), d_centroids, d_normals, d_field);
    PCPX_HIP(hipGetLastError());
    PCPX_HIP(hipStreamSynchronize(s));  // (the query buffers go back to the pool)
    return PCPX_OK;
}

}  // namespace pcpx

using namespace pcpx;

extern "C" {

// ---- surface reconstruction (pcpx_isosurface.hip) -------------------------------------------------------------------------

int pcpx_regular_grid_containing(const float min3[3], const float max3[3], const uint64_t dims[3], pcpx_grid3d* out)
{
    if (!min3 || !max3 || !dims || !out) return PCPX_ERR_INVALID;
    pcpx_grid3d g{};
    g.x = min3[0], g.y = min3[1], g.z = min3[2];
    g.sx = dims[0], g.sy = dims[1], g.sz = dims[2];
    g.dx = (max3[0] - min3[0]) / static_cast<float>(g.sx);
    g.dy = (max3[1] - min3[1]) / static_cast<float>(g.sy);
    g.dz = (max3[2] - min3[2]) / static_cast<float>(g.sz);
    g.x -= g.dx;
    g.y -= g.dx;  // (sic: regular_grid3d.hpp:84-86 moves every axis back by dx)
    g.z -= g.dx;
    g.sx += 2, g.sy += 2, g.sz += 2;
    *out = g;
    return PCPX_OK;
}

int pcpx_surface_nets_timed_dev(const float* d_field, const pcpx_grid3d* grid, float isovalue, int device, void* stream, float* d_out_xyz,
                                uint64_t vertex_capacity, uint32_t* d_out_tri, uint64_t triangle_capacity, uint64_t* out_nvertices,
                                uint64_t* out_ntriangles, float out_pass_ms[3])
{
    if (!grid || !out_nvertices || !out_ntriangles) return PCPX_ERR_INVALID;
    *out_nvertices = *out_ntriangles = 0;
    return on_shared(device, "pcpx_surface_nets_dev", [&](DeviceShared& sh) -> int {
        SurfaceNetsTimes t;
        const int r = surface_nets_device(d_field, *grid, isovalue, static_cast<hipStream_t>(stream), sh.pool, d_out_xyz, vertex_capacity,
                                          d_out_tri, triangle_capacity, out_nvertices, out_ntriangles, out_pass_ms ? &t : nullptr);
        if (out_pass_ms) out_pass_ms[0] = t.flags_ms, out_pass_ms[1] = t.vertices_ms, out_pass_ms[2] = t.triangles_ms;
        return r;
    });
}

int pcpx_surface_nets_dev(const float* d_field, const pcpx_grid3d* grid, float isovalue, int device, void* stream, float* d_out_xyz,
                          uint64_t vertex_capacity, uint32_t* d_out_tri, uint64_t triangle_capacity, uint64_t* out_nvertices,
                          uint64_t* out_ntriangles)
{
    return pcpx_surface_nets_timed_dev(d_field, grid, isovalue, device, stream, d_out_xyz, vertex_capacity, d_out_tri, triangle_capacity,
                                       out_nvertices, out_ntriangles, nullptr);
}

int pcpx_surface_nets(const float* field, const pcpx_grid3d* grid, float isovalue, int device, float* out_xyz, uint64_t vertex_capacity,
                      uint32_t* out_tri, uint64_t triangle_capacity, uint64_t* out_nvertices, uint64_t* out_ntriangles)
{
    if (!grid || !out_nvertices || !out_ntriangles) return PCPX_ERR_INVALID;
    *out_nvertices = *out_ntriangles = 0;
    if (grid->sx == 0 || grid->sy == 0 || grid->sz == 0) return PCPX_OK;
    if (!field) return PCPX_ERR_INVALID;
    const int valid = check_surface_grid(*grid);  // (before the field is read)
    if (valid != PCPX_OK) return valid;
    return on_shared(device, "pcpx_surface_nets", [&](DeviceShared& sh) -> int {
        PooledStream ps;
        PCPX_HIP(pooled_stream_get(&ps.s));
        const hipStream_t s = ps.s;
        const u64 corners = (grid->sx + 1) * (grid->sy + 1) * (grid->sz + 1);
        DevBuf df(sh.pool), dv(sh.pool), dt(sh.pool);
        int r;
        if ((r = df.alloc(corners * sizeof(float))) != PCPX_OK) return r;
        const u64 vcap = out_xyz ? vertex_capacity : 0, tcap = out_tri ? triangle_capacity : 0;
        if ((vcap > 0 && (r = dv.alloc(vcap * 3 * sizeof(float))) != PCPX_OK) || (tcap > 0 && (r = dt.alloc(tcap * 3 * sizeof(u32))) != PCPX_OK))
            return r;
        if ((r = upload_pageable(df.p, field, corners * sizeof(float), s)) != PCPX_OK) return r;
        r = surface_nets_device(df.as<float>(), *grid, isovalue, s, sh.pool, dv.as<float>(), vcap, dt.as<u32>(), tcap, out_nvertices,
                                out_ntriangles);
        if (r != PCPX_OK) return r;
        if (*out_nvertices) PCPX_HIP(hipMemcpyAsync(out_xyz, dv.p, *out_nvertices * 3 * sizeof(float), hipMemcpyDeviceToHost, s));
        if (*out_ntriangles) PCPX_HIP(hipMemcpyAsync(out_tri, dt.p, *out_ntriangles * 3 * sizeof(u32), hipMemcpyDeviceToHost, s));
        PCPX_HIP(hipStreamSynchronize(s));
        return PCPX_OK;
    });
}

int pcpx_surface_nets_hint_timed_dev(const float* d_field, const pcpx_grid3d* grid, float isovalue, const float hint[3], uint64_t queue_max,
                                     int device, void* stream, float* d_out_xyz, uint64_t vertex_capacity, uint32_t* d_out_tri,
                                     uint64_t triangle_capacity, uint64_t* out_nvertices, uint64_t* out_ntriangles, uint64_t* opt_out_seed_cube,
                                     float out_phase_ms[5], uint32_t* opt_out_rounds)
{
    if (opt_out_seed_cube) *opt_out_seed_cube = UINT64_MAX;
    if (!grid || !hint || !out_nvertices || !out_ntriangles) return PCPX_ERR_INVALID;
    *out_nvertices = *out_ntriangles = 0;
    return on_shared(device, "pcpx_surface_nets_hint_dev", [&](DeviceShared& sh) -> int {
        u64 seed = UINT64_MAX;
        const int r = surface_nets_hint_device(d_field, *grid, isovalue, hint, queue_max, static_cast<hipStream_t>(stream), sh.pool, d_out_xyz,
                                               vertex_capacity, d_out_tri, triangle_capacity, out_nvertices, out_ntriangles, &seed, out_phase_ms,
                                               opt_out_rounds);
        if (opt_out_seed_cube) *opt_out_seed_cube = seed;
        return r;
    });
}

int pcpx_surface_nets_hint_dev(const float* d_field, const pcpx_grid3d* grid, float isovalue, const float hint[3], uint64_t queue_max, int device,
                               void* stream, float* d_out_xyz, uint64_t vertex_capacity, uint32_t* d_out_tri, uint64_t triangle_capacity,
                               uint64_t* out_nvertices, uint64_t* out_ntriangles, uint64_t* opt_out_seed_cube)
{
    return pcpx_surface_nets_hint_timed_dev(d_field, grid, isovalue, hint, queue_max, device, stream, d_out_xyz, vertex_capacity, d_out_tri,
                                            triangle_capacity, out_nvertices, out_ntriangles, opt_out_seed_cube, nullptr, nullptr);
}

int pcpx_surface_nets_hint(const float* field, const pcpx_grid3d* grid, float isovalue, const float hint[3], uint64_t queue_max, int device,
                           float* out_xyz, uint64_t vertex_capacity, uint32_t* out_tri, uint64_t triangle_capacity, uint64_t* out_nvertices,
                           uint64_t* out_ntriangles, uint64_t* opt_out_seed_cube)
{
    if (opt_out_seed_cube) *opt_out_seed_cube = UINT64_MAX;
    if (!grid || !hint || !out_nvertices || !out_ntriangles) return PCPX_ERR_INVALID;
    *out_nvertices = *out_ntriangles = 0;
    if (!std::isfinite(hint[0]) || !std::isfinite(hint[1]) || !std::isfinite(hint[2])) return PCPX_ERR_INVALID;
    if (grid->sx == 0 || grid->sy == 0 || grid->sz == 0) return PCPX_OK;
    if (!field) return PCPX_ERR_INVALID;
    const int valid = check_surface_grid(*grid);  // (before the field is read)
    if (valid != PCPX_OK) return valid;
    return on_shared(device, "pcpx_surface_nets_hint", [&](DeviceShared& sh) -> int {
        PooledStream ps;
        PCPX_HIP(pooled_stream_get(&ps.s));
        const hipStream_t s = ps.s;
        const u64 corners = (grid->sx + 1) * (grid->sy + 1) * (grid->sz + 1);
        DevBuf df(sh.pool), dv(sh.pool), dt(sh.pool);
        int r;
        if ((r = df.alloc(corners * sizeof(float))) != PCPX_OK) return r;
        const u64 vcap = out_xyz ? vertex_capacity : 0, tcap = out_tri ? triangle_capacity : 0;
        if ((vcap > 0 && (r = dv.alloc(vcap * 3 * sizeof(float))) != PCPX_OK) || (tcap > 0 && (r = dt.alloc(tcap * 3 * sizeof(u32))) != PCPX_OK))
            return r;
        if ((r = upload_pageable(df.p, field, corners * sizeof(float), s)) != PCPX_OK) return r;
        u64 seed = UINT64_MAX;
        r = surface_nets_hint_device(df.as<float>(), *grid, isovalue, hint, queue_max, s, sh.pool, dv.as<float>(), vcap, dt.as<u32>(), tcap,
                                     out_nvertices, out_ntriangles, &seed, nullptr, nullptr);
        if (opt_out_seed_cube) *opt_out_seed_cube = seed;
        if (r != PCPX_OK) return r;
        if (*out_nvertices) PCPX_HIP(hipMemcpyAsync(out_xyz, dv.p, *out_nvertices * 3 * sizeof(float), hipMemcpyDeviceToHost, s));
        if (*out_ntriangles) PCPX_HIP(hipMemcpyAsync(out_tri, dt.p, *out_ntriangles * 3 * sizeof(u32), hipMemcpyDeviceToHost, s));
        PCPX_HIP(hipStreamSynchronize(s));
        return PCPX_OK;
    });
}

int pcpx_surface_nets_search_order(uint64_t queue_max, int32_t* out_offsets, uint64_t capacity, uint64_t* out_count, int* out_bounded)
{
    if (!out_count || !out_bounded) return PCPX_ERR_INVALID;
    *out_count = 0;
    *out_bounded = 0;
    return on_host("pcpx_surface_nets_search_order",
                   [&]() -> int { return surface_nets_search_order(queue_max, out_offsets, capacity, out_count, out_bounded); });
}

int pcpx_tangent_plane_sdf_dev(pcpx_index* h, const float* d_centroids, const float* d_normals, const pcpx_grid3d* grid, float eps,
                               float* d_out_field)
{
    return on_index(h, "pcpx_tangent_plane_sdf_dev", WHOLE_CLOUD, [&](Index* ix) -> int {
    if (!grid || !d_centroids || !d_normals || !d_out_field) return PCPX_ERR_INVALID;
    return tangent_plane_sdf_device(*ix, d_centroids, d_normals, *grid, eps, d_out_field);
    });
}

// the pipeline of examples/tangent_plane_surface_reconstruction.cpp:233-455 after the tree, device resident
static int reconstruct_device(Index* ix, u32 k, float eps, const uint64_t dims[3], float iso, float* d_xyz, u64 vcap, u32* d_tri, u64 tcap,
                              u64* out_nv, u64* out_nt, float* d_opt_centroids, float* d_opt_normals, pcpx_grid3d* opt_grid)
{
    pcpx_index* h = reinterpret_cast<pcpx_index*>(ix);
    if (k == 0 || !dims || !out_nv || !out_nt) return PCPX_ERR_INVALID;
    *out_nv = *out_nt = 0;
    int st = check_all_inserted(*ix, "pcpx_reconstruct_surface");
    if (st != PCPX_OK) return st;
    const u64 rows = ix->n_in;
    if (rows == 0) return PCPX_OK;
    DevBuf dc(ix->pool), dn(ix->pool), di(ix->pool), dk(ix->pool), df(ix->pool);
    float* d_c = d_opt_centroids;
    float* d_n = d_opt_normals;
    if ((!d_c && (st = dc.alloc(rows * 3 * sizeof(float))) != PCPX_OK) || (!d_n && (st = dn.alloc(rows * 3 * sizeof(float))) != PCPX_OK) ||
        (st = di.alloc(rows * k * sizeof(u32))) != PCPX_OK || (st = dk.alloc(rows * sizeof(u32))) != PCPX_OK)
        return st;
    if (!d_c) d_c = dc.as<float>();
    if (!d_n) d_n = dn.as<float>();
    // 1-2: tangent planes (estimate_tangent_planes), then propagate_normal_orientations over the kNN rows
    if ((st = pcpx_neighbourhoods_self_dev(h, k, eps, 0, UINT64_MAX, d_n, d_c, nullptr)) != PCPX_OK) return st;
    if ((st = pcpx_knn_self_dev(h, k, eps, 0, UINT64_MAX, di.as<u32>(), dk.as<u32>(), nullptr)) != PCPX_OK) return st;
    if ((st = orient_normals_device(ix->d_xyz, rows, di.as<u32>(), dk.as<u32>(), k, d_n, ix->stream, nullptr, nullptr)) != PCPX_OK) return st;
    // 3: the grid around the index's box
    pcpx_grid3d g{};
    if ((st = pcpx_regular_grid_containing(ix->bbox, ix->bbox + 3, dims, &g)) != PCPX_OK) return st;
    if (opt_grid) *opt_grid = g;
    // 4-5: the field, surface nets
    const u64 corners = (g.sx + 1) * (g.sy + 1) * (g.sz + 1);
    if ((st = df.alloc(corners * sizeof(float))) != PCPX_OK) return st;
    if ((st = tangent_plane_sdf_device(*ix, d_c, d_n, g, eps, df.as<float>())) != PCPX_OK) return st;
    return surface_nets_device(df.as<float>(), g, iso, ix->stream, ix->pool, d_xyz, vcap, d_tri, tcap, out_nv, out_nt);
}

int pcpx_reconstruct_surface_dev(pcpx_index* h, uint32_t k, float eps, const uint64_t dims[3], float isovalue, float* d_out_xyz,
                                 uint64_t vertex_capacity, uint32_t* d_out_tri, uint64_t triangle_capacity, uint64_t* out_nvertices,
                                 uint64_t* out_ntriangles, float* d_opt_out_centroids, float* d_opt_out_normals, pcpx_grid3d* opt_out_grid)
{
    return on_index(h, "pcpx_reconstruct_surface_dev", WHOLE_CLOUD, [&](Index* ix) {
        return reconstruct_device(ix, k, eps, dims, isovalue, d_out_xyz, vertex_capacity, d_out_tri, triangle_capacity, out_nvertices,
                                  out_ntriangles, d_opt_out_centroids, d_opt_out_normals, opt_out_grid);
    });
}

int pcpx_reconstruct_surface(pcpx_index* h, uint32_t k, float eps, const uint64_t dims[3], float isovalue, float* out_xyz,
                             uint64_t vertex_capacity, uint32_t* out_tri, uint64_t triangle_capacity, uint64_t* out_nvertices,
                             uint64_t* out_ntriangles, float* opt_out_centroids, float* opt_out_normals, pcpx_grid3d* opt_out_grid)
{
    return on_index(h, "pcpx_reconstruct_surface", WHOLE_CLOUD, [&](Index* ix) -> int {
        const u64 rows = ix->n_in;
        const u64 vcap = out_xyz ? vertex_capacity : 0, tcap = out_tri ? triangle_capacity : 0;
        DevBuf dv(ix->pool), dt(ix->pool), dc(ix->pool), dn(ix->pool);
        int r;
        if ((vcap > 0 && (r = dv.alloc(vcap * 3 * sizeof(float))) != PCPX_OK) || (tcap > 0 && (r = dt.alloc(tcap * 3 * sizeof(u32))) != PCPX_OK) ||
            (opt_out_centroids && rows > 0 && (r = dc.alloc(rows * 3 * sizeof(float))) != PCPX_OK) ||
            (opt_out_normals && rows > 0 && (r = dn.alloc(rows * 3 * sizeof(float))) != PCPX_OK))
            return r;
        r = reconstruct_device(ix, k, eps, dims, isovalue, dv.as<float>(), vcap, dt.as<u32>(), tcap, out_nvertices, out_ntriangles,
                               dc.as<float>(), dn.as<float>(), opt_out_grid);
        if (r != PCPX_OK && r != PCPX_ERR_CAPACITY) return r;
        if (r == PCPX_OK) {
            if (*out_nvertices) PCPX_HIP(hipMemcpyAsync(out_xyz, dv.p, *out_nvertices * 3 * sizeof(float), hipMemcpyDeviceToHost, ix->stream));
            if (*out_ntriangles) PCPX_HIP(hipMemcpyAsync(out_tri, dt.p, *out_ntriangles * 3 * sizeof(u32), hipMemcpyDeviceToHost, ix->stream));
        }
        if (dc.p) PCPX_HIP(hipMemcpyAsync(opt_out_centroids, dc.p, rows * 3 * sizeof(float), hipMemcpyDeviceToHost, ix->stream));
        if (dn.p) PCPX_HIP(hipMemcpyAsync(opt_out_normals, dn.p, rows * 3 * sizeof(float), hipMemcpyDeviceToHost, ix->stream));
        PCPX_HIP(hipStreamSynchronize(ix->stream));
        return r;
    });
}

}  // extern "C"
