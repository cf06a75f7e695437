// Driver over a real build of the reference's headers -- TEST INFRASTRUCTURE ONLY.
//
// Compiled (oracle/Makefile, target _ref/libpcp_ref.so) against the reference's include/ and the range-v3 stand-ins in
// oracle/ref_shim/, with the flags of libpcp_oracle.so.  Every query below is the reference's own template, instantiated
// here; nothing is restated except the WLOP iteration around the header's own pieces (ref_wlop_from_sample, with line
// citations), which has to take its initial sample from the caller because wlop() draws it from std::random_device.
//
// Element types: point indices (std::uint32_t for the octree, std::size_t for the kd-trees, as WLOP uses them).
#include <cassert>  // wlop.hpp uses assert without including it

#include <pcp/algorithm/average_distance_to_neighbors.hpp>
#include <pcp/algorithm/surface_nets.hpp>
#include <pcp/algorithm/wlop.hpp>
#include <pcp/common/axis_aligned_bounding_box.hpp>
#include <pcp/common/points/point.hpp>
#include <pcp/common/sphere.hpp>
#include <pcp/kdtree/linked_kdtree.hpp>
#include <pcp/octree/linked_octree.hpp>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <execution>
#include <iterator>
#include <memory>
#include <numeric>
#include <thread>
#include <vector>

namespace {

using u32 = std::uint32_t;
using u64 = std::uint64_t;
using point_type = pcp::point_t;
constexpr u32 kNone = 0xFFFFFFFFu;

template <class F>
void parallel_for(u64 n, int nthreads, F const& f)
{
    int const t = std::max(1, std::min<int>(nthreads, static_cast<int>(std::max<u64>(1, n / 64))));
    if (t == 1) {
        for (u64 i = 0; i < n; ++i) f(i);
        return;
    }
    std::vector<std::thread> pool;
    for (int w = 0; w < t; ++w)
        pool.emplace_back([&, w] {
            for (u64 i = static_cast<u64>(w); i < n; i += static_cast<u64>(t)) f(i);
        });
    for (auto& th : pool) th.join();
}

std::vector<point_type> to_points(float const* xyz, u64 n)
{
    std::vector<point_type> p(n);
    for (u64 i = 0; i < n; ++i) p[i] = point_type{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    return p;
}

// ---- linked_octree_t over point indices ----
struct PointView
{
    std::vector<point_type> const* pts;
    point_type operator()(u32 i) const { return (*pts)[i]; }
};

using octree_type = pcp::basic_linked_octree_t<u32>;

struct Octree
{
    std::vector<point_type> pts;
    std::vector<u32> ids;
    std::unique_ptr<octree_type> tree;
};

template <class Vec>
u64 copy_capped(Vec const& v, u32* out, u64 cap)
{
    for (u64 i = 0; i < v.size() && i < cap; ++i) out[i] = static_cast<u32>(v[i]);
    return v.size();
}

// ---- basic_linked_kdtree_t<std::size_t, K, map> for K = 1 ... 16 ----
struct KdBase
{
    virtual ~KdBase() = default;
    virtual void knn(float const* q, u32 k, float eps, u32* idx, u32* cnt) const = 0;
    virtual u64 range_aabb(float const* box, u32* out, u64 cap) const = 0;
};

template <std::size_t K>
struct Kd final : KdBase
{
    using coords = std::array<float, K>;
    struct Map
    {
        std::vector<coords> const* c;
        coords operator()(std::size_t i) const { return (*c)[i]; }
    };
    std::vector<coords> c;
    std::vector<std::size_t> ids;
    std::unique_ptr<pcp::basic_linked_kdtree_t<std::size_t, K, Map>> tree;

    Kd(float const* pts, u64 n, pcp::kdtree::construction_params_t const* params) : c(n), ids(n)
    {
        for (u64 i = 0; i < n; ++i)
            for (std::size_t a = 0; a < K; ++a) c[i][a] = pts[i * K + a];
        std::iota(ids.begin(), ids.end(), std::size_t{0});
        Map const m{&c};
        if (params)
            tree = std::make_unique<pcp::basic_linked_kdtree_t<std::size_t, K, Map>>(ids.begin(), ids.end(), m, *params);
        else
            tree = std::make_unique<pcp::basic_linked_kdtree_t<std::size_t, K, Map>>(ids.begin(), ids.end(), m);
    }
    void knn(float const* q, u32 k, float eps, u32* idx, u32* cnt) const override
    {
        coords t;
        for (std::size_t a = 0; a < K; ++a) t[a] = q[a];
        auto const r = tree->nearest_neighbours(t, k, eps);
        for (u32 i = 0; i < k; ++i) idx[i] = i < r.size() ? static_cast<u32>(r[i]) : kNone;
        *cnt = static_cast<u32>(r.size());
    }
    u64 range_aabb(float const* box, u32* out, u64 cap) const override
    {
        pcp::kd_axis_aligned_bounding_box_t<float, K> b;
        for (std::size_t a = 0; a < K; ++a) {
            b.min[a] = box[a];
            b.max[a] = box[K + a];
        }
        auto r = tree->range_search(b);
        std::sort(r.begin(), r.end());
        return copy_capped(r, out, cap);
    }
};

template <std::size_t K>
KdBase* make_kd(u64 dims, float const* pts, u64 n, pcp::kdtree::construction_params_t const* p)
{
    if constexpr (K > 16) {
        return nullptr;
    } else {
        if (dims == K) return new Kd<K>(pts, n, p);
        return make_kd<K + 1>(dims, pts, n, p);
    }
}

// ---- surface nets ----
struct Mesh
{
    std::vector<point_type> v;
    std::vector<pcp::common::shared_vertex_mesh_triangle<std::uint32_t>> t;
};

// The field the reference evaluates: the corner array the GPU takes.  Each position the reference asks for must be one
// of the grid's corners exactly as get_world_point_of computes it; the corner is recovered from the coordinates and the
// position compared bit for bit.  A position outside the grid's box (the hint overload walks cubes past the faces)
// yields `outside` when the caller allows it.  Anything else is a misreading of the reference's evaluation: abort.
struct CornerField
{
    float const* field;
    pcp::common::regular_grid3d_t<float> grid;
    float outside;
    bool allow_outside;

    static bool recover(float p, float o, float d, std::size_t s, std::size_t& i)
    {
        double const r = std::nearbyint((static_cast<double>(p) - static_cast<double>(o)) / static_cast<double>(d));
        if (!(r >= 0.0 && r <= static_cast<double>(s))) return false;
        i = static_cast<std::size_t>(r);
        return true;
    }
    bool outside_box(float x, float y, float z) const
    {
        float const hx = grid.x + static_cast<float>(grid.sx) * grid.dx, hy = grid.y + static_cast<float>(grid.sy) * grid.dy,
                    hz = grid.z + static_cast<float>(grid.sz) * grid.dz;
        return x < grid.x || x > hx || y < grid.y || y > hy || z < grid.z || z > hz;
    }
    float operator()(float x, float y, float z) const
    {
        std::size_t i = 0, j = 0, k = 0;
        if (recover(x, grid.x, grid.dx, grid.sx, i) && recover(y, grid.y, grid.dy, grid.sy, j) &&
            recover(z, grid.z, grid.dz, grid.sz, k)) {
            point_type const w = pcp::algorithm::isosurface::get_world_point_of<point_type, float>(i, j, k, grid);
            if (w.x() == x && w.y() == y && w.z() == z)
                return field[i + (grid.sx + 1) * (j + (grid.sy + 1) * k)];
        }
        if (allow_outside && outside_box(x, y, z)) return outside;
        std::fprintf(stderr, "pcp_ref: surface_nets evaluated f(%.9g, %.9g, %.9g), which is no corner of the grid\n",
                     static_cast<double>(x), static_cast<double>(y), static_cast<double>(z));
        std::abort();
    }
};

pcp::common::regular_grid3d_t<float> make_grid(float const* o_d, u64 const* s)
{
    pcp::common::regular_grid3d_t<float> g;
    g.x = o_d[0];
    g.y = o_d[1];
    g.z = o_d[2];
    g.dx = o_d[3];
    g.dy = o_d[4];
    g.dz = o_d[5];
    g.sx = s[0];
    g.sy = s[1];
    g.sz = s[2];
    return g;
}

} // namespace

extern "C" {

// grid6 (NULL: the constructor that computes the bounding box, linked_octree.hpp:103-121, when capacity and depth are
// the defaults; else that box with the given parameters through the explicit constructor, :83-91)
void* ref_octree_create(float const* xyz, u64 n, u32 capacity, u32 max_depth, float const* grid6)
{
    auto* t = new Octree();
    t->pts = to_points(xyz, n);
    t->ids.resize(n);
    std::iota(t->ids.begin(), t->ids.end(), 0u);
    PointView const pv{&t->pts};
    octree_type::params_type params;
    if (!grid6 && capacity == params.node_capacity && max_depth == params.max_depth) {
        t->tree = std::make_unique<octree_type>(t->ids.begin(), t->ids.end(), pv);
        return t;
    }
    params.node_capacity = capacity;
    params.max_depth = static_cast<std::uint8_t>(max_depth);
    if (grid6) {
        params.voxel_grid.min = point_type{grid6[0], grid6[1], grid6[2]};
        params.voxel_grid.max = point_type{grid6[3], grid6[4], grid6[5]};
    } else {
        params.voxel_grid = pcp::bounding_box<std::vector<point_type>::const_iterator, point_type>(t->pts.cbegin(), t->pts.cend());
    }
    t->tree = std::make_unique<octree_type>(t->ids.begin(), t->ids.end(), pv, params);
    return t;
}
void ref_octree_destroy(void* h) { delete static_cast<Octree*>(h); }
u64 ref_octree_size(void* h) { return static_cast<Octree*>(h)->tree->size(); }
void ref_octree_grid(void* h, float* out6)
{
    auto const& g = static_cast<Octree*>(h)->tree->voxel_grid();
    float const v[6] = {g.min.x(), g.min.y(), g.min.z(), g.max.x(), g.max.y(), g.max.z()};
    std::copy(v, v + 6, out6);
}
// nearest_neighbours(target, k, point_view, eps) per query; rows padded with 0xFFFFFFFF
void ref_octree_knn(void* h, float const* q, u64 nq, u32 k, double eps, u32* idx, u32* cnt, int nthreads)
{
    auto const* t = static_cast<Octree*>(h);
    PointView const pv{&t->pts};
    parallel_for(nq, nthreads, [&](u64 i) {
        point_type const target{q[3 * i], q[3 * i + 1], q[3 * i + 2]};
        auto const r = t->tree->nearest_neighbours(target, k, pv, eps);
        for (u32 c = 0; c < k; ++c) idx[i * k + c] = c < r.size() ? r[c] : kNone;
        cnt[i] = static_cast<u32>(r.size());
    });
}
// range_search with a sphere_t; returns the number found, writes at most cap indices (ascending)
u64 ref_octree_range_sphere(void* h, float const* c, float r, u32* out, u64 cap)
{
    auto const* t = static_cast<Octree*>(h);
    pcp::sphere_t<point_type> s;
    s.position = point_type{c[0], c[1], c[2]};
    s.radius = r;
    auto v = t->tree->range_search(s, PointView{&t->pts});
    std::sort(v.begin(), v.end());
    return copy_capped(v, out, cap);
}
// one radius per sphere: counts of every sphere (the lists through ref_octree_range_sphere)
void ref_octree_range_count_spheres(void* h, float const* c, float const* r, u64 nq, u32* cnt, int nthreads)
{
    auto const* t = static_cast<Octree*>(h);
    PointView const pv{&t->pts};
    parallel_for(nq, nthreads, [&](u64 i) {
        pcp::sphere_t<point_type> s;
        s.position = point_type{c[3 * i], c[3 * i + 1], c[3 * i + 2]};
        s.radius = r[i];
        cnt[i] = static_cast<u32>(t->tree->range_search(s, pv).size());
    });
}
u64 ref_octree_range_aabb(void* h, float const* b6, u32* out, u64 cap)
{
    auto const* t = static_cast<Octree*>(h);
    pcp::axis_aligned_bounding_box_t<point_type> b;
    b.min = point_type{b6[0], b6[1], b6[2]};
    b.max = point_type{b6[3], b6[4], b6[5]};
    auto v = t->tree->range_search(b, PointView{&t->pts});
    std::sort(v.begin(), v.end());
    return copy_capped(v, out, cap);
}

// basic_linked_kdtree_t<std::size_t, dims, map>; use_params = 0: the reference's default construction_params_t
void* ref_kd_create(u64 dims, float const* pts, u64 n, int use_params, u64 max_depth, int compute_max_depth,
                    u64 max_elements_per_leaf)
{
    pcp::kdtree::construction_params_t p;
    p.max_depth = max_depth;
    p.compute_max_depth = compute_max_depth != 0;
    p.max_elements_per_leaf = max_elements_per_leaf;
    return make_kd<1>(dims, pts, n, use_params ? &p : nullptr);
}
void ref_kd_destroy(void* h) { delete static_cast<KdBase*>(h); }
void ref_kd_knn(void* h, u64 dims, float const* q, u64 nq, u32 k, float eps, u32* idx, u32* cnt, int nthreads)
{
    auto const* t = static_cast<KdBase*>(h);
    parallel_for(nq, nthreads, [&](u64 i) { t->knn(q + i * dims, k, eps, idx + i * k, cnt + i); });
}
u64 ref_kd_range_aabb(void* h, float const* box, u32* out, u64 cap)
{
    return static_cast<KdBase*>(h)->range_aabb(box, out, cap);
}

// average_distances_to_neighbors over self-query rows: knn_map(e) = row e (its first cnt[e] entries)
void ref_average_distances(float const* xyz, u64 n, u32 const* nbr, u32 const* cnt, u32 k, float* out)
{
    std::vector<point_type> const pts = to_points(xyz, n);
    std::vector<u32> ids(n);
    std::iota(ids.begin(), ids.end(), 0u);
    auto const point_map = [&](u32 i) { return pts[i]; };
    auto const knn_map = [&](u32 i) { return std::vector<u32>(nbr + u64(i) * k, nbr + u64(i) * k + cnt[i]); };
    std::vector<float> const m = pcp::algorithm::average_distances_to_neighbors(ids.begin(), ids.end(), point_map, knn_map);
    std::copy(m.begin(), m.end(), out);
}

// surface_nets(std::execution::seq, f, grid, isovalue), or with hint != NULL the hint overload with
// breadth_first_search_queue_max_size = queue_max.  grid6 = (x, y, z, dx, dy, dz), s3 = (sx, sy, sz), field: the
// (sx+1)(sy+1)(sz+1) corner values, x fastest.  Returns a mesh handle (ref_mesh_*).
void* ref_surface_nets(float const* field, float const* grid6, u64 const* s3, float isovalue, float const* hint,
                       u64 queue_max, int allow_outside, float outside)
{
    auto const grid = make_grid(grid6, s3);
    CornerField f{field, grid, outside, allow_outside != 0};
    auto* m = new Mesh();
    if (hint) {
        point_type const p{hint[0], hint[1], hint[2]};
        std::tie(m->v, m->t) = pcp::algorithm::isosurface::surface_nets(std::execution::seq, f, grid, p, isovalue, queue_max);
    } else {
        std::tie(m->v, m->t) = pcp::algorithm::isosurface::surface_nets(std::execution::seq, f, grid, isovalue);
    }
    return m;
}
void ref_mesh_sizes(void* h, u64* nv, u64* nt)
{
    *nv = static_cast<Mesh*>(h)->v.size();
    *nt = static_cast<Mesh*>(h)->t.size();
}
void ref_mesh_copy(void* h, float* v, u32* t)
{
    auto const* m = static_cast<Mesh*>(h);
    for (std::size_t i = 0; i < m->v.size(); ++i) {
        v[3 * i] = m->v[i].x();
        v[3 * i + 1] = m->v[i].y();
        v[3 * i + 2] = m->v[i].z();
    }
    for (std::size_t i = 0; i < m->t.size(); ++i)
        for (int c = 0; c < 3; ++c) t[3 * i + c] = m->t[i].indices()[c];
}
void ref_mesh_destroy(void* h) { delete static_cast<Mesh*>(h); }

// WLOP from a given initial sample: the iteration of pcp::algorithm::wlop::wlop (include/pcp/algorithm/wlop.hpp:287-428)
// around the header's own pieces -- detail::compute_vj, compute_wi, solve_first_energy_median and
// solve_second_energy_repulsion_force -- and its kd-tree parameters.  The header shuffles the source indices and takes the
// last I of them as the sample (:345-356); here the source order is the indices outside the sample, ascending, then the
// sample, so that the sample is the caller's.
struct WlopCoords  // a kd-tree coordinate map over points held elsewhere (the source cloud, or the moving sample)
{
    std::vector<point_type> const* pts;
    std::array<float, 3> operator()(std::size_t i) const { return {(*pts)[i].x(), (*pts)[i].y(), (*pts)[i].z()}; }
};
struct WlopWeights
{
    std::vector<float> const* w;
    float operator()(std::size_t i) const { return (*w)[i]; }
};

void ref_wlop_from_sample(float const* xyz, u64 J, u64 const* sample, u64 I, double mu_, double h_, u64 K, int uniform,
                          float* out)
{
    namespace wd = pcp::algorithm::wlop::detail;
    using kdtree = pcp::basic_linked_kdtree_t<std::size_t, 3u, WlopCoords>;
    std::vector<point_type> const source = to_points(xyz, J);
    float const mu = static_cast<float>(mu_), h = static_cast<float>(h_);  // the header's scalars are the points' (:298-299)
    float const support2 = h * h / 16.f;                                  // theta(r^2) = exp(-r^2 / (h / 4)^2), :321-327
    auto const theta = [support2](float const r2) { return std::exp(-r2 / support2); };

    std::vector<std::size_t> source_order;  // the shuffled index range of :318-319 and :345-347, sample last
    {
        std::vector<char> chosen(J, 0);
        for (u64 i = 0; i < I; ++i) chosen[sample[i]] = 1;
        for (u64 j = 0; j < J; ++j)
            if (!chosen[j]) source_order.push_back(j);
        source_order.insert(source_order.end(), sample, sample + I);
    }
    std::vector<point_type> moving(I), next(I);  // x and x' of the header
    for (u64 i = 0; i < I; ++i) moving[i] = source[sample[i]];
    next = moving;
    std::vector<std::size_t> sample_ids(I);
    std::iota(sample_ids.begin(), sample_ids.end(), std::size_t{0});
    std::vector<float> density(J, 1.f), repulsion_weight(I, 1.f);  // v_j and w_i, 1 unless uniform (:310-313)
    WlopCoords const source_coords{&source}, moving_coords{&moving};
    WlopWeights const density_of{&density}, weight_of{&repulsion_weight};

    pcp::kdtree::construction_params_t params;  // :360-363
    params.compute_max_depth = true;
    params.construction = pcp::kdtree::construction_t::nth_element;
    params.max_elements_per_leaf = 64u;
    kdtree const source_tree{source_order.begin(), source_order.end(), source_coords, params};
    if (uniform)  // :371-381: written in source order, read by point index (DESIGN.md 'Semantics', WLOP densities)
        for (u64 p = 0; p < J; ++p) density[p] = wd::compute_vj(source_order[p], h, source_tree, source_coords, theta);
    for (u64 it = 0; it < K; ++it) {  // :383-425
        kdtree const sample_tree{sample_ids.begin(), sample_ids.end(), moving_coords, params};
        if (uniform)
            for (u64 i = 0; i < I; ++i) repulsion_weight[i] = wd::compute_wi(i, h, sample_tree, moving_coords, theta);
        for (u64 i = 0; i < I; ++i) {
            auto const m = wd::solve_first_energy_median(i, h, source_tree, source_coords, moving_coords, density_of, theta);
            auto const f = wd::solve_second_energy_repulsion_force(i, h, mu, sample_tree, moving_coords, weight_of, theta);
            next[i] = point_type{m.x() + f.x(), m.y() + f.y(), m.z() + f.z()};
        }
        moving = next;
    }
    for (u64 i = 0; i < I; ++i) {  // :427
        out[3 * i] = next[i].x();
        out[3 * i + 1] = next[i].y();
        out[3 * i + 2] = next[i].z();
    }
}

// The public pcp::algorithm::wlop::wlop (its sample drawn from std::random_device): I output points.
void ref_wlop_public(float const* xyz, u64 J, u64 I, double mu, double h, u64 K, int uniform, float* out)
{
    std::vector<point_type> const P = to_points(xyz, J);
    std::vector<std::size_t> ids(J);
    std::iota(ids.begin(), ids.end(), std::size_t{0});
    pcp::algorithm::wlop::params_t params;
    params.I = I;
    params.mu = mu;
    params.h = h;
    params.k = K;
    params.uniform = uniform != 0;
    std::vector<point_type> res;
    pcp::algorithm::wlop::wlop(ids.begin(), ids.end(), std::back_inserter(res), [&](std::size_t i) { return P[i]; }, params);
    for (std::size_t i = 0; i < res.size() && i < I; ++i) {
        out[3 * i] = res[i].x();
        out[3 * i + 1] = res[i].y();
        out[3 * i + 2] = res[i].z();
    }
}

} // extern "C"
