// Fixed-radius neighbourhoods through the C++ drop-in: algorithm::estimate_normals (both overloads), estimate_tangent_planes and
// average_distances_to_neighbors over an octree of point views, once with pcp::gpu::self_range_map(octree, r) (one launch of the
// sphere walk's moments form each), once with pcp::gpu::range_map(octree, view map, r) (one batch call each), and once with the
// reference-style lambda `[&](auto const& p) { return octree.range_search(sphere_t{p, r}, view map); }` through the generic path
// (a range search per element, then pcp::estimate_normal's two-pass float arithmetic).  The maps must agree with the lambda:
// exactly on the neighbourhood sizes; for normals, 1 - |cos| <= 1e-5 on the rows with n >= 3 whose double-precision scatter
// matrix has lambda0 <= 0.5 lambda1 (the worst of the other rows is reported); centroids within 2e-6 x the cloud's extent;
// mean distances within 1e-5 relative.
// usage: range_neighbourhoods_shape <in.ply> <radius>
// prints one JSON object; exit status 0 when every check holds
#include <pcp/pcp.hpp>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <execution>
#include <filesystem>
#include <initializer_list>
#include <utility>
#include <vector>

namespace {
// eigenvalues of a symmetric 3x3 matrix (cyclic Jacobi, double), ascending
std::array<double, 3> eigenvalues(std::array<double, 9> a)
{
    for (int sweep = 0; sweep < 50; ++sweep)
    {
        double const off = a[1] * a[1] + a[2] * a[2] + a[5] * a[5];
        if (off < 1e-300) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q)
            {
                double const apq = a[3 * p + q];
                if (apq == 0.) continue;
                double const theta = (a[3 * q + q] - a[3 * p + p]) / (2. * apq);
                double const t     = (theta >= 0. ? 1. : -1.) / (std::fabs(theta) + std::sqrt(theta * theta + 1.));
                double const c = 1. / std::sqrt(t * t + 1.), s = t * c;
                for (int k = 0; k < 3; ++k)  // A <- J^T A J
                {
                    double const akp = a[3 * k + p], akq = a[3 * k + q];
                    a[3 * k + p] = c * akp - s * akq;
                    a[3 * k + q] = s * akp + c * akq;
                }
                for (int k = 0; k < 3; ++k)
                {
                    double const apk = a[3 * p + k], aqk = a[3 * q + k];
                    a[3 * p + k] = c * apk - s * aqk;
                    a[3 * q + k] = s * apk + c * aqk;
                }
            }
    }
    std::array<double, 3> l{a[0], a[4], a[8]};
    std::sort(l.begin(), l.end());
    return l;
}
} // namespace

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    using point_type      = pcp::point_t;
    using point_view_type = pcp::point_view_t;
    using normal_type     = pcp::normal_t;
    using plane_type      = pcp::common::plane3d_t;
    float const r         = std::strtof(argv[2], nullptr);

    auto [points, unused] = pcp::io::read_ply<point_type, normal_type>(std::filesystem::path{argv[1]});
    (void)unused;
    if (points.empty()) return 1;
    std::size_t const n = points.size();
    std::vector<point_view_type> views;
    views.reserve(n);
    for (auto& p : points) views.push_back(point_view_type{&p});
    auto const view_map = [](point_view_type const& p) { return p; };
    pcp::basic_linked_octree_t<point_view_type> octree{views.begin(), views.end(), view_map};
    if (octree.size() != n) return 3;

    auto const self_map  = pcp::gpu::self_range_map(octree, r);
    auto const batch_map = pcp::gpu::range_map(octree, view_map, r);
    auto const lambda    = [&](point_view_type const& p) {
        pcp::sphere_t<point_type> sphere{};
        sphere.position = point_type{p};
        sphere.radius   = r;
        return octree.range_search(sphere, view_map);
    };
    auto const keep_normal = pcp::algorithm::default_normal_transform<point_view_type, normal_type>;
    auto const keep_plane  = pcp::algorithm::default_plane_transform<point_view_type, plane_type>;

    std::vector<normal_type> n_self(n), n_self_seq, n_batch(n), n_ref(n);
    pcp::algorithm::estimate_normals(std::execution::par, views.begin(), views.end(), n_self.begin(), view_map, self_map, keep_normal);
    pcp::algorithm::estimate_normals(views.begin(), views.end(), std::back_inserter(n_self_seq), view_map, self_map, keep_normal);
    pcp::algorithm::estimate_normals(std::execution::par, views.begin(), views.end(), n_batch.begin(), view_map, batch_map, keep_normal);
    pcp::algorithm::estimate_normals(views.begin(), views.end(), n_ref.begin(), view_map, lambda, keep_normal);

    std::vector<plane_type> p_self(n), p_batch(n), p_ref(n);
    pcp::algorithm::estimate_tangent_planes(std::execution::par, views.begin(), views.end(), p_self.begin(), view_map, self_map, keep_plane);
    pcp::algorithm::estimate_tangent_planes(views.begin(), views.end(), p_batch.begin(), view_map, batch_map, keep_plane);
    pcp::algorithm::estimate_tangent_planes(views.begin(), views.end(), p_ref.begin(), view_map, lambda, keep_plane);

    auto const m_self  = pcp::algorithm::average_distances_to_neighbors(views.begin(), views.end(), view_map, self_map);
    auto const m_batch = pcp::algorithm::average_distances_to_neighbors(views.begin(), views.end(), view_map, batch_map);

    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (auto const& p : points)
    {
        double const c[3] = {p.x(), p.y(), p.z()};
        for (int a = 0; a < 3; ++a) lo[a] = std::min(lo[a], c[a]), hi[a] = std::max(hi[a], c[a]);
    }
    double const extent = std::max({hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]});

    auto one_minus_cos = [](normal_type const& a, normal_type const& b) {
        return 1. - std::fabs(double(a.nx()) * b.nx() + double(a.ny()) * b.ny() + double(a.nz()) * b.nz());
    };
    std::size_t well = 0, failures = 0, small_rows = 0;
    double worst_well = 0., worst_other = 0., worst_centroid = 0., worst_mean = 0.;
    for (std::size_t i = 0; i < n; ++i)
    {
        auto const nb = lambda(views[i]);
        std::size_t const m = nb.size();
        // the double-precision scatter matrix of the neighbourhood: its conditioning decides which tolerance applies
        double mu[3] = {0, 0, 0};
        for (auto const& q : nb) mu[0] += q.x(), mu[1] += q.y(), mu[2] += q.z();
        for (double& v : mu) v /= double(m);
        std::array<double, 9> c{};
        for (auto const& q : nb)
        {
            double const d[3] = {q.x() - mu[0], q.y() - mu[1], q.z() - mu[2]};
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) c[3 * a + b] += d[a] * d[b];
        }
        auto const l = eigenvalues(c);
        bool const conditioned = m >= 3 && l[0] <= 0.5 * l[1] && l[1] > 1e-9 * l[2];  // (not collinear)
        using normal_pair = std::pair<normal_type const*, normal_type const*>;  // (range map, lambda)
        for (normal_pair const& pr : {normal_pair{&n_self[i], &n_ref[i]}, normal_pair{&n_self_seq[i], &n_ref[i]}, normal_pair{&n_batch[i], &n_ref[i]},
                                      normal_pair{&p_self[i].normal(), &p_ref[i].normal()}, normal_pair{&p_batch[i].normal(), &p_ref[i].normal()}})
        {
            double const e = one_minus_cos(*pr.first, *pr.second);
            if (conditioned) worst_well = std::max(worst_well, e);
            else worst_other = std::max(worst_other, e);
            if (conditioned && !(e <= 1e-5)) ++failures;
        }
        well += conditioned ? 1u : 0u;
        small_rows += m < 3 ? 1u : 0u;
        for (plane_type const* got : {&p_self[i], &p_batch[i]})
        {
            double const e = std::max({std::fabs(double(got->point().x()) - mu[0]), std::fabs(double(got->point().y()) - mu[1]),
                                       std::fabs(double(got->point().z()) - mu[2])});
            worst_centroid = std::max(worst_centroid, e / extent);
            if (!(e <= 2e-6 * extent)) ++failures;
        }
        double dsum = 0.;
        for (auto const& q : nb)
        {
            double const d[3] = {double(q.x()) - views[i].x(), double(q.y()) - views[i].y(), double(q.z()) - views[i].z()};
            dsum += std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        }
        double const mean = dsum / double(m);
        for (float got : {m_self[i], m_batch[i]})
        {
            double const e = std::fabs(double(got) - mean) / std::max(mean, 1e-30);
            worst_mean = std::max(worst_mean, mean > 0. ? e : std::fabs(double(got)));
            if (!(mean > 0. ? e <= 1e-5 : got == 0.f)) ++failures;
        }
    }
    std::printf("{\"points\": %zu, \"radius\": %.9g, \"conditioned_rows\": %zu, \"rows_below_3\": %zu, \"worst_1mcos_conditioned\": %.3e, "
                "\"worst_1mcos_other\": %.3e, \"worst_centroid_over_extent\": %.3e, \"worst_mean_rel\": %.3e, \"failures\": %zu}\n",
                n, double(r), well, small_rows, worst_well, worst_other, worst_centroid, worst_mean, failures);
    return failures == 0 && n_self_seq.size() == n ? 0 : 4;
}
