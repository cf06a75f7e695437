// pcp::gpu::ransac_sphere / ransac_cylinder / sphere_fit / cylinder_fit -- sphere and cylinder detection on the GPU
// (include/pcpx_shapes.h): the sphere or cylinder most points of a cloud lie on, by a fixed number of hypotheses
// from two oriented points each, scored against all points; and the closed-form least-squares sphere or cylinder of a set of points.
// Not part of the reference API: the reference has no model fitting.  As in pcp/gpu/planes.hpp no container is involved: the cloud and
// its normals are flat row-major x, y, z arrays.  The normals' signs play no part.
#ifndef PCP_GPU_SHAPES_HPP
#define PCP_GPU_SHAPES_HPP

#include "pcp/gpu/device_index.hpp"
#include "pcpx_shapes.h"

#include <array>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

namespace pcp {
namespace gpu {

using shape_model_t = std::array<double, 8>;

// axis == nullptr: no axis gate (cylinders only; the axis is normalised here, in double, and rounded once); min_normal_cos < 0: no
// normal gate
struct shape_options_t
{
    std::uint32_t seed   = 0u;
    bool refit           = true;
    float min_radius     = 0.f;
    float max_radius     = std::numeric_limits<float>::infinity();
    float min_normal_sin = 0.1f;
    float min_normal_cos = -1.f;
    float const* axis    = nullptr; // 3 floats
    float min_axis_cos   = 0.f;
    int device           = 0;
};

struct sphere_t
{
    bool found = false;
    std::array<double, 3> center{};
    double radius = 0.;
    std::uint32_t hypothesis = 0;
    shape_model_t model{};              // the winning hypothesis itself (cx, cy, cz, R, 0, 0, 0, 0)
    std::vector<std::uint32_t> inliers; // rows of the cloud, in record order
};

struct cylinder_t
{
    bool found = false;
    std::array<double, 3> point{}, axis{};
    double radius = 0.;
    std::uint32_t hypothesis = 0;
    shape_model_t model{};              // the winning hypothesis itself (px, py, pz, ux, uy, uz, R, 0)
    std::vector<std::uint32_t> inliers;
};

struct shape_fit_result_t
{
    bool ok = false; // false: a degenerate set (zeros and a NaN rms)
    shape_model_t model{};
    double rms = 0.;
};

namespace detail {
inline pcpx_shape_params shape_params(std::uint32_t kind, std::uint64_t hypotheses, float max_distance, shape_options_t const& o)
{
    pcpx_shape_params p{};
    p.hypotheses     = hypotheses;
    p.kind           = kind;
    p.seed           = o.seed;
    p.flags          = (o.refit ? PCPX_SHAPE_REFIT : 0u) | (o.min_normal_cos >= 0.f ? PCPX_SHAPE_NORMALS : 0u) | (o.axis ? PCPX_SHAPE_AXIS : 0u);
    p.max_distance   = max_distance;
    p.min_radius     = o.min_radius;
    p.max_radius     = o.max_radius;
    p.min_normal_sin = o.min_normal_sin;
    p.min_normal_cos = o.min_normal_cos >= 0.f ? o.min_normal_cos : 0.f;
    if (o.axis) {
        double const a[3] = {o.axis[0], o.axis[1], o.axis[2]};
        double const norm = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
        for (int j = 0; j < 3; ++j) p.axis[j] = static_cast<float>(norm > 0. ? a[j] / norm : a[j]); // (a zero axis is refused by the call)
        p.min_axis_cos = o.min_axis_cos;
    }
    p.origin_row = PCPX_SHAPE_ORIGIN_FIRST;
    return p;
}

// the call; best: the refit when it was asked for, else the hypothesis
inline bool ransac_shape(std::uint32_t kind, float const* points, float const* normals, std::size_t n, std::uint64_t hypotheses, float max_distance,
                         shape_options_t const& o, std::uint32_t const* rows, std::size_t rows_count, std::uint32_t& hypothesis, shape_model_t& model,
                         shape_model_t& best, std::vector<std::uint32_t>& inliers)
{
    pcpx_shape_params const p = shape_params(kind, hypotheses, max_distance, o);
    inliers.resize(rows ? rows_count : n);
    std::uint32_t found  = 0;
    std::uint64_t count = 0;
    check(pcpx_shape_ransac(points, n, normals, rows, rows_count, nullptr, &p, o.device, nullptr, &found, &hypothesis, nullptr, inliers.data(), &count,
                            model.data(), o.refit ? best.data() : nullptr),
          "pcpx_shape_ransac");
    inliers.resize(count);
    if (!o.refit) best = model;
    return found != 0;
}
} // namespace detail

// points, normals: n x 3.  rows == nullptr: all n points; else the listed rows (rows_count of them).  A point is an inlier when it
// lies within max_distance of the sphere.  Ties in the inlier count go to the lowest hypothesis.  center and radius: the least-squares
// sphere over the inliers, or with options.refit = false the hypothesis.
inline sphere_t ransac_sphere(float const* points, float const* normals, std::size_t n, std::uint64_t hypotheses, float max_distance,
                              shape_options_t const& options = {}, std::uint32_t const* rows = nullptr, std::size_t rows_count = 0)
{
    sphere_t r;
    shape_model_t best{};
    r.found  = detail::ransac_shape(PCPX_SHAPE_SPHERE, points, normals, n, hypotheses, max_distance, options, rows, rows_count, r.hypothesis, r.model, best, r.inliers);
    r.center = {best[0], best[1], best[2]};
    r.radius = best[3];
    return r;
}

inline cylinder_t ransac_cylinder(float const* points, float const* normals, std::size_t n, std::uint64_t hypotheses, float max_distance,
                                  shape_options_t const& options = {}, std::uint32_t const* rows = nullptr, std::size_t rows_count = 0)
{
    cylinder_t r;
    shape_model_t best{};
    r.found  = detail::ransac_shape(PCPX_SHAPE_CYLINDER, points, normals, n, hypotheses, max_distance, options, rows, rows_count, r.hypothesis, r.model, best, r.inliers);
    r.point  = {best[0], best[1], best[2]};
    r.axis   = {best[3], best[4], best[5]};
    r.radius = best[6];
    return r;
}

// The algebraic least-squares sphere of the points (rows == nullptr: all of them; else the listed rows), float64 throughout.
inline shape_fit_result_t sphere_fit(float const* points, std::size_t n, std::uint32_t const* rows = nullptr, std::size_t rows_count = 0, int device = 0)
{
    shape_fit_result_t r;
    std::uint32_t status = 0;
    check(pcpx_shape_fit(points, n, nullptr, rows, rows_count, nullptr, PCPX_SHAPE_SPHERE, 0u, device, nullptr, r.model.data(), &r.rms, &status), "pcpx_shape_fit");
    r.ok = status == PCPX_SHAPE_FIT_OK;
    return r;
}

// The least-squares cylinder: the axis the normals span least, and the least-squares circle across it.
inline shape_fit_result_t cylinder_fit(float const* points, float const* normals, std::size_t n, std::uint32_t const* rows = nullptr,
                                       std::size_t rows_count = 0, int device = 0)
{
    shape_fit_result_t r;
    std::uint32_t status = 0;
    check(pcpx_shape_fit(points, n, normals, rows, rows_count, nullptr, PCPX_SHAPE_CYLINDER, 0u, device, nullptr, r.model.data(), &r.rms, &status),
          "pcpx_shape_fit");
    r.ok = status == PCPX_SHAPE_FIT_OK;
    return r;
}

} // namespace gpu
} // namespace pcp

#endif
