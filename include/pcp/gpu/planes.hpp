// pcp::gpu::ransac_plane / plane_fit / extract_planes -- plane detection on the GPU (include/pcpx_planes.h): the
// plane most points of a cloud lie on, by a fixed number of three-point hypotheses each scored against all points; the least-squares
// plane of a set of points; and plane after plane, each on the points the earlier ones left.  Not part of the reference API: the
// reference has no model fitting.  No container is involved: the cloud is a flat row-major x, y, z array.  A plane is (n0, n1, n2, d)
// with n . x + d = 0.
#ifndef PCP_GPU_PLANES_HPP
#define PCP_GPU_PLANES_HPP

#include "pcp/gpu/device_index.hpp"
#include "pcpx_planes.h"

#include <array>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace pcp {
namespace gpu {

using plane_t = std::array<double, 4>;

// what is common to ransac_plane and extract_planes; normals == nullptr: no normal gate; axis == nullptr: no axis gate (the axis is
// normalised here, in double, and rounded once)
struct plane_options_t
{
    std::uint32_t seed     = 0u;
    bool refit             = true;
    float const* normals   = nullptr; // n x 3
    float min_normal_cos   = 0.f;
    float const* axis      = nullptr; // 3 floats
    float min_axis_cos     = 0.f;
    int device             = 0;
};

struct ransac_plane_result_t
{
    bool found               = false;
    std::uint32_t hypothesis = 0;
    plane_t plane{};                    // the winning hypothesis itself
    plane_t refit{};                    // the least-squares plane over its inliers (the hypothesis again when refit was not asked for)
    std::vector<std::uint32_t> inliers; // rows of the cloud, in record order
};

struct plane_fit_result_t
{
    plane_t plane{};
    double rms = 0.;
};

struct extract_planes_result_t
{
    std::vector<std::uint32_t> labels; // per point: the round that took it, or PCPX_PLANE_NONE
    std::vector<plane_t> planes, refits;
    std::vector<std::uint32_t> scores;
};

namespace detail {
inline pcpx_plane_params plane_params(std::uint64_t hypotheses, float max_distance, plane_options_t const& o)
{
    pcpx_plane_params p{};
    p.hypotheses   = hypotheses;
    p.seed         = o.seed;
    p.flags        = (o.refit ? PCPX_PLANE_REFIT : 0u) | (o.normals ? PCPX_PLANE_NORMALS : 0u) | (o.axis ? PCPX_PLANE_AXIS : 0u);
    p.max_distance = max_distance;
    p.min_normal_cos = o.min_normal_cos;
    if (o.axis) {
        double const a[3] = {o.axis[0], o.axis[1], o.axis[2]};
        double const norm = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
        for (int j = 0; j < 3; ++j) p.axis[j] = static_cast<float>(norm > 0. ? a[j] / norm : a[j]); // (a zero axis is refused by the call)
        p.min_axis_cos = o.min_axis_cos;
    }
    p.origin_row = PCPX_PLANE_ORIGIN_FIRST;
    return p;
}
} // namespace detail

// points: n x 3.  rows == nullptr: all n points; else the listed rows (rows_count of them).  A point is an inlier when it lies within
// max_distance of the plane (and, under the normal gate, its normal is within the cone).  Ties in the inlier count go to the lowest
// hypothesis.
inline ransac_plane_result_t ransac_plane(float const* points, std::size_t n, std::uint64_t hypotheses, float max_distance,
                                          plane_options_t const& options = {}, std::uint32_t const* rows = nullptr, std::size_t rows_count = 0)
{
    ransac_plane_result_t r;
    r.inliers.resize(rows ? rows_count : n);
    pcpx_plane_params const p = detail::plane_params(hypotheses, max_distance, options);
    std::uint32_t found = 0, score = 0;
    check(pcpx_plane_ransac(points, n, options.normals, rows, rows_count, &p, options.device, &found, &r.hypothesis, &score, r.inliers.data(),
                            r.plane.data(), options.refit ? r.refit.data() : nullptr),
          "pcpx_plane_ransac");
    r.found = found != 0;
    r.inliers.resize(score);
    if (!options.refit) r.refit = r.plane;
    return r;
}

// The plane minimising the sum of squared distances of the points (rows == nullptr: all of them; else the listed rows), float64
// throughout; zeros and a NaN rms with fewer than three usable rows.
inline plane_fit_result_t plane_fit(float const* points, std::size_t n, std::uint32_t const* rows = nullptr, std::size_t rows_count = 0, int device = 0)
{
    plane_fit_result_t r;
    check(pcpx_plane_fit(points, n, rows, rows_count, device, r.plane.data(), &r.rms), "pcpx_plane_fit");
    return r;
}

// Up to max_planes planes, each found on the points the earlier ones left; stops at the first whose score is below min_inliers.
inline extract_planes_result_t extract_planes(float const* points, std::size_t n, std::uint64_t hypotheses, float max_distance,
                                              std::uint32_t min_inliers, std::uint32_t max_planes, plane_options_t const& options = {})
{
    extract_planes_result_t r;
    pcpx_plane_params p = detail::plane_params(hypotheses, max_distance, options);
    p.min_inliers       = min_inliers;
    p.max_planes        = max_planes;
    std::size_t const m = max_planes ? max_planes : 1;
    r.labels.resize(n);
    r.planes.resize(m);
    r.refits.resize(m);
    r.scores.resize(m);
    std::uint32_t count = 0;
    check(pcpx_extract_planes(points, n, options.normals, &p, options.device, r.labels.data(), &count, r.planes[0].data(),
                              options.refit ? r.refits[0].data() : nullptr, r.scores.data()),
          "pcpx_extract_planes");
    r.planes.resize(count);
    r.refits.resize(count);
    r.scores.resize(count);
    if (!options.refit) r.refits = r.planes;
    return r;
}

} // namespace gpu
} // namespace pcp

#endif
