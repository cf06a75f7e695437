// pcp::gpu::gicp_rigid -- Generalized ICP on the GPU (include/pcpx_gicp.h): the loop of pcp::gpu::icp_rigid
// with a plane-to-plane step, from both clouds' normals or from both clouds' covariances.  Not part of the reference API: the
// reference has no registration.  The target is a device_index_t; the source a flat row-major x, y, z array.  Transforms are
// row-major 4 x 4 and take source points to target points.
#ifndef PCP_GPU_GICP_HPP
#define PCP_GPU_GICP_HPP

#include "pcp/gpu/icp.hpp"
#include "pcpx_gicp.h"

#include <cstddef>
#include <cstdint>

namespace pcp {
namespace gpu {

// six floats per row: the upper triangle xx, xy, xz, yy, yz, zz of a covariance
struct covariances_t
{
    float const* rows;
};

namespace detail {
inline icp_result_t gicp_call(device_index_t const& target, float const* source, std::size_t m, float radius, std::uint32_t flags, float const* source_rows,
                              float const* target_rows, float epsilon, transform_t const* pose, std::uint32_t max_iterations)
{
    icp_result_t r;
    r.count.resize(max_iterations);
    r.rms.resize(max_iterations);
    r.partner.resize(m);
    check(pcpx_gicp_rigid(target.handle(), source, m, pose ? pose->data() : nullptr, radius, max_iterations, flags, source_rows, target_rows, epsilon,
                          r.transform.data(), &r.status, &r.iterations, &r.last_count, r.count.data(), r.rms.data(), r.partner.data()),
          "pcpx_gicp_rigid");
    r.count.resize(r.iterations);
    r.rms.resize(r.iterations);
    return r;
}
} // namespace detail

// from normals (m x 3 by source row, n_in x 3 by input row of the target; neither oriented nor of unit length needed): every point's
// covariance is 1 across its normal and `epsilon`, in (0, 1], along it
inline icp_result_t gicp_rigid(device_index_t const& target, float const* source, std::size_t m, float radius, float const* source_normals,
                               float const* target_normals, float epsilon = 1e-3f, transform_t const* pose = nullptr, std::uint32_t max_iterations = 50)
{
    return detail::gicp_call(target, source, m, radius, 0u, source_normals, target_normals, epsilon, pose, max_iterations);
}

// from covariances (m x 6 by source row, n_in x 6 by input row of the target)
inline icp_result_t gicp_rigid(device_index_t const& target, float const* source, std::size_t m, float radius, covariances_t source_cov,
                               covariances_t target_cov, transform_t const* pose = nullptr, std::uint32_t max_iterations = 50)
{
    return detail::gicp_call(target, source, m, radius, PCPX_GICP_COVARIANCES, source_cov.rows, target_cov.rows, 0.f, pose, max_iterations);
}

} // namespace gpu
} // namespace pcp

#endif
