// pcp::gpu::nearest_posed / icp_rigid -- iterative closest point on the GPU (include/pcpx_icp.h): the exact
// nearest indexed point of every source point under a pose, and the loop around it, point to point or point to plane.  Not part of
// the reference API: the reference has no registration.  The target is a device_index_t; the source a flat row-major x, y, z array.
// Transforms are row-major 4 x 4 and take source points to target points -- what pcp::gpu::ransac_rigid returns goes straight in.
#ifndef PCP_GPU_ICP_HPP
#define PCP_GPU_ICP_HPP

#include "pcp/gpu/device_index.hpp"
#include "pcp/gpu/registration.hpp"
#include "pcpx_icp.h"

#include <cstddef>
#include <cstdint>
#include <vector>

namespace pcp {
namespace gpu {

struct nearest_posed_result_t
{
    std::vector<std::uint32_t> partner; // by source row; PCPX_ICP_NONE where there is none
    std::vector<float> d2;              // +inf there
};

struct icp_result_t
{
    transform_t transform{};
    std::uint32_t status     = 0; // PCPX_ICP_EXHAUSTED, _CONVERGED, _STARVED or _DEGENERATE
    std::uint32_t iterations = 0; // pose updates made
    std::uint32_t last_count = 0; // partners of the last search
    std::vector<std::uint32_t> count; // per update
    std::vector<double> rms;          // per update
    std::vector<std::uint32_t> partner; // the last partner list, by source row
    bool converged() const { return status == PCPX_ICP_CONVERGED; }
};

// the smallest (squared distance, input index) among the indexed points within `radius` of every source point moved by `pose`
// (nullptr: the identity): ties go to the lowest input index
inline nearest_posed_result_t nearest_posed(device_index_t const& target, float const* source, std::size_t m, float radius,
                                            transform_t const* pose = nullptr)
{
    nearest_posed_result_t r;
    r.partner.resize(m);
    r.d2.resize(m);
    check(pcpx_nearest_posed(target.handle(), source, m, pose ? pose->data() : nullptr, radius, r.partner.data(), r.d2.data()), "pcpx_nearest_posed");
    return r;
}

// ICP from `pose` (nullptr: the identity): point to point, or point to plane with the target's normals (n_in x 3, by input row)
inline icp_result_t icp_rigid(device_index_t const& target, float const* source, std::size_t m, float radius, transform_t const* pose = nullptr,
                              std::uint32_t max_iterations = 50, float const* target_normals = nullptr)
{
    icp_result_t r;
    r.count.resize(max_iterations);
    r.rms.resize(max_iterations);
    r.partner.resize(m);
    check(pcpx_icp_rigid(target.handle(), source, m, pose ? pose->data() : nullptr, radius, max_iterations, target_normals ? PCPX_ICP_POINT_TO_PLANE : 0u,
                         target_normals, r.transform.data(), &r.status, &r.iterations, &r.last_count, r.count.data(), r.rms.data(), r.partner.data()),
          "pcpx_icp_rigid");
    r.count.resize(r.iterations);
    r.rms.resize(r.iterations);
    return r;
}

} // namespace gpu
} // namespace pcp

#endif
