// pcp::gpu::match_nearest / match_correspondences -- descriptor matching on the GPU (include/pcpx_match.h):
// for every row of one set of descriptors the exact nearest and second nearest row of another, by brute force over all pairs, and
// the correspondences that pass Lowe's ratio test and the mutual test.  Not part of the reference API: the reference has no
// descriptors.  No container is involved: the sets are vectors of std::array<float, D> (what pcp::gpu::fpfh returns) or flat
// row-major arrays.  Distances are squared, float32, summed in column order without FMA; ties go to the lower index.
#ifndef PCP_GPU_MATCHING_HPP
#define PCP_GPU_MATCHING_HPP

#include "pcp/gpu/device_index.hpp"
#include "pcpx_match.h"

#include <array>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace pcp {
namespace gpu {

// per source row: the nearest and second nearest target rows (PCPX_MATCH_NONE and +inf where there is none)
struct nearest_matches_t
{
    std::vector<std::uint32_t> index, second_index;
    std::vector<float> d2, second_d2;
};

struct correspondence_t
{
    std::uint32_t source, target;
    float d2;
};

// src: m x dims, tgt: n x dims, row-major float32, 1 <= dims <= PCPX_MATCH_MAX_DIMS.  skip_zero_rows: rows of zeros (descriptors that
// could not be computed) take no part on either side.
inline nearest_matches_t match_nearest(float const* src, std::size_t m, float const* tgt, std::size_t n, std::uint32_t dims,
                                       bool skip_zero_rows = false, int device = 0)
{
    nearest_matches_t r;
    r.index.resize(m);
    r.second_index.resize(m);
    r.d2.resize(m);
    r.second_d2.resize(m);
    check(pcpx_match_nearest(src, m, tgt, n, dims, skip_zero_rows ? PCPX_MATCH_SKIP_ZERO_ROWS : 0u, device, r.index.data(), r.d2.data(),
                             r.second_index.data(), r.second_d2.data()),
          "pcpx_match_nearest");
    return r;
}

// The (source, target = the source's nearest target) pairs, ascending source, that pass d_best <= max_ratio * d_second -- evaluated
// as d2_best <= (max_ratio * max_ratio) * d2_second in float32; 1 is no test -- and, with `mutual`, whose source is the target's
// nearest source too.
inline std::vector<correspondence_t> match_correspondences(float const* src, std::size_t m, float const* tgt, std::size_t n, std::uint32_t dims,
                                                           float max_ratio = 1.f, bool mutual = true, bool skip_zero_rows = false, int device = 0)
{
    std::vector<std::uint32_t> pairs(2 * m);
    std::vector<float> d2(m);
    std::uint64_t count  = 0;
    std::uint32_t const flags = (skip_zero_rows ? PCPX_MATCH_SKIP_ZERO_ROWS : 0u) | (mutual ? PCPX_MATCH_MUTUAL : 0u);
    check(pcpx_match_correspondences(src, m, tgt, n, dims, max_ratio * max_ratio, flags, device, pairs.data(), d2.data(), &count),
          "pcpx_match_correspondences");
    std::vector<correspondence_t> out(static_cast<std::size_t>(count));
    for (std::size_t k = 0; k < out.size(); ++k) out[k] = correspondence_t{pairs[2 * k], pairs[2 * k + 1], d2[k]};
    return out;
}

// the same over vectors of fixed-size descriptors (std::array<float, D> is D dense floats)
template <std::size_t D>
nearest_matches_t match_nearest(std::vector<std::array<float, D>> const& src, std::vector<std::array<float, D>> const& tgt,
                                bool skip_zero_rows = false, int device = 0)
{
    static_assert(D >= 1 && D <= PCPX_MATCH_MAX_DIMS && sizeof(std::array<float, D>) == D * sizeof(float), "1 .. 64 dense floats");
    return match_nearest(src.empty() ? nullptr : src.front().data(), src.size(), tgt.empty() ? nullptr : tgt.front().data(), tgt.size(),
                         static_cast<std::uint32_t>(D), skip_zero_rows, device);
}

template <std::size_t D>
std::vector<correspondence_t> match_correspondences(std::vector<std::array<float, D>> const& src, std::vector<std::array<float, D>> const& tgt,
                                                    float max_ratio = 1.f, bool mutual = true, bool skip_zero_rows = false, int device = 0)
{
    static_assert(D >= 1 && D <= PCPX_MATCH_MAX_DIMS && sizeof(std::array<float, D>) == D * sizeof(float), "1 .. 64 dense floats");
    return match_correspondences(src.empty() ? nullptr : src.front().data(), src.size(), tgt.empty() ? nullptr : tgt.front().data(), tgt.size(),
                                 static_cast<std::uint32_t>(D), max_ratio, mutual, skip_zero_rows, device);
}

} // namespace gpu
} // namespace pcp

#endif
