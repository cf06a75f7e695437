// pcp::gpu::label_objects -- objects from labels on the GPU (include/pcpx_objects.h): the rows of every label,
// its size, centroid, covariance, axis-aligned box and oriented box, with the minimum / maximum size filter of PCL's
// EuclideanClusterExtraction, objects in ascending label order and every bit defined (the oriented box: given its axes).  Not part of
// the reference API: the reference has no clustering.  No container is involved: the cloud is a flat row-major x, y, z array and the
// labels one std::uint32_t per row, as DeviceIndex::cluster and its kin write them.
#ifndef PCP_GPU_OBJECTS_HPP
#define PCP_GPU_OBJECTS_HPP

#include "pcp/gpu/device_index.hpp"
#include "pcpx_objects.h"

#include <cstddef>
#include <cstdint>
#include <vector>

namespace pcp {
namespace gpu {

struct label_objects_options_t
{
    bool skip_none           = false; // rows labelled `none_label` are in no object
    std::uint32_t none_label = PCPX_OBJECTS_NONE;
    std::uint32_t min_size   = 1u;
    std::uint32_t max_size   = 0u; // 0: no upper bound
    int device               = 0;
};

struct label_objects_result_t
{
    std::vector<std::uint32_t> labels;        // S, ascending
    std::vector<std::uint32_t> counts;        // S: the members of every object
    std::vector<std::uint32_t> first_row;     // S: the lowest member row
    std::vector<std::uint32_t> offsets;       // S + 1: object o's rows are rows[offsets[o] .. offsets[o + 1])
    std::vector<std::uint32_t> rows;          // offsets[S]: the member rows by object, ascending within one
    std::vector<double> centroid;             // S x 3
    std::vector<double> covariance;           // S x 6: xx, xy, xz, yy, yz, zz
    std::vector<float> aabb;                  // S x 6: lo x, y, z, hi x, y, z
    std::vector<double> obb;                  // S x 15: centre 3, axes e0 e1 e2 row-major 9, half sizes 3
    std::vector<std::uint32_t> object_of_row; // n: PCPX_OBJECTS_NONE for a row in no object
    std::uint64_t skipped = 0;                // rows with a non-finite coordinate or the none label
    std::size_t size() const { return counts.size(); }
};

// points: n x 3; labels: n.  Two calls: the first counts the objects, the second fills arrays of that size.
inline label_objects_result_t label_objects(float const* points, std::uint32_t const* labels, std::size_t n,
                                            label_objects_options_t const& options = {})
{
    pcpx_objects_params p{};
    p.flags      = options.skip_none ? PCPX_OBJECTS_SKIP : 0u;
    p.none_label = options.none_label;
    p.min_size   = options.min_size;
    p.max_size   = options.max_size;
    label_objects_result_t r;
    std::uint64_t count = 0;
    int const sized     = pcpx_label_objects(points, labels, n, &p, 0, options.device, nullptr, &count, nullptr, nullptr, nullptr, nullptr, nullptr,
                                             nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (sized != PCPX_ERR_CAPACITY) check(sized, "pcpx_label_objects");
    std::size_t const S = static_cast<std::size_t>(count), room = S ? S : 1;
    r.labels.resize(room);
    r.counts.resize(room);
    r.first_row.resize(room);
    r.offsets.resize(room + 1);
    r.rows.resize(n ? n : 1);
    r.centroid.resize(room * 3);
    r.covariance.resize(room * 6);
    r.aabb.resize(room * 6);
    r.obb.resize(room * 15);
    r.object_of_row.resize(n ? n : 1);
    check(pcpx_label_objects(points, labels, n, &p, room, options.device, nullptr, &count, r.labels.data(), r.counts.data(), r.first_row.data(),
                             r.offsets.data(), r.rows.data(), r.centroid.data(), r.covariance.data(), r.aabb.data(), r.obb.data(),
                             r.object_of_row.data(), &r.skipped),
          "pcpx_label_objects");
    r.labels.resize(S);
    r.counts.resize(S);
    r.first_row.resize(S);
    r.offsets.resize(S + 1);
    r.rows.resize(r.offsets[S]);
    r.centroid.resize(S * 3);
    r.covariance.resize(S * 6);
    r.aabb.resize(S * 6);
    r.obb.resize(S * 15);
    r.object_of_row.resize(n);
    return r;
}

} // namespace gpu
} // namespace pcp

#endif
