// The last step of "floor -> walls -> cluster the rest -> objects" with pcp::gpu::label_objects (include/pcp/gpu/objects.hpp) on a
// hand-made set: the corners of two boxes under the labels 7 and 3 with their rows interleaved, a lattice of 5 x 5 x 3 points under the
// label 40, a pair under the label 9 that the size filter rejects, rows without a label and one that is not finite.
// tests/test_gpu_objects.py compares what is printed with the Python call and the model (tests/objects_model.py) on the printed set.
// usage: objects_shape
// prints one JSON object (floats and doubles as their bits); exit status 0 when the calls agree with each other
#include <pcp/gpu/objects.hpp>

#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

namespace {
template <class U, class T>
U bits(T v)
{
    static_assert(sizeof(U) == sizeof(T), "same size");
    U u;
    std::memcpy(&u, &v, sizeof(u));
    return u;
}
template <class T>
std::string list(std::vector<T> const& v)
{
    std::string s = "[";
    for (std::size_t i = 0; i < v.size(); ++i) s += (i ? ", " : "") + std::to_string(v[i]);
    return s + "]";
}
std::string list_bits(std::vector<float> const& v)
{
    std::vector<std::uint32_t> u;
    for (float f : v) u.push_back(bits<std::uint32_t>(f));
    return list(u);
}
std::string list_bits(std::vector<double> const& v)
{
    std::vector<std::uint64_t> u;
    for (double f : v) u.push_back(bits<std::uint64_t>(f));
    return list(u);
}
std::string result(pcp::gpu::label_objects_result_t const& r)
{
    return "{\"labels\": " + list(r.labels) + ", \"counts\": " + list(r.counts) + ", \"first_row\": " + list(r.first_row) + ", \"offsets\": " +
           list(r.offsets) + ", \"rows\": " + list(r.rows) + ", \"centroid\": " + list_bits(r.centroid) + ", \"cov\": " + list_bits(r.covariance) +
           ", \"aabb\": " + list_bits(r.aabb) + ", \"obb\": " + list_bits(r.obb) + ", \"object_of_row\": " + list(r.object_of_row) +
           ", \"skipped\": " + std::to_string(r.skipped) + "}";
}
} // namespace

int main()
{
    std::uint32_t const none = PCPX_OBJECTS_NONE;
    std::vector<float> p;
    std::vector<std::uint32_t> labels;
    auto add = [&](float x, float y, float z, std::uint32_t label) {
        p.insert(p.end(), {x, y, z});
        labels.push_back(label);
    };
    for (int c = 0; c < 8; ++c) { // two boxes, corner by corner: 1 x 2 x 4 at the origin under 7, 4 x 1 x 2 at (10, 20, 30) under 3
        add(static_cast<float>(c & 1), 2.f * static_cast<float>((c >> 1) & 1), 4.f * static_cast<float>((c >> 2) & 1), 7u);
        add(10.f + 4.f * static_cast<float>(c & 1), 20.f + static_cast<float>((c >> 1) & 1), 30.f + 2.f * static_cast<float>((c >> 2) & 1), 3u);
    }
    add(-5.f, -5.f, -5.f, none);
    for (int i = 0; i < 5; ++i)
        for (int j = 0; j < 5; ++j)
            for (int k = 0; k < 3; ++k) add(100.f + 0.5f * static_cast<float>(i), 0.25f * static_cast<float>(j), -8.f + 0.125f * static_cast<float>(k), 40u);
    add(50.f, 50.f, 50.f, 9u);
    add(51.f, 50.f, 50.f, 9u);
    add(std::numeric_limits<float>::infinity(), 0.f, 0.f, 7u);
    add(0.f, 0.f, 0.f, none);
    std::size_t const n = labels.size();

    pcp::gpu::label_objects_options_t options;
    options.skip_none = true;
    options.min_size  = 3;
    auto const objects = pcp::gpu::label_objects(p.data(), labels.data(), n, options);
    options.max_size   = 8;
    auto const small   = pcp::gpu::label_objects(p.data(), labels.data(), n, options);
    auto const nothing = pcp::gpu::label_objects(p.data(), labels.data(), 0);

    bool agree = objects.size() == 3 && objects.labels == std::vector<std::uint32_t>{3u, 7u, 40u} &&
                 objects.counts == std::vector<std::uint32_t>{8u, 8u, 75u} && objects.skipped == 3 && objects.rows.size() == 91 &&
                 objects.first_row == std::vector<std::uint32_t>{1u, 0u, 17u} && small.size() == 2 && small.rows.size() == 16 && nothing.size() == 0 &&
                 nothing.offsets == std::vector<std::uint32_t>{0u} && nothing.object_of_row.empty();
    // the boxes' centres and half sizes, exact: the corners are small integers
    if (agree) {
        double const want_centre[2][3] = {{12.0, 20.5, 31.0}, {0.5, 1.0, 2.0}}, want_half[2][3] = {{2.0, 1.0, 0.5}, {2.0, 1.0, 0.5}};
        for (int o = 0; o < 2; ++o)
            for (int a = 0; a < 3; ++a) {
                agree = agree && objects.centroid[static_cast<std::size_t>(3 * o + a)] == want_centre[o][a];
                double const centre = objects.obb[static_cast<std::size_t>(15 * o + a)], half = objects.obb[static_cast<std::size_t>(15 * o + 12 + a)];
                agree = agree && centre > want_centre[o][a] - 1e-12 && centre < want_centre[o][a] + 1e-12;
                agree = agree && half > want_half[o][a] - 1e-12 && half < want_half[o][a] + 1e-12;
            }
        agree = agree && objects.aabb[0] == 10.f && objects.aabb[3] == 14.f && objects.aabb[6 + 2] == 0.f && objects.aabb[6 + 5] == 4.f;
    }
    std::printf("{\"p\": %s, \"labels\": %s, \"objects\": %s, \"small\": %s, \"calls_agree\": %s}\n", list_bits(p).c_str(), list(labels).c_str(),
                result(objects).c_str(), result(small).c_str(), agree ? "true" : "false");
    return agree ? 0 : 4;
}
