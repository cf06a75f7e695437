// The flow of an ICP example -- a target cloud in an index, a source that is part of it under a small motion, the nearest partners
// under a first pose, the loop -- with pcp::gpu::nearest_posed and pcp::gpu::icp_rigid (include/pcp/gpu/icp.hpp) on a hand-made set:
// a bumpy sheet of 24 x 24 points, every third of them turned by two degrees about z and shifted.
// tests/test_gpu_icp.py compares what is printed with the model (tests/icp_model.py) run on the printed set.
// usage: icp_shape
// prints one JSON object (floats as their bits); exit status 0 when the loop converged
#include <pcp/gpu/icp.hpp>

#include <cmath>
#include <cstdio>
#include <cstring>
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
template <class C>
std::string list_bits64(C const& v)
{
    std::vector<std::uint64_t> u;
    for (double f : v) u.push_back(bits<std::uint64_t>(f));
    return list(u);
}
} // namespace

int main()
{
    constexpr int SIDE = 24;
    std::vector<float> target, source;
    double const c = std::cos(2.0 * 3.14159265358979323846 / 180.0), s = std::sin(2.0 * 3.14159265358979323846 / 180.0);
    for (int i = 0; i < SIDE; ++i) {
        for (int j = 0; j < SIDE; ++j) {
            // (a jittered sheet: no two distances tie, and the bumps pin the motion down)
            float const x = static_cast<float>(i) / 8.f + static_cast<float>((i * 7 + j * 3) % 5) / 64.f;
            float const y = static_cast<float>(j) / 8.f + static_cast<float>((i * 5 + j * 11) % 7) / 96.f;
            float const z = 0.25f * static_cast<float>(std::sin(1.5 * x) * std::cos(1.25 * y)) + 0.05f * x * y;
            target.insert(target.end(), {x, y, z});
            if ((i * SIDE + j) % 3 == 0) {  // the source: the point under the inverse of the motion
                double const dx = x - 0.02, dy = y + 0.015, dz = z - 0.01;
                source.insert(source.end(), {static_cast<float>(c * dx + s * dy), static_cast<float>(-s * dx + c * dy), static_cast<float>(dz)});
            }
        }
    }
    pcp::gpu::device_index_t index;
    index.build(target.data(), target.size() / 3);
    pcp::gpu::transform_t const pose{1., 0., 0., 0.005, 0., 1., 0., 0., 0., 0., 1., 0., 0., 0., 0., 1.};
    float const radius            = 0.2f;
    std::uint32_t const max_iterations = 40;
    auto const near = pcp::gpu::nearest_posed(index, source.data(), source.size() / 3, radius, &pose);
    auto const icp  = pcp::gpu::icp_rigid(index, source.data(), source.size() / 3, radius, &pose, max_iterations);
    std::vector<std::uint32_t> count = icp.count;
    std::vector<double> rms        = icp.rms;
    std::printf("{\"target\": %s, \"source\": %s, \"pose\": %s, \"radius\": %u, \"max_iterations\": %u, \"partner\": %s, \"d2\": %s, "
                "\"icp\": {\"transform\": %s, \"status\": %u, \"iterations\": %u, \"last_count\": %u, \"count\": %s, \"rms\": %s, \"partner\": %s}}\n",
                list_bits(target).c_str(), list_bits(source).c_str(), list_bits64(pose).c_str(), bits<std::uint32_t>(radius), max_iterations,
                list(near.partner).c_str(), list_bits(near.d2).c_str(), list_bits64(icp.transform).c_str(), icp.status, icp.iterations, icp.last_count,
                list(count).c_str(), list_bits64(rms).c_str(), list(icp.partner).c_str());
    return icp.converged() ? 0 : 4;
}
