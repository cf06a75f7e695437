// The flow of a Generalized ICP example -- a target cloud in an index, a source that is part of it under a small motion, rough
// normals for both, the loop -- with pcp::gpu::gicp_rigid (include/pcp/gpu/gicp.hpp) on the hand-made set of icp_shape.cpp: a bumpy
// sheet of 24 x 24 points, every third of them turned by two degrees about z and shifted.  Both overloads run: the normals, and the
// covariances diag(1, 1, epsilon) those normals stand for.
// tests/test_gpu_gicp.py compares what is printed with the model (tests/gicp_model.py) run on the printed set.
// usage: gicp_shape
// prints one JSON object (floats as their bits); exit status 0 when both loops converged
#include <pcp/gpu/gicp.hpp>

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
std::string run(pcp::gpu::icp_result_t const& r)
{
    return "{\"transform\": " + list_bits64(r.transform) + ", \"status\": " + std::to_string(r.status) + ", \"iterations\": " +
           std::to_string(r.iterations) + ", \"last_count\": " + std::to_string(r.last_count) + ", \"count\": " + list(r.count) + ", \"rms\": " +
           list_bits64(r.rms) + ", \"partner\": " + list(r.partner) + "}";
}
} // namespace

int main()
{
    constexpr int SIDE = 24;
    std::vector<float> target, source;
    double const c = std::cos(2.0 * 3.14159265358979323846 / 180.0), s = std::sin(2.0 * 3.14159265358979323846 / 180.0);
    for (int i = 0; i < SIDE; ++i) {
        for (int j = 0; j < SIDE; ++j) {
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
    std::size_t const n = target.size() / 3, m = source.size() / 3;
    // rough normals: straight up, of length 2 on the target (the length does not matter); epsilon a quarter
    float const epsilon = 0.25f;
    std::vector<float> target_normals, source_normals, target_cov, source_cov;
    for (std::size_t i = 0; i < n; ++i) target_normals.insert(target_normals.end(), {0.f, 0.f, 2.f});
    for (std::size_t i = 0; i < m; ++i) source_normals.insert(source_normals.end(), {0.f, 0.f, -1.f});
    for (std::size_t i = 0; i < n; ++i) target_cov.insert(target_cov.end(), {1.f, 0.f, 0.f, 1.f, 0.f, epsilon});
    for (std::size_t i = 0; i < m; ++i) source_cov.insert(source_cov.end(), {1.f, 0.f, 0.f, 1.f, 0.f, epsilon});
    pcp::gpu::device_index_t index;
    index.build(target.data(), n);
    pcp::gpu::transform_t const pose{1., 0., 0., 0.005, 0., 1., 0., 0., 0., 0., 1., 0., 0., 0., 0., 1.};
    float const radius                 = 0.2f;
    std::uint32_t const max_iterations = 40;
    auto const by_normals = pcp::gpu::gicp_rigid(index, source.data(), m, radius, source_normals.data(), target_normals.data(), epsilon, &pose, max_iterations);
    auto const by_cov     = pcp::gpu::gicp_rigid(index, source.data(), m, radius, pcp::gpu::covariances_t{source_cov.data()},
                                             pcp::gpu::covariances_t{target_cov.data()}, &pose, max_iterations);
    std::printf("{\"target\": %s, \"source\": %s, \"pose\": %s, \"radius\": %u, \"epsilon\": %u, \"max_iterations\": %u, \"target_normals\": %s, "
                "\"source_normals\": %s, \"target_cov\": %s, \"source_cov\": %s, \"normals\": %s, \"covariances\": %s}\n",
                list_bits(target).c_str(), list_bits(source).c_str(), list_bits64(pose).c_str(), bits<std::uint32_t>(radius), bits<std::uint32_t>(epsilon),
                max_iterations, list_bits(target_normals).c_str(), list_bits(source_normals).c_str(), list_bits(target_cov).c_str(),
                list_bits(source_cov).c_str(), run(by_normals).c_str(), run(by_cov).c_str());
    return by_normals.converged() && by_cov.converged() ? 0 : 4;
}
