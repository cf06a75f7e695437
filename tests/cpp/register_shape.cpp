// The flow of a registration example -- two clouds, their correspondences, the pose most of them agree on, the least-squares fit --
// with pcp::gpu::ransac_rigid and pcp::gpu::rigid_fit (include/pcp/gpu/registration.hpp) on a hand-made set: points on a grid of
// eighths under an exact quarter turn about z plus a shift, every fourth target an outlier, one pair out of range.
// tests/test_gpu_register.py compares what is printed with the model (tests/register_model.py) run on the printed set.
// usage: register_shape
// prints one JSON object (floats as their bits); exit status 0 when the two overloads agree
#include <pcp/gpu/registration.hpp>

#include <array>
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
std::string list_bits(pcp::gpu::transform_t const& v)
{
    std::vector<std::uint64_t> u;
    for (double f : v) u.push_back(bits<std::uint64_t>(f));
    return list(u);
}
std::string result(pcp::gpu::ransac_result_t const& r)
{
    return std::string("{\"found\": ") + (r.found ? "1" : "0") + ", \"hypothesis\": " + std::to_string(r.hypothesis) +
           ", \"inliers\": " + list(r.inliers) + ", \"transform\": " + list_bits(r.transform) + ", \"refit\": " + list_bits(r.refit) + "}";
}
} // namespace

int main()
{
    constexpr std::size_t N = 16;
    std::vector<float> p, q;
    std::vector<std::uint32_t> pairs;
    std::vector<pcp::gpu::correspondence_t> matched;
    for (std::size_t k = 0; k < N; ++k) {
        float const x = static_cast<float>(k * 37 % 11) / 4.f, y = static_cast<float>(k * 53 % 13) / 8.f, z = static_cast<float>(k * 71 % 7) / 2.f;
        p.insert(p.end(), {x, y, z});
        if (k % 4 == 3) q.insert(q.end(), {x + 3.f, 2.f * y, -z});         // an outlier
        else q.insert(q.end(), {1.f - y, x - 2.f, z + 0.5f});              // a quarter turn about z, then (1, -2, 0.5)
        pairs.insert(pairs.end(), {static_cast<std::uint32_t>(k), static_cast<std::uint32_t>(k)});
        matched.push_back(pcp::gpu::correspondence_t{static_cast<std::uint32_t>(k), static_cast<std::uint32_t>(k), 0.f});
    }
    pairs.insert(pairs.end(), {3u, static_cast<std::uint32_t>(N)}); // a target that does not exist
    matched.push_back(pcp::gpu::correspondence_t{3u, static_cast<std::uint32_t>(N), 0.f});

    std::uint64_t const hypotheses = 256;
    float const max_distance = 0.01f, similarity = 0.9f;
    std::uint32_t const seed = 7;
    auto const flat   = pcp::gpu::ransac_rigid(p.data(), N, q.data(), N, pairs.data(), pairs.size() / 2, hypotheses, max_distance, seed, similarity);
    auto const vec    = pcp::gpu::ransac_rigid(p.data(), N, q.data(), N, matched, hypotheses, max_distance, seed, similarity);
    auto const plain  = pcp::gpu::ransac_rigid(p.data(), N, q.data(), N, matched, hypotheses, max_distance, seed, 0.f, false);
    auto const nobody = pcp::gpu::ransac_rigid(p.data(), N, q.data(), N, pairs.data(), 2, hypotheses, max_distance, seed);
    auto const fit    = pcp::gpu::rigid_fit(p.data(), N, q.data(), N, pairs.data(), pairs.size() / 2, flat.inliers.data(), flat.inliers.size());
    auto const all    = pcp::gpu::rigid_fit(p.data(), N, q.data(), N, pairs.data(), pairs.size() / 2);

    bool const agree = result(flat) == result(vec) && plain.refit == plain.transform && list_bits(fit.transform) == list_bits(flat.refit);
    std::printf("{\"p\": %s, \"q\": %s, \"pairs\": %s, \"hypotheses\": %llu, \"seed\": %u, \"max_distance\": %u, \"edge_similarity\": %u, "
                "\"gated\": %s, \"plain\": %s, \"two_pairs\": %s, \"fit_inliers\": {\"transform\": %s, \"rms\": %llu}, "
                "\"fit_all\": {\"transform\": %s, \"rms\": %llu}, \"overloads_agree\": %s}\n",
                list_bits(p).c_str(), list_bits(q).c_str(), list(pairs).c_str(), static_cast<unsigned long long>(hypotheses), seed,
                bits<std::uint32_t>(max_distance), bits<std::uint32_t>(similarity), result(flat).c_str(), result(plain).c_str(),
                result(nobody).c_str(), list_bits(fit.transform).c_str(), static_cast<unsigned long long>(bits<std::uint64_t>(fit.rms)),
                list_bits(all.transform).c_str(), static_cast<unsigned long long>(bits<std::uint64_t>(all.rms)), agree ? "true" : "false");
    return agree ? 0 : 4;
}
