// The flow of a plane-detection example -- a cloud, its dominant plane, the least-squares fit, plane after plane -- with
// pcp::gpu::ransac_plane, pcp::gpu::plane_fit and pcp::gpu::extract_planes (include/pcp/gpu/planes.hpp) on a hand-made set: a 6 x 6
// grid of eighths at z = 1/2, a 5 x 5 one at x = -1, and eight points off both.
// tests/test_gpu_planes.py compares what is printed with the model (tests/planes_model.py) run on the printed set.
// usage: planes_shape
// prints one JSON object (floats as their bits); exit status 0 when the calls agree with each other
#include <pcp/gpu/planes.hpp>

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
std::string list_bits(pcp::gpu::plane_t const& v)
{
    std::vector<std::uint64_t> u;
    for (double f : v) u.push_back(bits<std::uint64_t>(f));
    return list(u);
}
std::string result(pcp::gpu::ransac_plane_result_t const& r)
{
    return std::string("{\"found\": ") + (r.found ? "1" : "0") + ", \"hypothesis\": " + std::to_string(r.hypothesis) +
           ", \"inliers\": " + list(r.inliers) + ", \"plane\": " + list_bits(r.plane) + ", \"refit\": " + list_bits(r.refit) + "}";
}
} // namespace

int main()
{
    std::vector<float> p;
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) p.insert(p.end(), {static_cast<float>(i) / 8.f, static_cast<float>(j) / 8.f, 0.5f});
    for (int i = 0; i < 5; ++i)
        for (int j = 0; j < 5; ++j) p.insert(p.end(), {-1.f, static_cast<float>(i) / 8.f, static_cast<float>(j) / 8.f - 1.f});
    for (int k = 0; k < 8; ++k) p.insert(p.end(), {static_cast<float>(k * 5 % 7) / 4.f + 2.f, static_cast<float>(k * 3 % 5) / 2.f, static_cast<float>(k) + 3.f});
    std::size_t const n = p.size() / 3;

    std::uint64_t const hypotheses = 256;
    float const max_distance       = 0.01f;
    pcp::gpu::plane_options_t options;
    options.seed = 7;
    auto const best = pcp::gpu::ransac_plane(p.data(), n, hypotheses, max_distance, options);
    pcp::gpu::plane_options_t plain_options = options;
    plain_options.refit                     = false;
    auto const plain = pcp::gpu::ransac_plane(p.data(), n, hypotheses, max_distance, plain_options);
    std::vector<std::uint32_t> const two{1u, 40u};
    auto const nobody = pcp::gpu::ransac_plane(p.data(), n, hypotheses, max_distance, options, two.data(), two.size());
    auto const fit    = pcp::gpu::plane_fit(p.data(), n, best.inliers.data(), best.inliers.size());
    auto const all    = pcp::gpu::plane_fit(p.data(), n);
    auto const peeled = pcp::gpu::extract_planes(p.data(), n, hypotheses, max_distance, 20u, 4u, options);

    std::string planes = "[", refits = "[";
    for (std::size_t r = 0; r < peeled.planes.size(); ++r) {
        planes += (r ? ", " : "") + list_bits(peeled.planes[r]);
        refits += (r ? ", " : "") + list_bits(peeled.refits[r]);
    }
    planes += "]", refits += "]";
    bool const agree = best.found && plain.refit == plain.plane && list_bits(plain.plane) == list_bits(best.plane) && !nobody.found &&
                       (list_bits(fit.plane) == list_bits(best.refit) || list_bits(pcp::gpu::plane_t{-fit.plane[0], -fit.plane[1], -fit.plane[2], -fit.plane[3]}) == list_bits(best.refit));
    std::printf("{\"p\": %s, \"hypotheses\": %llu, \"seed\": %u, \"max_distance\": %u, \"best\": %s, \"plain\": %s, \"two_rows\": %s, "
                "\"fit_inliers\": {\"plane\": %s, \"rms\": %llu}, \"fit_all\": {\"plane\": %s, \"rms\": %llu}, "
                "\"peeled\": {\"labels\": %s, \"planes\": %s, \"refits\": %s, \"scores\": %s}, \"calls_agree\": %s}\n",
                list_bits(p).c_str(), static_cast<unsigned long long>(hypotheses), options.seed, bits<std::uint32_t>(max_distance), result(best).c_str(),
                result(plain).c_str(), result(nobody).c_str(), list_bits(fit.plane).c_str(), static_cast<unsigned long long>(bits<std::uint64_t>(fit.rms)),
                list_bits(all.plane).c_str(), static_cast<unsigned long long>(bits<std::uint64_t>(all.rms)), list(peeled.labels).c_str(), planes.c_str(),
                refits.c_str(), list(peeled.scores).c_str(), agree ? "true" : "false");
    return agree ? 0 : 4;
}
