// The flow of a shape-detection example -- a cloud with normals, its dominant ball, its dominant pipe, the least-squares fits -- with
// pcp::gpu::ransac_sphere, ransac_cylinder, sphere_fit and cylinder_fit (include/pcp/gpu/shapes.hpp) on a generated set: 300 points of
// a ball of radius 0.5 about (0.25, -0.5, 1), 300 points of a pipe of radius 0.25 along z through (-1, 1, .), and 100 points off
// both, each with its normal (those off the shapes: a fixed direction).
// tests/test_gpu_shapes.py compares what is printed with the model (tests/shapes_model.py) run on the printed set.
// usage: shapes_shape
// prints one JSON object (floats as their bits); exit status 0 when the calls agree with each other
#include <pcp/gpu/shapes.hpp>

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
std::string list_bits(pcp::gpu::shape_model_t const& v)
{
    std::vector<std::uint64_t> u;
    for (double f : v) u.push_back(bits<std::uint64_t>(f));
    return list(u);
}
template <class R>
std::string result(R const& r, pcp::gpu::shape_model_t const& refit)
{
    return std::string("{\"found\": ") + (r.found ? "1" : "0") + ", \"hypothesis\": " + std::to_string(r.hypothesis) + ", \"inliers\": " + list(r.inliers) +
           ", \"model\": " + list_bits(r.model) + ", \"refit\": " + list_bits(refit) + "}";
}
// a fixed sequence in [0, 1)
double next(std::uint32_t& s)
{
    s = s * 1664525u + 1013904223u;
    return (s >> 8) / 16777216.0;
}
} // namespace

int main()
{
    std::vector<float> p, nrm;
    std::uint32_t s          = 12345u;
    double const two_pi      = 6.283185307179586;
    auto const push = [&](double x, double y, double z, double a, double b, double c) {
        p.insert(p.end(), {static_cast<float>(x), static_cast<float>(y), static_cast<float>(z)});
        nrm.insert(nrm.end(), {static_cast<float>(a), static_cast<float>(b), static_cast<float>(c)});
    };
    for (int i = 0; i < 300; ++i) {  // the ball
        double const z = 2.0 * next(s) - 1.0, phi = two_pi * next(s), r = std::sqrt(1.0 - z * z), sign = i % 3 ? 1.0 : -1.0;
        double const d[3] = {r * std::cos(phi), r * std::sin(phi), z};
        push(0.25 + 0.5 * d[0], -0.5 + 0.5 * d[1], 1.0 + 0.5 * d[2], sign * d[0], sign * d[1], sign * d[2]);
    }
    for (int i = 0; i < 300; ++i) {  // the pipe
        double const phi = two_pi * next(s), z = 2.0 * next(s) - 1.0, sign = i % 2 ? 1.0 : -1.0;
        push(-1.0 + 0.25 * std::cos(phi), 1.0 + 0.25 * std::sin(phi), z, sign * std::cos(phi), sign * std::sin(phi), 0.0);
    }
    for (int i = 0; i < 100; ++i) push(4.0 * next(s) - 2.0, 4.0 * next(s) - 2.0, 4.0 * next(s) - 2.0, 0.6, 0.0, 0.8);
    std::size_t const n = p.size() / 3;

    std::uint64_t const hypotheses = 512;
    float const max_distance       = 0.01f;
    pcp::gpu::shape_options_t options;
    options.seed = 7;
    auto const ball = pcp::gpu::ransac_sphere(p.data(), nrm.data(), n, hypotheses, max_distance, options);
    auto const pipe = pcp::gpu::ransac_cylinder(p.data(), nrm.data(), n, hypotheses, max_distance, options);
    pcp::gpu::shape_options_t plain_options = options;
    plain_options.refit                     = false;
    auto const plain = pcp::gpu::ransac_sphere(p.data(), nrm.data(), n, hypotheses, max_distance, plain_options);
    std::vector<std::uint32_t> const one{5u};
    auto const nobody   = pcp::gpu::ransac_sphere(p.data(), nrm.data(), n, hypotheses, max_distance, options, one.data(), one.size());
    auto const ball_fit = pcp::gpu::sphere_fit(p.data(), n, ball.inliers.data(), ball.inliers.size());
    auto const pipe_fit = pcp::gpu::cylinder_fit(p.data(), nrm.data(), n, pipe.inliers.data(), pipe.inliers.size());

    pcp::gpu::shape_model_t const ball_refit{ball.center[0], ball.center[1], ball.center[2], ball.radius, 0., 0., 0., 0.};
    pcp::gpu::shape_model_t const pipe_refit{pipe.point[0], pipe.point[1], pipe.point[2], pipe.axis[0], pipe.axis[1], pipe.axis[2], pipe.radius, 0.};
    pcp::gpu::shape_model_t const plain_best{plain.center[0], plain.center[1], plain.center[2], plain.radius, 0., 0., 0., 0.};
    bool const agree = ball.found && pipe.found && !nobody.found && ball_fit.ok && pipe_fit.ok && list_bits(plain.model) == list_bits(ball.model) &&
                       list_bits(plain_best) == list_bits(plain.model) && list_bits(ball_fit.model) == list_bits(ball_refit) &&
                       list_bits(pipe_fit.model) == list_bits(pipe_refit);
    std::printf("{\"p\": %s, \"n\": %s, \"hypotheses\": %llu, \"seed\": %u, \"max_distance\": %u, \"ball\": %s, \"pipe\": %s, \"plain\": %s, "
                "\"one_row\": %s, \"ball_fit\": {\"model\": %s, \"rms\": %llu}, \"pipe_fit\": {\"model\": %s, \"rms\": %llu}, \"calls_agree\": %s}\n",
                list_bits(p).c_str(), list_bits(nrm).c_str(), static_cast<unsigned long long>(hypotheses), options.seed, bits<std::uint32_t>(max_distance),
                result(ball, ball_refit).c_str(), result(pipe, pipe_refit).c_str(), result(plain, plain_best).c_str(), result(nobody, pcp::gpu::shape_model_t{}).c_str(),
                list_bits(ball_fit.model).c_str(), static_cast<unsigned long long>(bits<std::uint64_t>(ball_fit.rms)), list_bits(pipe_fit.model).c_str(),
                static_cast<unsigned long long>(bits<std::uint64_t>(pipe_fit.rms)), agree ? "true" : "false");
    return agree ? 0 : 4;
}
