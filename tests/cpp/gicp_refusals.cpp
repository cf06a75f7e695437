// A stand-alone program that needs no device: every refusal of include/pcpx_gicp.h, with host arrays and with PCPX_GICP_ON_DEVICE.  The argument checks come
// before the handle is looked at, so every call here passes a NULL handle and bad arguments, must return PCPX_ERR_INVALID and must
// leave the error text of ITS refusal, not of the handle's.  tests/test_gicp_cpu.py builds and runs it against the library; built
// together with the library's host code under -fsanitize=address,undefined it is the host-side sanitizer check of the argument paths.
// usage: gicp_refusals        (exit status = the number of checks that failed)
#include <pcpx_gicp.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

namespace {
int failures = 0;
void expect(bool ok, char const* what)
{
    if (ok) return;
    ++failures;
    std::printf("FAILED: %s (last error: %s)\n", what, pcpx_last_error() ? pcpx_last_error() : "none");
}
struct Args {
    float const* s;
    std::uint64_t m;
    double const* pose;
    float radius;
    std::uint32_t max_iterations, flags;
    float const *source_cov, *target_cov;
    float epsilon;
    double* transform;
    std::uint32_t* partner;
};
int loop(Args const& a, bool dev)
{
    return pcpx_gicp_rigid(nullptr, a.s, a.m, a.pose, a.radius, a.max_iterations, a.flags | (dev ? PCPX_GICP_ON_DEVICE : 0u), a.source_cov, a.target_cov,
                           a.epsilon, a.transform, nullptr, nullptr, nullptr, nullptr, nullptr, a.partner);
}
} // namespace

int main()
{
    std::vector<float> cloud(6 * 8, 0.f);
    std::vector<std::uint32_t> partner(8, 9u);
    double xf[16];
    for (double& v : xf) v = 7.0;
    float const nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    std::uint64_t const big = 0xFFFFFFFFull;
    Args const good{cloud.data(), 8, nullptr, 0.5f, 10u, 0u, cloud.data(), cloud.data(), 1e-3f, xf, partner.data()};
    Args good_cov = good;
    good_cov.flags = PCPX_GICP_COVARIANCES, good_cov.epsilon = 0.f;

    for (int dev = 0; dev < 2; ++dev) {
        auto refused = [&](Args const& from, auto change, char const* what, char const* text) {
            Args a = from;
            change(a);
            int const st = loop(a, dev != 0);
            expect(st == PCPX_ERR_INVALID && pcpx_last_error() && std::strstr(pcpx_last_error(), text) != nullptr, what);
        };
        for (Args const* from : std::vector<Args const*>{&good, &good_cov}) {
            refused(*from, [](Args& a) { a.radius = -1e-30f; }, "negative radius", "radius");
            refused(*from, [](Args& a) { a.radius = -1.f; }, "radius -1", "radius");
            refused(*from, [&](Args& a) { a.radius = nan; }, "NaN radius", "radius");
            refused(*from, [&](Args& a) { a.radius = inf; }, "infinite radius", "radius");
            refused(*from, [&](Args& a) { a.radius = -inf; }, "radius -inf", "radius");
            refused(*from, [&](Args& a) { a.m = big; }, "m = 2^32 - 1", "source points");
            refused(*from, [&](Args& a) { a.m = big << 8; }, "m = 2^40", "source points");
            refused(*from, [](Args& a) { a.s = nullptr; }, "NULL source with m > 0", "source array");
            refused(*from, [](Args& a) { a.max_iterations = 0u; }, "no iterations", "max_iterations");
            refused(*from, [](Args& a) { a.max_iterations = PCPX_ICP_MAX_ITERATIONS + 1u; }, "1025 iterations", "max_iterations");
            refused(*from, [](Args& a) { a.max_iterations = 0xFFFFFFFFu; }, "2^32 - 1 iterations", "max_iterations");
            refused(*from, [](Args& a) { a.transform = nullptr; }, "NULL transform", "transform");
            refused(*from, [](Args& a) { a.flags |= 4u; }, "unknown flag", "flag");
            refused(*from, [](Args& a) { a.flags |= 0x80000000u; }, "unknown high flag", "flag");
            refused(*from, [](Args& a) { a.source_cov = nullptr; }, "NULL source covariances with m > 0", "source covariance");
            refused(*from, [](Args& a) { a.target_cov = nullptr; }, "NULL target covariances", "target covariance");
            refused(*from, [](Args& a) { a.target_cov = nullptr, a.s = nullptr, a.source_cov = nullptr, a.m = 0; }, "NULL target covariances, empty source",
                    "target covariance");
            refused(*from, [&](Args& a) { a.epsilon = nan; }, "NaN epsilon", "epsilon");
            refused(*from, [&](Args& a) { a.epsilon = inf; }, "infinite epsilon", "epsilon");
            refused(*from, [](Args& a) { a.epsilon = -1e-3f; }, "negative epsilon", "epsilon");
            refused(*from, [](Args& a) { a.epsilon = 1.5f; }, "epsilon above 1", "epsilon");
        }
        refused(good, [](Args& a) { a.epsilon = 0.f; }, "epsilon 0 with normals", "epsilon must be in");
        refused(good_cov, [](Args& a) { a.epsilon = 1e-3f; }, "an epsilon with covariances", "epsilon must be 0");
        refused(good_cov, [](Args& a) { a.epsilon = 1.f; }, "epsilon 1 with covariances", "epsilon must be 0");
        // good arguments reach the handle, which is NULL here; epsilon = 1 is inside
        Args one = good;
        one.epsilon = 1.f;
        Args empty = good;
        empty.s = nullptr, empty.source_cov = nullptr, empty.m = 0;  // (an empty source is fine: it gets as far as the handle)
        for (Args const* a : std::vector<Args const*>{&good, &good_cov, &one, &empty})
            expect(loop(*a, dev != 0) == PCPX_ERR_INVALID && std::strstr(pcpx_last_error(), "null handle") != nullptr, "NULL handle");
    }
    bool untouched = true;
    for (double v : xf) untouched = untouched && v == 7.0;
    for (std::uint32_t v : partner) untouched = untouched && v == 9u;
    expect(untouched, "a refused call wrote nothing");
    std::printf("%d checks failed\n", failures);
    return failures;
}
