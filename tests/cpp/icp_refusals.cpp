// A stand-alone program that needs no device: every refusal of include/pcpx_icp.h, in host and _dev form.  The argument checks come
// before the handle is looked at, so every call here passes a NULL handle and bad arguments, must return PCPX_ERR_INVALID and must
// leave the error text of ITS refusal, not of the handle's.  tests/test_icp_cpu.py builds and runs it against the library; built
// together with the library's host code under -fsanitize=address,undefined it is the host-side sanitizer check of the argument paths.
// usage: icp_refusals        (exit status = the number of checks that failed)
#include <pcpx_icp.h>

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
    float const* normals;
    double* transform;
    std::uint32_t* partner;
};
int nearest(Args const& a, bool dev)
{
    return dev ? pcpx_nearest_posed_dev(nullptr, a.s, a.m, a.pose, a.radius, a.partner, nullptr)
               : pcpx_nearest_posed(nullptr, a.s, a.m, a.pose, a.radius, a.partner, nullptr);
}
int loop(Args const& a, bool dev)
{
    return dev ? pcpx_icp_rigid_dev(nullptr, a.s, a.m, a.pose, a.radius, a.max_iterations, a.flags, a.normals, a.transform, nullptr, nullptr, nullptr, nullptr,
                                    nullptr, a.partner)
               : pcpx_icp_rigid(nullptr, a.s, a.m, a.pose, a.radius, a.max_iterations, a.flags, a.normals, a.transform, nullptr, nullptr, nullptr, nullptr,
                                nullptr, a.partner);
}
} // namespace

int main()
{
    std::vector<float> cloud(3 * 8, 0.f);
    std::vector<std::uint32_t> partner(8, 9u);
    double xf[16];
    for (double& v : xf) v = 7.0;
    float const nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    std::uint64_t const big = 0xFFFFFFFFull;
    Args const good{cloud.data(), 8, nullptr, 0.5f, 10u, 0u, nullptr, xf, partner.data()};

    for (int dev = 0; dev < 2; ++dev) {
        auto refused = [&](auto change, char const* what, char const* text, bool is_loop) {
            Args a = good;
            change(a);
            int const st = is_loop ? loop(a, dev != 0) : nearest(a, dev != 0);
            expect(st == PCPX_ERR_INVALID && pcpx_last_error() && std::strstr(pcpx_last_error(), text) != nullptr, what);
        };
        for (int is_loop = 0; is_loop < 2; ++is_loop) {
            refused([](Args& a) { a.radius = -1e-30f; }, "negative radius", "radius", is_loop != 0);
            refused([](Args& a) { a.radius = -1.f; }, "radius -1", "radius", is_loop != 0);
            refused([&](Args& a) { a.radius = nan; }, "NaN radius", "radius", is_loop != 0);
            refused([&](Args& a) { a.radius = inf; }, "infinite radius", "radius", is_loop != 0);
            refused([&](Args& a) { a.radius = -inf; }, "radius -inf", "radius", is_loop != 0);
            refused([&](Args& a) { a.m = big; }, "m = 2^32 - 1", "source points", is_loop != 0);
            refused([&](Args& a) { a.m = big << 8; }, "m = 2^40", "source points", is_loop != 0);
            refused([](Args& a) { a.s = nullptr; }, "NULL source with m > 0", "source array", is_loop != 0);
        }
        refused([](Args& a) { a.partner = nullptr; }, "NULL partner", "partner", false);
        refused([](Args& a) { a.max_iterations = 0u; }, "no iterations", "max_iterations", true);
        refused([](Args& a) { a.max_iterations = PCPX_ICP_MAX_ITERATIONS + 1u; }, "1025 iterations", "max_iterations", true);
        refused([](Args& a) { a.max_iterations = 0xFFFFFFFFu; }, "2^32 - 1 iterations", "max_iterations", true);
        refused([](Args& a) { a.flags = 2u; }, "unknown flag", "flag", true);
        refused([](Args& a) { a.flags = 0x80000001u; }, "unknown high flag", "flag", true);
        refused([](Args& a) { a.flags = PCPX_ICP_POINT_TO_PLANE; }, "point to plane without normals", "without normals", true);
        refused([&](Args& a) { a.normals = cloud.data(); }, "normals without the flag", "normals without", true);
        refused([](Args& a) { a.transform = nullptr; }, "NULL transform", "transform", true);
        // good arguments reach the handle, which is NULL here
        expect(nearest(good, dev != 0) == PCPX_ERR_INVALID && std::strstr(pcpx_last_error(), "null handle") != nullptr, "NULL handle (nearest)");
        expect(loop(good, dev != 0) == PCPX_ERR_INVALID && std::strstr(pcpx_last_error(), "null handle") != nullptr, "NULL handle (loop)");
        Args empty = good;
        empty.s = nullptr, empty.m = 0;  // (an empty source is fine: it gets as far as the handle)
        expect(nearest(empty, dev != 0) == PCPX_ERR_INVALID && std::strstr(pcpx_last_error(), "null handle") != nullptr, "empty source (nearest)");
        expect(loop(empty, dev != 0) == PCPX_ERR_INVALID && std::strstr(pcpx_last_error(), "null handle") != nullptr, "empty source (loop)");
    }
    bool untouched = true;
    for (double v : xf) untouched = untouched && v == 7.0;
    for (std::uint32_t v : partner) untouched = untouched && v == 9u;
    expect(untouched, "a refused call wrote nothing");
    std::printf("%d checks failed\n", failures);
    return failures;
}
