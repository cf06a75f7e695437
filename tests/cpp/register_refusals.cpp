// A stand-alone program that needs no device: pcpx_ransac_plan and every refusal of include/pcpx_register.h, in host and _dev form.
// Every refused call must return PCPX_ERR_INVALID and leave an error text.  tests/test_register_cpu.py builds and runs it against the
// library; built together with the library's host code under -fsanitize=address,undefined it is the host-side sanitizer check of
// the argument paths.
// usage: register_refusals        (exit status = the number of checks that failed)
#include <pcpx_register.h>

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
    float const* p;
    std::uint64_t np;
    float const* q;
    std::uint64_t nq;
    std::uint32_t const* pairs;
    std::uint64_t capacity, hypotheses;
    float tau2, s2;
    std::uint32_t flags;
    std::uint32_t* found;
    double* refit;
    std::uint32_t const* positions;
    std::uint64_t positions_capacity;
    double* transform;
};
int ransac(Args const& a, bool dev)
{
    if (dev)
        return pcpx_ransac_rigid_dev(a.p, a.np, a.q, a.nq, a.pairs, a.capacity, nullptr, a.hypotheses, 1u, a.tau2, a.s2, a.flags, 0, nullptr, a.found, nullptr,
                                     nullptr, nullptr, nullptr, nullptr, a.refit);
    return pcpx_ransac_rigid(a.p, a.np, a.q, a.nq, a.pairs, a.capacity, a.hypotheses, 1u, a.tau2, a.s2, a.flags, 0, a.found, nullptr, nullptr, nullptr,
                             nullptr, a.refit);
}
int fit(Args const& a, bool dev)
{
    if (dev)
        return pcpx_rigid_fit_dev(a.p, a.np, a.q, a.nq, a.pairs, a.capacity, nullptr, a.positions, a.positions_capacity, nullptr, 0, nullptr, a.transform,
                                  nullptr);
    return pcpx_rigid_fit(a.p, a.np, a.q, a.nq, a.pairs, a.capacity, a.positions, a.positions_capacity, 0, a.transform, nullptr);
}
} // namespace

int main()
{
    std::vector<float> cloud(3 * 8, 0.f);
    std::vector<std::uint32_t> pairs(2 * 8, 0u), positions(8, 0u);
    std::uint32_t found = 9;
    double xf[16];
    float const nan = std::numeric_limits<float>::quiet_NaN();
    std::uint64_t const big = 0xFFFFFFFFull;
    Args const good{cloud.data(), 8, cloud.data(), 8, pairs.data(), 8, 64, 0.01f, 0.81f, 0u, &found, nullptr, positions.data(), 8, xf};

    for (int dev = 0; dev < 2; ++dev) {
        auto refused = [&](auto change, char const* what, bool is_fit = false) {
            Args a = good;
            change(a);
            int const st = is_fit ? fit(a, dev != 0) : ransac(a, dev != 0);
            expect(st == PCPX_ERR_INVALID && pcpx_last_error() && std::strlen(pcpx_last_error()) > 0, what);
        };
        refused([](Args& a) { a.p = nullptr; }, "NULL p");
        refused([](Args& a) { a.q = nullptr; }, "NULL q");
        refused([](Args& a) { a.pairs = nullptr; }, "NULL pairs");
        refused([](Args& a) { a.hypotheses = 0; }, "no hypotheses");
        refused([&](Args& a) { a.hypotheses = big; }, "too many hypotheses");
        refused([&](Args& a) { a.capacity = big; }, "too large a capacity");
        refused([&](Args& a) { a.np = big + 1; }, "too many points");
        refused([](Args& a) { a.tau2 = -1e-30f; }, "negative max_distance_sq");
        refused([&](Args& a) { a.tau2 = nan; }, "NaN max_distance_sq");
        refused([](Args& a) { a.s2 = -0.1f; }, "negative edge_similarity_sq");
        refused([](Args& a) { a.s2 = 1.0000001f; }, "edge_similarity_sq above 1");
        refused([&](Args& a) { a.s2 = nan; }, "NaN edge_similarity_sq");
        refused([](Args& a) { a.flags = 2u; }, "unknown flag");
        refused([](Args& a) { a.flags = 0x80000001u; }, "unknown high flag");
        refused([](Args& a) { a.flags = PCPX_RANSAC_REFIT; }, "refit without an array");
        refused([](Args& a) { a.found = nullptr; }, "NULL found");
        refused([](Args& a) { a.p = nullptr; }, "fit: NULL p", true);
        refused([](Args& a) { a.q = nullptr; }, "fit: NULL q", true);
        refused([](Args& a) { a.pairs = nullptr; }, "fit: NULL pairs", true);
        refused([&](Args& a) { a.capacity = big; }, "fit: too large a capacity", true);
        refused([&](Args& a) { a.positions_capacity = big; }, "fit: too many positions", true);
        refused([](Args& a) { a.positions = nullptr; }, "fit: NULL positions with a size", true);
        refused([](Args& a) { a.transform = nullptr; }, "fit: NULL transform", true);
    }
    expect(found == 9, "a refused call wrote nothing");

    // the plan: every output optional, the sizes refused as by the calls, the cut covers the capacity
    expect(pcpx_ransac_plan(64, 1000, nullptr, nullptr, nullptr) == PCPX_OK, "plan without outputs");
    expect(pcpx_ransac_plan(0, 1000, nullptr, nullptr, nullptr) == PCPX_ERR_INVALID, "plan: no hypotheses");
    expect(pcpx_ransac_plan(big, 1000, nullptr, nullptr, nullptr) == PCPX_ERR_INVALID, "plan: too many hypotheses");
    expect(pcpx_ransac_plan(64, big, nullptr, nullptr, nullptr) == PCPX_ERR_INVALID, "plan: too large a capacity");
    std::uint64_t const sizes[][2] = {{1, 0}, {1, 1}, {64, 255}, {64, 256}, {65, 513}, {4096, 1535}, {1000000, 10000}, {big - 1, big - 1}, {1, big - 1}};
    for (auto const& s : sizes) {
        std::uint32_t segments = 7;
        std::uint64_t rows = 7, bytes = 7;
        expect(pcpx_ransac_plan(s[0], s[1], &segments, &rows, &bytes) == PCPX_OK, "plan");
        if (s[1] == 0) expect(segments == 0 && rows == 0, "plan of no pairs");
        else expect(segments >= 1 && segments <= 256 && rows % 256 == 0 && (segments - 1) * rows < s[1] && s[1] <= segments * rows, "the cut covers the capacity");
        expect(bytes % 256 == 0 && bytes >= 32 * s[1], "the scratch holds the records");
    }
    std::printf("%d checks failed\n", failures);
    return failures;
}
