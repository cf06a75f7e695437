// A stand-alone program that needs no device: pcpx_plane_plan and every refusal of include/pcpx_planes.h, in host and _dev form.
// Every refused call must return PCPX_ERR_INVALID and leave an error text.  tests/test_planes_cpu.py builds and runs it against the
// library; built together with the library's host code under -fsanitize=address,undefined it is the host-side sanitizer check of
// the argument paths.
// usage: planes_refusals        (exit status = the number of checks that failed)
#include <pcpx_planes.h>

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
    float const* points;
    std::uint64_t n;
    float const* normals;
    std::uint32_t const* rows;
    std::uint64_t capacity;
    pcpx_plane_params params;
    bool null_params;
    std::uint32_t* found;
    double* plane;
    double* refit;
    std::uint32_t* labels;
    std::uint32_t* count;
};
enum Call { RANSAC, FIT, EXTRACT };
int call(Args const& a, Call which, bool dev)
{
    pcpx_plane_params const* prm = a.null_params ? nullptr : &a.params;
    switch (which) {
    case RANSAC:
        if (dev)
            return pcpx_plane_ransac_dev(a.points, a.n, a.normals, a.rows, a.capacity, nullptr, prm, 0, nullptr, a.found, nullptr, nullptr, nullptr, nullptr,
                                         a.plane, a.refit);
        return pcpx_plane_ransac(a.points, a.n, a.normals, a.rows, a.capacity, prm, 0, a.found, nullptr, nullptr, nullptr, a.plane, a.refit);
    case FIT:
        if (dev) return pcpx_plane_fit_dev(a.points, a.n, a.rows, a.capacity, nullptr, 0, nullptr, a.plane, nullptr);
        return pcpx_plane_fit(a.points, a.n, a.rows, a.capacity, 0, a.plane, nullptr);
    default:
        if (dev) return pcpx_extract_planes_dev(a.points, a.n, a.normals, prm, 0, nullptr, a.labels, a.count, a.plane, a.refit, nullptr);
        return pcpx_extract_planes(a.points, a.n, a.normals, prm, 0, a.labels, a.count, a.plane, a.refit, nullptr);
    }
}
} // namespace

int main()
{
    std::vector<float> cloud(3 * 8, 0.f);
    std::vector<std::uint32_t> rows(8, 0u), labels(8, 9u);
    std::uint32_t found = 9, count = 9;
    double plane[4 * 64], refit[4 * 64];
    float const nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    std::uint64_t const big = 0xFFFFFFFFull;
    pcpx_plane_params prm{};
    prm.hypotheses   = 64;
    prm.max_distance = 0.01f;
    prm.origin_row   = PCPX_PLANE_ORIGIN_FIRST;
    prm.max_planes   = 3;
    Args const good{cloud.data(), 8, cloud.data(), rows.data(), 8, prm, false, &found, plane, refit, labels.data(), &count};

    for (int dev = 0; dev < 2; ++dev) {
        auto refused = [&](auto change, char const* what, Call which) {
            Args a = good;
            if (which == EXTRACT) a.rows = nullptr, a.capacity = 0;
            change(a);
            int const st = call(a, which, dev != 0);
            expect(st == PCPX_ERR_INVALID && pcpx_last_error() && std::strlen(pcpx_last_error()) > 0, what);
        };
        for (Call which : {RANSAC, EXTRACT}) {
            refused([](Args& a) { a.points = nullptr; }, "NULL points", which);
            refused([&](Args& a) { a.n = big; }, "too many points", which);
            refused([](Args& a) { a.null_params = true; }, "NULL params", which);
            refused([](Args& a) { a.params.hypotheses = 0; }, "no hypotheses", which);
            refused([&](Args& a) { a.params.hypotheses = big; }, "too many hypotheses", which);
            refused([](Args& a) { a.params.max_distance = -1e-30f; }, "negative max_distance", which);
            refused([&](Args& a) { a.params.max_distance = nan; }, "NaN max_distance", which);
            refused([](Args& a) { a.params.flags = 8u; }, "unknown flag", which);
            refused([](Args& a) { a.params.flags = 0x80000001u; }, "unknown high flag", which);
            refused([](Args& a) { a.params.flags = PCPX_PLANE_REFIT, a.refit = nullptr; }, "refit without an array", which);
            refused([](Args& a) { a.params.flags = PCPX_PLANE_NORMALS, a.normals = nullptr; }, "a normal gate without normals", which);
            refused([](Args& a) { a.params.flags = PCPX_PLANE_NORMALS, a.params.min_normal_cos = -0.1f; }, "negative min_normal_cos", which);
            refused([](Args& a) { a.params.flags = PCPX_PLANE_NORMALS, a.params.min_normal_cos = 1.0000001f; }, "min_normal_cos above 1", which);
            refused([&](Args& a) { a.params.flags = PCPX_PLANE_NORMALS, a.params.min_normal_cos = nan; }, "NaN min_normal_cos", which);
            refused([](Args& a) { a.params.flags = PCPX_PLANE_AXIS; }, "a zero axis", which);
            refused([&](Args& a) { a.params.flags = PCPX_PLANE_AXIS, a.params.axis[1] = inf; }, "an infinite axis", which);
            refused([&](Args& a) { a.params.flags = PCPX_PLANE_AXIS, a.params.axis[2] = nan; }, "a NaN axis", which);
            refused([](Args& a) { a.params.flags = PCPX_PLANE_AXIS, a.params.axis[0] = 1.f, a.params.min_axis_cos = 1.5f; }, "min_axis_cos above 1", which);
            refused([&](Args& a) { a.params.flags = PCPX_PLANE_AXIS, a.params.axis[0] = 1.f, a.params.min_axis_cos = nan; }, "NaN min_axis_cos", which);
        }
        refused([](Args& a) { a.rows = nullptr; }, "NULL rows with a size", RANSAC);
        refused([&](Args& a) { a.capacity = big; }, "too large a capacity", RANSAC);
        refused([](Args& a) { a.found = nullptr; }, "NULL found", RANSAC);
        refused([](Args& a) { a.params.max_planes = 0; }, "no planes", EXTRACT);
        refused([](Args& a) { a.params.max_planes = PCPX_PLANES_MAX + 1; }, "too many planes", EXTRACT);
        refused([](Args& a) { a.labels = nullptr; }, "NULL labels", EXTRACT);
        refused([](Args& a) { a.count = nullptr; }, "NULL count", EXTRACT);
        refused([](Args& a) { a.points = nullptr; }, "fit: NULL points", FIT);
        refused([&](Args& a) { a.n = big; }, "fit: too many points", FIT);
        refused([](Args& a) { a.rows = nullptr; }, "fit: NULL rows with a size", FIT);
        refused([&](Args& a) { a.capacity = big; }, "fit: too large a capacity", FIT);
        refused([](Args& a) { a.plane = nullptr; }, "fit: NULL plane", FIT);
    }
    expect(found == 9 && count == 9 && labels[0] == 9, "a refused call wrote nothing");

    // the plan: every output optional, the sizes refused as by the calls, the cut covers the capacity
    expect(pcpx_plane_plan(64, 1000, 0, 0, nullptr, nullptr, nullptr) == PCPX_OK, "plan without outputs");
    expect(pcpx_plane_plan(0, 1000, 0, 0, nullptr, nullptr, nullptr) == PCPX_ERR_INVALID, "plan: no hypotheses");
    expect(pcpx_plane_plan(big, 1000, 0, 0, nullptr, nullptr, nullptr) == PCPX_ERR_INVALID, "plan: too many hypotheses");
    expect(pcpx_plane_plan(64, big, 0, 0, nullptr, nullptr, nullptr) == PCPX_ERR_INVALID, "plan: too large a capacity");
    expect(pcpx_plane_plan(64, 1000, 8u, 0, nullptr, nullptr, nullptr) == PCPX_ERR_INVALID, "plan: unknown flag");
    expect(pcpx_plane_plan(64, 1000, 0, PCPX_PLANES_MAX + 1, nullptr, nullptr, nullptr) == PCPX_ERR_INVALID, "plan: too many planes");
    std::uint64_t const sizes[][2] = {{1, 0}, {1, 1}, {64, 255}, {64, 256}, {65, 513}, {4096, 1535}, {1000000, 10000}, {big - 1, big - 1}, {1, big - 1}};
    for (auto const& s : sizes) {
        for (std::uint32_t flags : {0u, PCPX_PLANE_NORMALS}) {
            std::uint32_t segments = 7;
            std::uint64_t rows_per = 7, bytes = 7, peel_bytes = 7;
            expect(pcpx_plane_plan(s[0], s[1], flags, 0, &segments, &rows_per, &bytes) == PCPX_OK, "plan");
            expect(pcpx_plane_plan(s[0], s[1], flags, 6, nullptr, nullptr, &peel_bytes) == PCPX_OK, "plan of a peel");
            if (s[1] == 0) expect(segments == 0 && rows_per == 0, "plan of no rows");
            else expect(segments >= 1 && segments <= 256 && rows_per % 256 == 0 && (segments - 1) * rows_per < s[1] && s[1] <= segments * rows_per, "the cut covers the capacity");
            std::uint64_t const rec = flags ? 32 : 16;
            expect(bytes % 256 == 0 && bytes >= rec * s[1] && peel_bytes >= bytes + rec * s[1], "the scratch holds the records, a peel's both buffers");
        }
    }
    std::printf("%d checks failed\n", failures);
    return failures;
}
