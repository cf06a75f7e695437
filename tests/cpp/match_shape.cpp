// The flow of a matching example -- two sets of descriptors, the nearest rows, the correspondences -- with pcp::gpu::match_nearest and
// pcp::gpu::match_correspondences (include/pcp/gpu/matching.hpp) on a hand-made set with ties, a duplicate and a zero row on either
// side, through the std::array overloads and the flat ones.  tests/test_gpu_match.py compares what is printed with the model
// (tests/match_model.py) run on the printed sets.
// usage: match_shape
// prints one JSON object (d2 as the bits of the float32); exit status 0 when the two overloads agree
#include <pcp/gpu/matching.hpp>

#include <array>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace {
constexpr std::size_t D = 5;
using row_t             = std::array<float, D>;

std::uint32_t bits(float v)
{
    std::uint32_t u;
    std::memcpy(&u, &v, sizeof(u));
    return u;
}
std::string list(std::vector<std::uint32_t> const& v)
{
    std::string s = "[";
    for (std::size_t i = 0; i < v.size(); ++i) s += (i ? ", " : "") + std::to_string(v[i]);
    return s + "]";
}
std::string list_bits(std::vector<float> const& v)
{
    std::vector<std::uint32_t> u;
    for (float f : v) u.push_back(bits(f));
    return list(u);
}
std::string rows(std::vector<row_t> const& v)
{
    std::string s = "[";
    for (std::size_t i = 0; i < v.size(); ++i) s += (i ? ", " : "") + list_bits(std::vector<float>(v[i].begin(), v[i].end()));
    return s + "]";
}
std::string nearest(pcp::gpu::nearest_matches_t const& r)
{
    return "{\"index\": " + list(r.index) + ", \"d2\": " + list_bits(r.d2) + ", \"second_index\": " + list(r.second_index) +
           ", \"second_d2\": " + list_bits(r.second_d2) + "}";
}
std::string pairs(std::vector<pcp::gpu::correspondence_t> const& c)
{
    std::string s = "[";
    for (std::size_t k = 0; k < c.size(); ++k)
        s += (k ? ", " : "") + list({c[k].source, c[k].target, bits(c[k].d2)});
    return s + "]";
}
bool same(pcp::gpu::nearest_matches_t const& a, pcp::gpu::nearest_matches_t const& b)
{
    return a.index == b.index && a.second_index == b.second_index && list_bits(a.d2) == list_bits(b.d2) &&
           list_bits(a.second_d2) == list_bits(b.second_d2);
}
} // namespace

int main()
{
    std::vector<row_t> const src{{0, 0, 0, 0, 0}, {1, 0, 0, 0, 0}, {0, 2, 0, 0, 0}, {3, 3, 0, 0, 0}, {1, 0, 0, 0, 0}, {10, 10, 10, 10, 10}};
    std::vector<row_t> const tgt{{1, 0, 0, 0, 1}, {1, 0, 0, 1, 0}, {0, 2, 0, 0, 0}, {0, 0, 0, 0, 0}, {3, 3, 0, 0, 0.5f}, {9, 10, 10, 10, 10}, {-0.f, 0, 0, -0.f, 0}};

    auto const plain   = pcp::gpu::match_nearest(src, tgt);
    auto const skipped = pcp::gpu::match_nearest(src, tgt, true);
    auto const flat    = pcp::gpu::match_nearest(src.front().data(), src.size(), tgt.front().data(), tgt.size(), D, true);
    auto const mutual  = pcp::gpu::match_correspondences(src, tgt, 1.f, true, true);
    auto const ratio   = pcp::gpu::match_correspondences(src, tgt, 0.75f, false, false);
    auto const flat_c  = pcp::gpu::match_correspondences(src.front().data(), src.size(), tgt.front().data(), tgt.size(), D, 0.75f, false, false);
    auto const nobody  = pcp::gpu::match_nearest(src, std::vector<row_t>{});

    bool const agree = same(skipped, flat) && pairs(ratio) == pairs(flat_c);
    std::printf("{\"dims\": %zu, \"src\": %s, \"tgt\": %s, \"nearest\": %s, \"nearest_skip_zero_rows\": %s, \"nearest_no_targets\": %s, "
                "\"mutual_skip_zero_rows\": %s, \"ratio_075\": %s, \"overloads_agree\": %s}\n",
                D, rows(src).c_str(), rows(tgt).c_str(), nearest(plain).c_str(), nearest(skipped).c_str(), nearest(nobody).c_str(),
                pairs(mutual).c_str(), pairs(ratio).c_str(), agree ? "true" : "false");
    return agree ? 0 : 4;
}
