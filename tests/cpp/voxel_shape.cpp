// The flow of a downsampling example -- a cloud with colours, one point per cell -- with pcp::gpu::voxel_grid_downsample
// (include/pcp/gpu/voxel_grid.hpp) on a hand-made set: a 9 x 7 x 5 lattice of eighths with a second, shifted copy of a part of it, a
// point outside the grid's origin and one that is not finite.
// tests/test_gpu_voxel.py compares what is printed with the Python call and the model (tests/voxel_model.py) on the printed set.
// usage: voxel_shape
// prints one JSON object (floats as their bits); exit status 0 when the calls agree with each other
#include <pcp/gpu/voxel_grid.hpp>

#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

namespace {
std::uint32_t bits(float v)
{
    std::uint32_t u;
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
    for (float f : v) u.push_back(bits(f));
    return list(u);
}
std::string result(pcp::gpu::voxel_grid_result_t const& r)
{
    return "{\"points\": " + list_bits(r.points) + ", \"attrs\": " + list_bits(r.attributes) + ", \"counts\": " + list(r.counts) + ", \"keys\": " + list(r.keys) +
           ", \"rows\": " + list(r.rows) + ", \"owner\": " + list(r.owner) + ", \"dropped\": " + std::to_string(r.dropped) +
           ", \"origin\": " + list_bits(std::vector<float>(r.origin.begin(), r.origin.end())) + "}";
}
} // namespace

int main()
{
    std::vector<float> p, colour;
    for (int i = 0; i < 9; ++i)
        for (int j = 0; j < 7; ++j)
            for (int k = 0; k < 5; ++k) {
                p.insert(p.end(), {static_cast<float>(i) / 8.f, static_cast<float>(j) / 8.f, static_cast<float>(k) / 8.f});
                if ((i + j + k) % 3 == 0) p.insert(p.end(), {static_cast<float>(i) / 8.f + 0.0625f, static_cast<float>(j) / 8.f, static_cast<float>(k) / 8.f + 0.03125f});
            }
    p.insert(p.end(), {-1.f, 0.25f, 0.25f});
    p.insert(p.end(), {0.25f, std::numeric_limits<float>::quiet_NaN(), 0.25f});
    std::size_t const n = p.size() / 3;
    for (std::size_t r = 0; r < n; ++r) colour.insert(colour.end(), {static_cast<float>(r % 7) / 4.f, static_cast<float>(r % 5), static_cast<float>(r) / 16.f});

    std::array<float, 3> const leaf{0.25f, 0.5f, 0.25f};
    float const origin[3] = {0.f, 0.f, 0.f};
    pcp::gpu::voxel_grid_options_t coloured;
    coloured.origin            = origin;
    coloured.attributes        = colour.data();
    coloured.attribute_columns = 3;
    auto const fixed = pcp::gpu::voxel_grid_downsample(p.data(), n, leaf, coloured);
    auto const plain = pcp::gpu::voxel_grid_downsample(p.data(), n, leaf);
    pcp::gpu::voxel_grid_options_t bare = coloured;
    bare.attributes                     = nullptr;
    auto const uncoloured = pcp::gpu::voxel_grid_downsample(p.data(), n, leaf, bare);
    auto const nothing    = pcp::gpu::voxel_grid_downsample(p.data(), 0, leaf);

    std::uint64_t members = 0;
    for (std::uint32_t c : fixed.counts) members += c;
    bool const agree = fixed.size() > 0 && members + fixed.dropped == n && fixed.dropped == 2 && plain.dropped == 1 && plain.origin[0] == -1.f &&
                       uncoloured.attributes.empty() && list_bits(uncoloured.points) == list_bits(fixed.points) && uncoloured.keys == fixed.keys &&
                       uncoloured.rows == fixed.rows && uncoloured.owner == fixed.owner && nothing.size() == 0 && nothing.owner.empty();
    std::printf("{\"p\": %s, \"colour\": %s, \"leaf\": %s, \"fixed\": %s, \"plain\": %s, \"calls_agree\": %s}\n", list_bits(p).c_str(),
                list_bits(colour).c_str(), list_bits(std::vector<float>(leaf.begin(), leaf.end())).c_str(), result(fixed).c_str(), result(plain).c_str(),
                agree ? "true" : "false");
    return agree ? 0 : 4;
}
