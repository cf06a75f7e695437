// pcpx_path_start.h -- which node each lane stands for in k_knn's path start (WalkerT::start_path, pcpx_device.h), and which of those
// nodes are the group's own.  Host and device, plain integer arithmetic: included by pcpx_device.h under hipcc and, alone, by a
// plain C++ program (tests/cpp/path_start.cpp), which drives the start state through a restatement of the walker's pops.
//
// Group g of a self query holds the points of leaves [8 g, 8 g + 8): the last-level (height 1) nodes 2 g and 2 g + 1, and at height
// h >= 2 the node g >> (2 h - 3).  Every round of the root start (WalkerT::start) expands the root and each of these ancestors down
// to height 2 -- depth - 1 expansions whose outcome is known: every lane's own point lies inside.  The path start tests, in ONE step
// of the wave, all children of all these ancestors:
//
//     lane 4 h + c, 1 <= h <= depth - 1  =  child c, a node of height h, of the group's ancestor of height h + 1
//     its level-local index             =  ((g >> (2 h - 1)) << 2) + c,    its heap id  =  level_base(depth - h) + that
//
// (lanes below 4 and from 4 depth on stand for nothing).  These are the aligned groups of four siblings the root start loads, so a
// padding sibling is an initialised record.  Bit 4 h + c is also where WalkerT's pending bits keep that child while the walk is
// inside the height-2 ancestor: the ballot of the passing lanes IS the start state, with ploc = g >> 1 and l = 1.  Cleared in it are
// the path's own child at every height >= 2 (the walk is already inside it) and, at height 1, the group's own two last-level nodes
// (all their leaves lie in a self group's seed range: the walk would skip every one).
#ifndef PCPX_PATH_START_H
#define PCPX_PATH_START_H

#include <cstdint>

#if defined(__HIPCC__)
#define PCPX_PATH_START_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define PCPX_PATH_START_FN inline
#endif

namespace pcpx {

struct PathLane {
    bool on;            // the lane stands for a node that is to be tested
    std::uint32_t node;  // heap id of that node (0, the root, for a lane that stands for none or for one of the group's own)
};

// level_shift0 = 30 - 2 depth, as WalkerT keeps it: level_base(depth - h) = 0x55555555 >> (level_shift0 + 2 + 2 h)
PCPX_PATH_START_FN PathLane path_lane(std::uint32_t lane, std::uint32_t g, std::uint32_t depth, std::uint32_t level_shift0)
{
    const std::uint32_t h = lane >> 2, c = lane & 3u;
    const bool stands = h >= 1u && h < depth;
    const std::uint32_t hc = stands ? h : 1u;  // (shift counts stay in range for the other lanes)
    const std::uint32_t local = ((g >> (2u * hc - 1u)) << 2) + c;
    // the group's own: the node of height h over last-level node 2 g, (2 g) >> (2 h - 2) -- and at height 1 node 2 g + 1 as well
    const std::uint32_t pair = hc == 1u ? 1u : 0u;
    const bool own = (local >> pair) == ((2u * g) >> (2u * hc - 2u + pair));
    const std::uint32_t base = 0x55555555u >> ((level_shift0 + 2u + 2u * hc) & 31u);
    PathLane out;
    out.on = stands && !own;
    out.node = out.on ? base + local : 0u;
    return out;
}

}  // namespace pcpx

#undef PCPX_PATH_START_FN
#endif
