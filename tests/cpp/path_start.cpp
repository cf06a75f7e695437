// k_knn's path start (csrc/pcpx_device.h, WalkerT::start_path) on the host, in two parts.
//
// 1. The bound (csrc/pcpx_box_bound.h): for boxes U and W, points p in U and q in W and a cap, whenever the reference's float
//    d2(p, q) <= cap, box_gap_bound_fused(U, W) <= box_bound_tau(cap).  Disjoint, touching and overlapping boxes, corners an ulp apart,
//    coordinates near 1e6, squares that underflow, cap = d2 exactly, its float neighbours, 0, +inf and FLT_MAX; a NaN-poisoned U fails
//    every cap.  Built with -ffp-contract=off; the reference's products pass through volatiles.
//
// 2. The walker.  Implicit trees of depth 2 ... 15 (a node's box is a cell of a nested subdivision, a leaf's lies inside its cell;
//    nodes beyond the last real one of a level are NaN-poisoned padding), so that no tree is ever stored.  For a group g -- the first,
//    the last, and paths through child 0 and child 3 at every level -- 64 queries inside the group's own leaves, each with a tau
//    within the round's cap: the start state of pcpx_path_start.h's lanes, driven through a restatement of pop_scaled / expand_any
//    with the exact per-lane test, must visit, outside the seed range, exactly the leaves the root start visits, and every node it
//    expands that the root start does not must yield an empty mask.
//
// Prints one line of counts; exit status 0 iff nothing is violated and the cases of interest did occur.
#include "pcpx_box_bound.h"
#include "pcpx_path_start.h"

#include <algorithm>
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>
#include <set>
#include <vector>

namespace {

using u32 = std::uint32_t;
using u64 = std::uint64_t;
const float INF = std::numeric_limits<float>::infinity();

struct Box {
    float lo3[3], hi3[3], poison, pad;
    float lo(int a) const { return lo3[a]; }
    float hi(int a) const { return hi3[a]; }
};

float ref_d2(const float* p, const float* q)
{
    volatile float ex = p[0] - q[0], ey = p[1] - q[1], ez = p[2] - q[2];
    volatile float a = ex * ex, b = ey * ey, c = ez * ez;
    volatile float ab = a + b;
    return ab + c;
}

std::mt19937_64 rng(20250611u);
float uniform(float a, float b) { return a + (b - a) * static_cast<float>(rng() >> 40) * 0x1p-24f; }
float inside(float lo, float hi) { return std::fmin(std::fmax(uniform(lo, hi), lo), hi); }

// ---- 1. the bound ----------------------------------------------------------------------------------------------------------------

struct BoundCounts {
    u64 cases = 0, premise = 0, violations = 0, slack_needed = 0, touching = 0, overlapping = 0, ulp_apart = 0, tiny = 0, far = 0,
        poisoned_passed = 0, inf_failed = 0;
};

void check_bound(const Box& u, const Box& w, const float* p, const float* q, BoundCounts& n)
{
    const float R = ref_d2(p, q);
    const float F = pcpx::box_gap_bound_fused(u, w);
    if (R != 0.f && R < 1e-37f) ++n.tiny;
    const float caps[] = {R, std::nextafter(R, INF), std::nextafter(R, -INF), R * uniform(1.f, 4.f), R * uniform(0.f, 1.f), 0.f, INF, FLT_MAX};
    for (const float cap : caps) {
        ++n.cases;
        const bool passes = F <= pcpx::box_bound_tau(cap);
        if (cap == INF && !passes) ++n.inf_failed;  // the uncapped round passes every real box
        if (R <= cap) {
            ++n.premise;
            if (!passes && ++n.violations <= 10)
                std::printf("violated: R %a F %a cap %a bound %a  p (%a %a %a) q (%a %a %a)\n", R, F, cap, pcpx::box_bound_tau(cap), p[0], p[1], p[2],
                            q[0], q[1], q[2]);
            if (F > cap) ++n.slack_needed;
        }
    }
    Box poisoned = u;
    poisoned.poison = std::numeric_limits<float>::quiet_NaN();
    const float Fp = pcpx::box_gap_bound_fused(poisoned, w);
    for (const float cap : {R, 0.f, INF, FLT_MAX}) {
        ++n.cases;
        if (!std::isnan(Fp) || Fp <= pcpx::box_bound_tau(cap)) ++n.poisoned_passed;
    }
}

// boxes of `extent` around `offset`; per axis W lies below U, above it, touches it, is an ulp away, or overlaps it
void bound_family(float offset, float extent, float reach, int boxes, BoundCounts& n)
{
    for (int i = 0; i < boxes; ++i) {
        Box u{}, w{};
        float pn[3], qn[3], pi[3], qi[3];
        bool touch = false, overlap = true, ulp = false;
        for (int a = 0; a < 3; ++a) {
            const float c = offset + uniform(-1.f, 1.f) * extent * 8.f;
            const float s = c + uniform(-1.f, 1.f) * extent, t = c + uniform(-1.f, 1.f) * extent;
            u.lo3[a] = std::fmin(s, t);
            u.hi3[a] = std::fmax(s, t);
            const float size = uniform(0.f, 2.f) * extent;
            const u64 side = rng() % 6u;
            float wlo;
            if (side == 0) wlo = u.hi3[a] + uniform(0.f, reach) * extent;                // above, at a distance
            else if (side == 1) wlo = u.lo3[a] - size - uniform(0.f, reach) * extent;     // below
            else if (side == 2) wlo = u.hi3[a], touch = true;                              // touching from above
            else if (side == 3) wlo = std::nextafter(u.hi3[a], INF), ulp = true;           // an ulp above
            else wlo = uniform(u.lo3[a] - size, u.hi3[a]);                                  // overlapping
            w.lo3[a] = wlo;
            w.hi3[a] = side == 1 && rng() % 4u == 0 ? std::nextafter(u.lo3[a], -INF) : std::fmax(wlo + size, wlo);  // (below: sometimes an ulp below)
            if (w.hi3[a] < w.lo3[a]) w.hi3[a] = w.lo3[a];
            overlap = overlap && w.lo3[a] <= u.hi3[a] && u.lo3[a] <= w.hi3[a];
            // the nearest pair of the two intervals, and a pair anywhere inside
            pn[a] = std::fmin(std::fmax(w.lo3[a], u.lo3[a]), u.hi3[a]);
            if (w.hi3[a] < u.lo3[a]) pn[a] = u.lo3[a];
            qn[a] = std::fmin(std::fmax(pn[a], w.lo3[a]), w.hi3[a]);
            pi[a] = inside(u.lo3[a], u.hi3[a]);
            qi[a] = inside(w.lo3[a], w.hi3[a]);
        }
        n.touching += touch, n.overlapping += overlap, n.ulp_apart += ulp;
        if (std::fabs(offset) >= 9e5f) ++n.far;
        check_bound(u, w, pn, qn, n);
        check_bound(u, w, pi, qi, n);
        check_bound(u, w, pn, qi, n);
    }
}

// ---- 2. the walker ---------------------------------------------------------------------------------------------------------------

u32 level_base(int d) { return d == 0 ? 0u : 0x55555555u >> (32 - 2 * d); }

struct Tree {
    int depth;
    u32 nleaves;
    float inset;  // a leaf's box: its cell, drawn in by this share of the cell on every side
    u32 nreal(int d) const
    {
        const int sh = 2 * (depth - d);
        return static_cast<u32>((static_cast<u64>(nleaves) + (1ull << sh) - 1ull) >> sh);
    }
    // node `local` of level d: the cell reached from the unit cube by its base-4 digits, level j halving axes j % 3 and (j + 1) % 3
    Box box(int d, u32 local) const
    {
        Box b{};
        float lo[3] = {0.f, 0.f, 0.f}, size[3] = {1.f, 1.f, 1.f};
        for (int j = 1; j <= d; ++j) {
            const u32 digit = (local >> (2 * (d - j))) & 3u;
            const int a0 = j % 3, a1 = (j + 1) % 3;
            size[a0] *= 0.5f, size[a1] *= 0.5f;
            lo[a0] += (digit & 1u) ? size[a0] : 0.f;
            lo[a1] += (digit & 2u) ? size[a1] : 0.f;
        }
        const float in = d == depth ? inset : 0.f;
        for (int a = 0; a < 3; ++a) b.lo3[a] = lo[a] + in * size[a], b.hi3[a] = lo[a] + size[a] - in * size[a];
        b.poison = local < nreal(d) ? 0.f : std::numeric_limits<float>::quiet_NaN();
        return b;
    }
    Box by_heap_id(u32 id) const
    {
        int d = 0;
        while (d < depth && id >= level_base(d + 1)) ++d;
        return box(d, id - level_base(d));
    }
};

struct Lanes {
    float q[64][3], tau[64];
    u32 mask(const Tree& t, u32 first_child) const  // WalkerT::child_mask_at with the exact per-lane test
    {
        u32 m = 0;
        for (u32 c = 0; c < 4; ++c) {
            const Box b = t.by_heap_id(first_child + c);
            bool any = false;
            for (int i = 0; i < 64 && !any; ++i) any = pcpx::box_bound_fused(b, q[i][0], q[i][1], q[i][2]) <= pcpx::box_bound_tau(tau[i]);
            m |= any ? 1u << c : 0u;
        }
        return m;
    }
};

struct Walk {  // WalkerT's state and pop_scaled / expand_any, restated
    u64 pend;
    u32 ploc, l2, lshift0;
    std::set<u32> leaves;              // visited outside the seed range
    std::vector<std::pair<u32, u32>> expanded;  // (first child's heap id, mask)
    void run(const Tree& t, const Lanes& ln, u32 s0, u32 seed_count)
    {
        while (pend != 0) {
            const u32 bit = static_cast<u32>(__builtin_ctzll(pend));
            pend &= ~(1ull << bit);
            const u32 h4 = bit & ~3u;
            const u32 up = ploc >> ((h4 >> 1) - l2);
            const u32 loc = (up << 2) + (bit & 3u);
            const u32 h2 = h4 >> 1;
            const u32 first_child = (loc << 2) + (0x55555555u >> (lshift0 + h2));
            const u32 m = ln.mask(t, first_child);
            expanded.emplace_back(first_child, m);
            l2 = h2 - 2u;
            ploc = loc;
            if (h4 != 4u) {
                pend |= static_cast<u64>(m) << (h4 - 4u);
            } else {
                for (u32 c = 0; c < 4; ++c)
                    if ((m >> c) & 1u) {
                        const u32 leaf = (loc << 2) + c;
                        if (leaf - s0 >= seed_count) leaves.insert(leaf);
                    }
            }
        }
    }
};

struct WalkCounts {
    u64 cases = 0, leaf_set_differs = 0, extra_with_mask = 0, extra_expansions = 0, leaves = 0, padded_own = 0, uncapped = 0, saved = 0,
        bad_lane = 0;
    int depth_lo = 99, depth_hi = 0;
};

void walk_case(const Tree& t, u32 g, float cap, u32 seed_extra, WalkCounts& n)
{
    const int depth = t.depth;
    // the queries: eight inside each of the group's real leaves, taus within the cap, some lanes idle
    Lanes ln;
    const u32 own_leaves = std::min<u32>(8u, t.nleaves - 8u * g);
    const float cell = std::ldexp(1.f, -2 * depth / 3);
    for (int i = 0; i < 64; ++i) {
        const Box b = t.box(depth, 8u * g + static_cast<u32>(i) % own_leaves);
        for (int a = 0; a < 3; ++a) ln.q[i][a] = inside(b.lo3[a], b.hi3[a]);
        const float want = cell * cell * uniform(0.f, 6.f);
        ln.tau[i] = rng() % 8u == 0 ? -1.f : rng() % 8u == 0 ? cap : std::fmin(want, cap);
    }
    u32 s0 = 8u * g, s1 = std::min(s0 + 8u, t.nleaves);
    s0 = s0 > seed_extra ? s0 - seed_extra : 0u;
    s1 = std::min(s1 + seed_extra, t.nleaves);
    const u32 lshift0 = static_cast<u32>(30 - 2 * depth);

    Walk root{};  // WalkerT::start: the root's children pending (every searching lane is inside the root)
    root.lshift0 = lshift0, root.ploc = 0, root.l2 = 2u * static_cast<u32>(depth - 1);
    const u32 m0 = ln.mask(t, 1u);
    root.expanded.emplace_back(1u, m0);
    root.pend = static_cast<u64>(m0) << (4 * (depth - 1));
    root.run(t, ln, s0, s1 - s0);

    Walk path{};  // WalkerT::start_path
    path.lshift0 = lshift0, path.ploc = g >> 1, path.l2 = 2;
    const Box own0 = t.box(depth - 1, 2u * g), own1 = t.box(depth - 1, 2u * g + 1u);
    Box w = own0;
    if (own1.poison == 0.f) {
        for (int a = 0; a < 3; ++a) w.lo3[a] = std::fmin(own0.lo3[a], own1.lo3[a]), w.hi3[a] = std::fmax(own0.hi3[a], own1.hi3[a]);
    } else {
        ++n.padded_own;
    }
    for (u32 lane = 0; lane < 64; ++lane) {
        const pcpx::PathLane pl = pcpx::path_lane(lane, g, static_cast<u32>(depth), lshift0);
        if (!pl.on) {
            if (pl.node != 0u) ++n.bad_lane;
            continue;
        }
        // the lane's node is child lane % 4 of the ancestor of height lane / 4 + 1, not one of the group's own
        const u32 h = lane >> 2;
        const u32 local = pl.node - level_base(depth - static_cast<int>(h));
        if (pl.node < level_base(depth - static_cast<int>(h)) || (local >> 2) != ((8u * g) >> (2 * (h + 1))) || (local & 3u) != (lane & 3u) ||
            local == ((8u * g) >> (2 * h)) || (h == 1 && local == ((8u * g) >> 2) + 1u))
            ++n.bad_lane;
        if (pcpx::box_gap_bound_fused(t.by_heap_id(pl.node), w) <= pcpx::box_bound_tau(cap)) path.pend |= 1ull << lane;
    }
    path.run(t, ln, s0, s1 - s0);

    ++n.cases;
    n.depth_lo = std::min(n.depth_lo, depth), n.depth_hi = std::max(n.depth_hi, depth);
    if (cap == INF) ++n.uncapped;
    n.leaves += root.leaves.size();
    if (root.leaves != path.leaves && ++n.leaf_set_differs <= 5)
        std::printf("leaf sets differ: depth %d nleaves %u g %u cap %a: root %zu path %zu\n", depth, t.nleaves, g, cap, root.leaves.size(), path.leaves.size());
    std::set<u32> by_root;
    for (const auto& e : root.expanded) by_root.insert(e.first);
    for (const auto& e : path.expanded)
        if (!by_root.count(e.first)) {
            ++n.extra_expansions;
            if (e.second != 0u) ++n.extra_with_mask;
        }
    // (one step of the wave stands for the root's expansion)
    n.saved += root.expanded.size() - (path.expanded.size() + 1u);
}

void walk_cases(WalkCounts& n)
{
    for (int depth = 2; depth <= 15; ++depth) {
        const u64 full = 1ull << (2 * depth), least = depth == 2 ? 2ull : (1ull << (2 * (depth - 1))) + 1ull;
        for (int rep = 0; rep < 6; ++rep) {
            Tree t;
            t.depth = depth;
            t.nleaves = static_cast<u32>(rep == 0 ? std::min<u64>(full, 0xFFFFFFF8ull) : rep == 1 ? least : least + rng() % (std::min<u64>(full, 0xFFFFFFF8ull) - least + 1ull));
            t.inset = rep % 2 ? uniform(0.f, 0.3f) : 0.f;
            const u32 groups = (t.nleaves + 7u) / 8u;
            std::vector<u32> gs = {0u, groups - 1u, groups > 1u ? groups - 2u : 0u, static_cast<u32>(rng() % groups)};
            for (int level = 1; level < depth; ++level)  // child 0 and child 3 of the ancestor of height level + 1 ... (as far as real)
                for (const u32 digit : {0u, 3u}) {
                    u32 leaf = static_cast<u32>(rng() % t.nleaves);
                    leaf = (leaf & ~(3u << (2 * level))) | (digit << (2 * level));
                    if (leaf < t.nleaves) gs.push_back(leaf / 8u);
                }
            const float cell = std::ldexp(1.f, -2 * depth / 3);
            for (const u32 g : gs) {
                for (const float r : {0.f, 0.3f, 1.1f, 2.5f}) walk_case(t, g, r * r * cell * cell, static_cast<u32>(rng() % 3u) * 2u, n);
                if (depth <= 4) walk_case(t, g, INF, static_cast<u32>(rng() % 3u) * 2u, n);
            }
        }
    }
}

}  // namespace

int main()
{
    BoundCounts b;
    const int boxes = 9000;
    for (const float reach : {0.05f, 1.f, 30.f}) {
        bound_family(0.f, 1.f, reach, boxes, b);
        for (const float offset : {1e3f, 5e4f, 1e6f, -1e6f})
            for (const float extent : {1e-2f, 1.f}) bound_family(offset, extent, reach, boxes, b);
        bound_family(0.f, 1e-20f, reach, boxes, b);  // squares underflow
        bound_family(0.f, 3e-19f, reach, boxes, b);  // squares land among the subnormals
    }
    WalkCounts w;
    walk_cases(w);
    std::printf("{\"bound_cases\": %" PRIu64 ", \"premise_held\": %" PRIu64 ", \"violations\": %" PRIu64 ", \"slack_needed\": %" PRIu64
                ", \"touching\": %" PRIu64 ", \"overlapping\": %" PRIu64 ", \"ulp_apart\": %" PRIu64 ", \"tiny_d2\": %" PRIu64 ", \"near_1e6\": %" PRIu64
                ", \"poisoned_passed\": %" PRIu64 ", \"uncapped_failed\": %" PRIu64 ", \"walk_cases\": %" PRIu64 ", \"depth_lo\": %d, \"depth_hi\": %d"
                ", \"leaf_set_differs\": %" PRIu64 ", \"extra_expansions\": %" PRIu64 ", \"extra_with_mask\": %" PRIu64 ", \"bad_lane\": %" PRIu64
                ", \"leaves_visited\": %" PRIu64 ", \"padded_own_node\": %" PRIu64 ", \"uncapped_walks\": %" PRIu64 ", \"expansions_saved\": %" PRIu64 "}\n",
                b.cases, b.premise, b.violations, b.slack_needed, b.touching, b.overlapping, b.ulp_apart, b.tiny, b.far, b.poisoned_passed, b.inf_failed,
                w.cases, w.depth_lo, w.depth_hi, w.leaf_set_differs, w.extra_expansions, w.extra_with_mask, w.bad_lane, w.leaves, w.padded_own, w.uncapped,
                w.saved);
    const bool ok = b.violations == 0 && b.poisoned_passed == 0 && b.inf_failed == 0 && b.cases >= 3000000u && b.touching > 0 && b.overlapping > 0 &&
                    b.ulp_apart > 0 && b.tiny > 0 && b.far > 0 && w.leaf_set_differs == 0 && w.extra_with_mask == 0 && w.bad_lane == 0 && w.depth_lo == 2 &&
                    w.depth_hi == 15 && w.leaves > 0 && w.padded_own > 0 && w.uncapped > 0;
    return ok ? 0 : 1;
}
