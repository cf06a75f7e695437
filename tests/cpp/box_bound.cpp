// The fused box bound of k_knn's node tests (csrc/pcpx_box_bound.h) on the host: whenever a point inside a box has a reference
// d2 <= tau, box_bound_fused(box, q) <= box_bound_tau(tau) -- the node is not pruned.  Boxes, queries and points in float32; the
// reference d2 is fl(fl(fl(ex^2) + fl(ey^2)) + fl(ez^2)) (built with -ffp-contract=off, and the products pass through volatiles).
// Prints one line of counts; exit status 0 iff no case violates the property and the cases that need the slack did occur.
#include "pcpx_box_bound.h"

#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>

namespace {

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

struct Counts {
    std::uint64_t cases = 0, premise = 0, violations = 0, corner_cases = 0, fused_above_unfused = 0, slack_needed = 0, idle_needed = 0,
                  nan_needed = 0, underflowed = 0;
};

std::mt19937_64 rng(20240917u);
float uniform(float a, float b) { return a + (b - a) * static_cast<float>(rng() >> 40) * 0x1p-24f; }

// one {box, query, contained point}: every tau of interest
void check(const Box& b, const float* q, const float* p, bool nearest, Counts& n)
{
    const float inf = std::numeric_limits<float>::infinity();
    const float R = ref_d2(p, q);
    const float F = pcpx::box_bound_fused(b, q[0], q[1], q[2]);
    if (nearest) {
        ++n.corner_cases;
        if (F > R) ++n.fused_above_unfused;  // (the point's differences ARE the box's axis distances: R is the unfused bound)
    }
    if (R != 0.f && R < 1e-37f) ++n.underflowed;
    const float taus[] = {R, std::nextafter(R, inf), R * uniform(1.f, 4.f), std::nextafter(R, -inf), R * uniform(0.f, 1.f), inf, 0.f, -1.f};
    for (const float tau : taus) {
        ++n.cases;
        const bool needed = F <= pcpx::box_bound_tau(tau);
        if (tau == -1.f && needed) ++n.idle_needed;  // an idle lane needs nothing
        if (R <= tau) {
            ++n.premise;
            if (!needed) {
                if (++n.violations <= 10)
                    std::printf("violated: R %a F %a tau %a bound %a  q (%a %a %a) p (%a %a %a)\n", R, F, tau, pcpx::box_bound_tau(tau), q[0], q[1],
                                q[2], p[0], p[1], p[2]);
            }
            if (F > tau) ++n.slack_needed;  // the unslackened test would have pruned the box
        }
    }
    // a padding node: NaN poison, needed by nobody whatever tau is
    Box pad = b;
    pad.poison = std::numeric_limits<float>::quiet_NaN();
    const float Fp = pcpx::box_bound_fused(pad, q[0], q[1], q[2]);
    for (const float tau : {R, inf, 0.f, -1.f}) {
        ++n.cases;
        if (!std::isnan(Fp) || Fp <= pcpx::box_bound_tau(tau)) ++n.nan_needed;
    }
}

// clouds at `offset` with boxes of `extent`, queries up to `reach` extents away
void family(float offset, float extent, float reach, int boxes, Counts& n)
{
    for (int i = 0; i < boxes; ++i) {
        Box b{};
        float q[3], inside[3], nearest[3];
        for (int a = 0; a < 3; ++a) {
            const float c = offset + uniform(-1.f, 1.f) * extent * 8.f;
            const float u = c + uniform(-1.f, 1.f) * extent, v = c + uniform(-1.f, 1.f) * extent;
            b.lo3[a] = std::fmin(u, v);
            b.hi3[a] = std::fmax(u, v);
            // per axis: below the box, above it, or within its range (so corners, edges, faces and the inside all occur)
            const std::uint64_t side = rng() % 3u;
            q[a] = side == 0 ? b.lo3[a] - uniform(0.f, reach) * extent : side == 1 ? b.hi3[a] + uniform(0.f, reach) * extent : uniform(b.lo3[a], b.hi3[a]);
            inside[a] = std::fmin(std::fmax(uniform(b.lo3[a], b.hi3[a]), b.lo3[a]), b.hi3[a]);
            nearest[a] = std::fmin(std::fmax(q[a], b.lo3[a]), b.hi3[a]);  // the box's corner / edge / face point nearest the query
        }
        check(b, q, nearest, true, n);
        check(b, q, inside, false, n);
    }
}

}  // namespace

int main()
{
    Counts n;
    const int boxes = 12000;
    for (const float reach : {0.05f, 1.f, 30.f}) {
        family(0.f, 1.f, reach, boxes, n);
        for (const float offset : {1e3f, 5e4f})
            for (const float extent : {1e-2f, 1e-1f, 1.f}) family(offset, extent, reach, boxes, n);
        family(0.f, 1e-20f, reach, boxes, n);  // squares underflow
        family(0.f, 1e-18f, reach, boxes, n);
        family(0.f, 3e-19f, reach, boxes, n);  // squares land among the subnormals
    }
    std::printf("{\"cases\": %" PRIu64 ", \"premise_held\": %" PRIu64 ", \"violations\": %" PRIu64 ", \"nearest_point_cases\": %" PRIu64
                ", \"fused_above_unfused\": %" PRIu64 ", \"slack_needed\": %" PRIu64 ", \"idle_lane_needed\": %" PRIu64 ", \"padding_needed\": %" PRIu64
                ", \"tiny_d2\": %" PRIu64 "}\n",
                n.cases, n.premise, n.violations, n.corner_cases, n.fused_above_unfused, n.slack_needed, n.idle_needed, n.nan_needed, n.underflowed);
    const bool ok = n.violations == 0 && n.idle_needed == 0 && n.nan_needed == 0 && n.cases >= 1000000u && n.fused_above_unfused > 0 &&
                    n.slack_needed > 0 && n.underflowed > 0;
    return ok ? 0 : 1;
}
