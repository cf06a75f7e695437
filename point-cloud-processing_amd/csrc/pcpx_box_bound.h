// pcpx_box_bound.h -- the fused box bound of k_knn's node tests, and the slack that makes it safe.  Host and device: included by
// pcpx_device.h under hipcc and, alone, by a plain C++ program (tests/cpp/box_bound.cpp), which brings its own box type -- anything
// with lo(axis), hi(axis) and a float `poison`, like NodeBox (pcpx_internal.h).
//
// box_d2 (pcpx_device.h) sums the squared axis distances the way the reference sums a point's: fl(fl(fl(dx^2) + fl(dy^2)) + fl(dz^2)),
// five instructions and one more for `poison`.  A node test only prunes, so any value that is, in float, a lower bound of every
// contained point's reference d2 selects the same rows; box_bound_fused forms the sum with three FMAs, `poison` as the first addend.
// That value can exceed the unfused one by an ulp (about one box in ten), so it is compared with a slackened tau:
//
//     need(box)  <=>  box_bound_fused(box, q) <= box_bound_tau(tau),    box_bound_tau(tau) = tau * (1 + 2^-20) + FLT_MIN
//
// Claim: for every point p inside the box with reference d2 R <= tau the test holds (the box is never pruned while it holds a
// point that could still be taken).  With u = 2^-24, e_a = fl(p_a - q_a) and d_a the box's axis distance:
//   * lo_a <= p_a <= hi_a and rounding is monotone, so fl(lo_a - q_a) <= e_a <= -fl(q_a - hi_a): d_a <= |e_a| on every axis, as for
//     box_d2.  FMA and fl are monotone in non-negative operands, so F = fused(d) <= fused(|e|) =: F'.
//   * a = fl(ex^2), b = fl(ey^2), c = fl(ez^2): R = fl(fl(a + b) + c), F' = fl(ez^2 + fl(ey^2 + a)) -- two products unrounded.
//     In the normal range ey^2 <= b / (1 - u), ez^2 <= c / (1 - u), a + b <= fl(a + b) / (1 - u), fl(a + b) + c <= R / (1 - u), so
//         fl(ey^2 + a) <= (a + b) (1 + u) / (1 - u) <= fl(a + b) (1 + u) / (1 - u)^2
//         F' <= (ez^2 + fl(ey^2 + a)) (1 + u) <= (fl(a + b) + c) (1 + u)^2 / (1 - u)^2 <= R (1 + u)^2 / (1 - u)^3 < R (1 + 5.1 u).
//   * K = 1 + 16 u: fl(tau K) >= tau K (1 - u) > tau (1 + 14 u), and adding FLT_MIN never rounds below the first addend.  So
//     box_bound_tau(tau) > tau (1 + 14 u) >= R (1 + 14 u) > F' >= F.
//   * Where a product or a sum falls below FLT_MIN, a rounding errs by at most 2^-150 absolutely instead of u relatively (sums
//     of floats are exact there): a handful of such errors on either side, against FLT_MIN = 2^-126 added to tau.
// Edges: tau = +inf stays +inf; an idle lane's tau = -1 stays negative and F >= 0, so it needs nothing; tau = 0 (coincident points,
// eps 0) becomes FLT_MIN, and a box that contains the query gives F = 0; a padding node's NaN `poison` makes F NaN: the test fails.
// tau itself, and every candidate test d2 <= tau, stay exact: the slack only ever lets a few more boxes through.
#ifndef PCPX_BOX_BOUND_H
#define PCPX_BOX_BOUND_H

#include <cfloat>
#include <cmath>

#if defined(__HIPCC__)
#define PCPX_BOX_BOUND_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define PCPX_BOX_BOUND_FN inline
#endif

namespace pcpx {

// (the FMAs are written out: the build has -ffp-contract=off, and a contraction the compiler chose would not be this one)
template <class Box>
PCPX_BOX_BOUND_FN float box_bound_fused(const Box& b, float qx, float qy, float qz)
{
    const float dx = fmaxf(fmaxf(b.lo(0) - qx, qx - b.hi(0)), 0.f);  // the axis distances exactly as box_d2 forms them
    const float dy = fmaxf(fmaxf(b.lo(1) - qy, qy - b.hi(1)), 0.f);
    const float dz = fmaxf(fmaxf(b.lo(2) - qz, qz - b.hi(2)), 0.f);
    return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, __builtin_fmaf(dx, dx, b.poison)));
}

constexpr float BOX_BOUND_K = 1.f + 0x1p-20f;

PCPX_BOX_BOUND_FN float box_bound_tau(float tau) { return tau * BOX_BOUND_K + FLT_MIN; }

// The same bound from a box U to a whole box W of queries (k_knn's path start, WalkerT::start_path: W = the tight box of a wave's 64
// queries, tau = the round's cap, which no lane's tau exceeds):
//
//     box_gap_bound_fused(U, W) <= box_bound_tau(cap)   whenever some p in U and q in W have reference d2(p, q) <= cap.
//
// The argument above carries over with g_a = max(fl(lo_U - hi_W), fl(lo_W - hi_U), 0) in the place of the axis distance d_a:
//   * lo_U <= p_a and q_a <= hi_W give lo_U - hi_W <= p_a - q_a in the reals, and rounding is monotone: fl(lo_U - hi_W) <= e_a;
//     likewise fl(lo_W - hi_U) <= fl(q_a - p_a) = -e_a.  So g_a <= |e_a| on every axis -- the only property of d_a the argument uses
//     -- and F = fused(g) <= fused(|e|) = F' < R (1 + 5.1 u) < box_bound_tau(R) <= box_bound_tau(cap), box_bound_tau being monotone.
//   * For any one query q in W, g_a <= d_a(U, q) as well (q_a <= hi_W, lo_W <= q_a): the value never exceeds box_bound_fused(U, q), so
//     a box this test drops is one the per-lane test drops for every lane whose tau is within the cap.
// Edges as above: cap = +inf passes every real box (the gaps of finite boxes are finite or overflow to +inf, and +inf <= +inf);
// cap = 0 becomes FLT_MIN, and touching or overlapping boxes give 0; U's NaN `poison` makes the value NaN: the test fails.
// W needs lo(axis) and hi(axis) only.
template <class Box, class QueryBox>
PCPX_BOX_BOUND_FN float box_gap_bound_fused(const Box& u, const QueryBox& w)
{
    const float gx = fmaxf(fmaxf(u.lo(0) - w.hi(0), w.lo(0) - u.hi(0)), 0.f);
    const float gy = fmaxf(fmaxf(u.lo(1) - w.hi(1), w.lo(1) - u.hi(1)), 0.f);
    const float gz = fmaxf(fmaxf(u.lo(2) - w.hi(2), w.lo(2) - u.hi(2)), 0.f);
    return __builtin_fmaf(gz, gz, __builtin_fmaf(gy, gy, __builtin_fmaf(gx, gx, u.poison)));
}

}  // namespace pcpx

#undef PCPX_BOX_BOUND_FN
#endif
