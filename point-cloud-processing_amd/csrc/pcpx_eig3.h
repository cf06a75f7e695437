// pcpx_eig3.h -- PCA normal of a 3x3 scatter matrix (shared by the fused kNN kernel, k_normals, the radius normals, MLS and the
// shape features).  Device code under hipcc; alone, a plain C++ program can include it too (tests/cpp/eig3_shape.cpp), where one
// "lane" is the whole wave.
#ifndef PCPX_EIG3_H
#define PCPX_EIG3_H

#if defined(__HIPCC__)
#include "pcpx_device.h"
#define PCPX_EIG3_INLINE __device__ __forceinline__
#define PCPX_EIG3_FN __device__
#else
#include <cmath>
#include <limits>
#define PCPX_EIG3_INLINE inline
#define PCPX_EIG3_FN inline
#endif

namespace pcpx {
namespace {

#if defined(__HIPCC__)
__device__ __forceinline__ bool eig_any(bool c) { return any_lane(c); }
#else
inline bool eig_any(bool c) { return c; }
#endif

// ------------------------------------------------------------------------------------------------
// PCA normal of one neighbourhood per thread.
// Restates pcp::estimate_normal (include/pcp/common/normals/normal_estimation.hpp:41-77): row mean,
// centred scatter matrix V'V'^T (not divided by n), Eigen 3.3.8 SelfAdjointEigenSolver<Matrix3f>
// ::compute (scale, closed-form 3x3 tridiagonalisation, implicit-shift QL, ascending sort), column of
// the smallest eigenvalue with the reference's "last tie wins" ifs.  All in float32 without FMA, in
// the same operation order as the CPU restatement used by the tests, so results are bit-comparable with it.
//
// The QL part is shaped for a wave: the 64 lanes of a wave sit in different branches of Eigen's code in the same trip (which
// Givens arm, which column pair, which end), and a wave pays for every branch one of its lanes takes.  So each lane evaluates
// one arm on selected operands and discards what it does not need; the float operations a lane keeps, and their order, are
// Eigen's (tests/cpp/eig3_shape.cpp compares with the branching form bit for bit).
// ------------------------------------------------------------------------------------------------

// Eigen's two arms, |p| > |q| and not, are one: t = num / den, u = +-sqrt(1 + t^2), r = 1 / u, m = t r, and
//   |p| > |q|:  c = 1 / u = r,                   s = -t c = -(t r) = -m
//   otherwise:  s = -1 / u = -(1 / u) = -r,      c = -t s = (-t)(-r) = t r = m
// (negation commutes with a rounded product or quotient).  A lane with p == 0 or q == 0 divides 0 or by 0 and drops the result.
PCPX_EIG3_INLINE void make_givens(float p, float q, float& c, float& s)
{
    const bool big = fabsf(p) > fabsf(q);
    const float num = big ? q : p, den = big ? p : q;
    const float t = num / den;
    float u = sqrtf(1.f + t * t);
    if (den < 0.f) u = -u;
    const float r = 1.f / u, m = t * r;
    c = big ? r : m;
    s = big ? -m : -r;
    if (p == 0.f) {
        c = 0.f;
        s = q < 0.f ? 1.f : -1.f;
    }
    if (q == 0.f) {  // (tested first by Eigen: applied last)
        c = p < 0.f ? -1.f : 1.f;
        s = 0.f;
    }
}

PCPX_EIG3_INLINE float eig_hypot(float x, float y)
{
    const float ax = fabsf(x), ay = fabsf(y);
    const bool xbig = ax > ay;
    const float p = xbig ? ax : ay, qp = (xbig ? ay : ax) / p;
    const float h = p * sqrtf(1.f + qp * qp);
    return p == 0.f ? 0.f : h;
}

// The tridiagonal matrix {diagonal d, subdiagonal e} and the accumulated rotations Q, in registers.
struct Ql3 {
    float d0, d1, d2, e0, e1;
    float q00, q10, q20, q01, q11, q21, q02, q12, q22;
};

constexpr int QL3_MAX_TRIPS = 90;  // Eigen's m_maxIterations * n = 30 * 3

// Implicit-shift QL sweeps until both subdiagonal entries are deflated; false if a lane would need more than QL3_MAX_TRIPS trips
// (it then stops where it is, as Eigen's NoConvergence does).  trips_done > 0 is for the test of that cap.
// A trip works on the block start ... end of the lane: {0,1}, {0,2} or {1,2}.  Its one or two rotations sit at two fixed
// sites, k = 0 on columns 0 and 1 for start == 0, then k = 1 on columns 1 and 2 for end == 2, each an exec-masked region that
// is skipped when no lane wants it.  A lane that is done (end == 0) passes through selects that keep what it has.
PCPX_EIG3_INLINE bool ql3_iterate(Ql3& m, int trips_done = 0)
{
    const float tiny = std::numeric_limits<float>::min();
    const float precision = 2.f * std::numeric_limits<float>::epsilon();
    float d0 = m.d0, d1 = m.d1, d2 = m.d2, e0 = m.e0, e1 = m.e1;
    float q00 = m.q00, q10 = m.q10, q20 = m.q20, q01 = m.q01, q11 = m.q11, q21 = m.q21, q02 = m.q02, q12 = m.q12, q22 = m.q22;
    int end = 2, start = 0;
    bool converged = true;
    for (int trip = trips_done + 1;; ++trip) {  // (a lane is in every trip until it is done: the count is the wave's)
        if (start == 0 && end > 0 && (fabsf(e0) <= (fabsf(d0) + fabsf(d1)) * precision || fabsf(e0) <= tiny)) e0 = 0.f;
        if (end == 2 && (fabsf(e1) <= (fabsf(d1) + fabsf(d2)) * precision || fabsf(e1) <= tiny)) e1 = 0.f;
        if (end == 2 && e1 == 0.f) end = 1;
        if (end == 1 && e0 == 0.f) end = 0;
        if (end > 0 && trip > QL3_MAX_TRIPS) {
            converged = false;
            end = 0;
        }
        if (!eig_any(end > 0)) break;
        start = (end == 2 && e0 != 0.f) ? 0 : end - 1;  // (-1 for a lane that is done: neither site, no deflation test)
        // Wilkinson shift from the trailing 2x2 block
        const bool two = end == 2;
        const float dem1 = two ? d1 : d0, de = two ? d2 : d1, ee = two ? e1 : e0;
        const float td = (dem1 - de) * 0.5f;
        const float e2 = ee * ee;
        const float h = eig_hypot(td, ee);
        float mu = de - e2 / (td + (td > 0.f ? h : -h));
        const bool e2_underflowed = end > 0 && td != 0.f && e2 == 0.f;
        if (eig_any(e2_underflowed)) {
            const float other = de - (ee / (td + (td > 0.f ? 1.f : -1.f))) * (ee / h);
            mu = e2_underflowed ? other : mu;
        }
        if (td == 0.f) mu = de - fabsf(ee);
        float x = (start == 0 ? d0 : d1) - mu;
        float z = start == 0 ? e0 : e1;
        if (start == 0) {  // k = 0: rows and columns 0, 1
            float c, s;
            make_givens(x, z, c, s);
            const float sdk = s * d0 + c * e0;
            const float dkp1 = s * e0 + c * d1;
            const float ndk = c * (c * d0 - s * e0) - s * (c * e0 - s * d1);
            d0 = ndk;
            d1 = s * sdk + c * dkp1;
            e0 = c * sdk - s * dkp1;
            x = e0;
            if (end == 2) {  // the bulge for k = 1
                z = -s * e1;
                e1 = c * e1;
            }
            float a, b;
            a = q00; b = q01; q00 = c * a - s * b; q01 = s * a + c * b;
            a = q10; b = q11; q10 = c * a - s * b; q11 = s * a + c * b;
            a = q20; b = q21; q20 = c * a - s * b; q21 = s * a + c * b;
        }
        if (end == 2) {  // k = 1: rows and columns 1, 2
            float c, s;
            make_givens(x, z, c, s);
            const float sdk = s * d1 + c * e1;
            const float dkp1 = s * e1 + c * d2;
            const float ndk = c * (c * d1 - s * e1) - s * (c * e1 - s * d2);
            d1 = ndk;
            d2 = s * sdk + c * dkp1;
            e1 = c * sdk - s * dkp1;
            if (start == 0) e0 = c * e0 - s * z;
            float a, b;
            a = q01; b = q02; q01 = c * a - s * b; q02 = s * a + c * b;
            a = q11; b = q12; q11 = c * a - s * b; q12 = s * a + c * b;
            a = q21; b = q22; q21 = c * a - s * b; q22 = s * a + c * b;
        }
    }
    m.d0 = d0; m.d1 = d1; m.d2 = d2; m.e0 = e0; m.e1 = e1;
    m.q00 = q00; m.q10 = q10; m.q20 = q20; m.q01 = q01; m.q11 = q11; m.q21 = q21; m.q02 = q02; m.q12 = q12; m.q22 = q22;
    return converged;
}

// AXIS: also the column of the largest eigenvalue after the ascending sort (column 2) in axis[3] -- the principal axis of the
// shape features (pcpx_range.hip, k_range_features); the default form is what every other caller compiles.
template <bool AXIS = false>
PCPX_EIG3_FN void eig3_smallest(float a00, float a10, float a20, float a11, float a21, float a22, float normal[3],
                                float evals[3], float* axis = nullptr)
{
    float scale = fmaxf(fmaxf(fmaxf(fabsf(a00), fabsf(a10)), fmaxf(fabsf(a20), fabsf(a11))),
                        fmaxf(fabsf(a21), fabsf(a22)));
    if (scale == 0.f) scale = 1.f;
    a00 /= scale; a10 /= scale; a20 /= scale; a11 /= scale; a21 /= scale; a22 /= scale;
    float d0, d1, d2, e0, e1;
    float q00 = 1.f, q10 = 0.f, q20 = 0.f, q01 = 0.f, q11 = 1.f, q21 = 0.f, q02 = 0.f, q12 = 0.f, q22 = 1.f;
    const float tiny = std::numeric_limits<float>::min();
    d0 = a00;
    float v1norm2 = a20 * a20;
    if (v1norm2 <= tiny) {
        d1 = a11; d2 = a22; e0 = a10; e1 = a21;
    } else {
        float beta = sqrtf(a10 * a10 + v1norm2);
        float inv_beta = 1.f / beta;
        float m01 = a10 * inv_beta, m02 = a20 * inv_beta;
        float q = 2.f * m01 * a21 + m02 * (a22 - a11);
        d1 = a11 + m02 * q;
        d2 = a22 - m02 * q;
        e0 = beta;
        e1 = a21 - m01 * q;
        q11 = m01; q21 = m02; q12 = m02; q22 = -m01;
    }
    // registers instead of arrays: diag = {d0,d1,d2}, sub = {e0,e1}, Q columns {q?0,q?1,q?2}
    Ql3 m = {d0, d1, d2, e0, e1, q00, q10, q20, q01, q11, q21, q02, q12, q22};
    const bool converged = ql3_iterate(m);
    d0 = m.d0; d1 = m.d1; d2 = m.d2;
    q00 = m.q00; q10 = m.q10; q20 = m.q20; q01 = m.q01; q11 = m.q11; q21 = m.q21; q02 = m.q02; q12 = m.q12; q22 = m.q22;
    if (converged) {
        // ascending selection sort (first minimum wins), swapping eigenvector columns
        auto swap01 = [&]() {
            float t;
            t = d0; d0 = d1; d1 = t;
            t = q00; q00 = q01; q01 = t; t = q10; q10 = q11; q11 = t; t = q20; q20 = q21; q21 = t;
        };
        auto swap02 = [&]() {
            float t;
            t = d0; d0 = d2; d2 = t;
            t = q00; q00 = q02; q02 = t; t = q10; q10 = q12; q12 = t; t = q20; q20 = q22; q22 = t;
        };
        auto swap12 = [&]() {
            float t;
            t = d1; d1 = d2; d2 = t;
            t = q01; q01 = q02; q02 = t; t = q11; q11 = q12; q12 = t; t = q21; q21 = q22; q22 = t;
        };
        int kmin = 0;
        float mv = d0;
        if (d1 < mv) { mv = d1; kmin = 1; }
        if (d2 < mv) { mv = d2; kmin = 2; }
        if (kmin == 1) swap01();
        else if (kmin == 2) swap02();
        if (d2 < d1) swap12();
    }
    float l0 = d0 * scale, l1 = d1 * scale, l2 = d2 * scale;
    evals[0] = l0; evals[1] = l1; evals[2] = l2;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    if (l0 <= l1 && l0 <= l2) { nx = q00; ny = q10; nz = q20; }
    if (l1 <= l0 && l1 <= l2) { nx = q01; ny = q11; nz = q21; }
    if (l2 <= l0 && l2 <= l1) { nx = q02; ny = q12; nz = q22; }
    normal[0] = nx; normal[1] = ny; normal[2] = nz;
    if constexpr (AXIS) { axis[0] = q02; axis[1] = q12; axis[2] = q22; }
}

}  // namespace
}  // namespace pcpx

#undef PCPX_EIG3_INLINE
#undef PCPX_EIG3_FN
#endif
