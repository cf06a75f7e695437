// The wave-shaped eigen-solver (csrc/pcpx_eig3.h: one Givens arm, two fixed rotation sites, state by selects) on the host, against
// the branching form it replaced, which is kept below word for word: normal, eigenvalues and principal axis bit for bit on
//   * scatter matrices of point sets, formed as the kernels form them: k = 3 ... 32 points; free, planar, collinear, coincident and
//     lattice sets; scales 2^-20 ... 2^20; offsets up to 1 000;
//   * raw symmetric matrices with entries zero, at 2^-140, at 2^100 and of every magnitude in between;
//   * the same with inf or NaN entries: NaN where the branching form gives NaN (sign and payload free), equal bits elsewhere.
// The cap of 90 trips is reached by no finite matrix found so far; ql3_iterate is called with 90 trips already counted on a state
// that is not deflated: it must report no convergence and leave the state as it is.  What eig3_smallest does with an unconverged
// state (no sort) is not covered.
// Built with -ffp-contract=off.  Prints one line of counts; exit status 0 iff nothing differs.
#include "pcpx_eig3.h"

#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>

namespace branching {
#define __device__
#define __forceinline__ inline
// ---- the solver as it was before the wave shape, unchanged ----
__device__ __forceinline__ void make_givens(float p, float q, float& c, float& s)
{
    if (q == 0.f) {
        c = p < 0.f ? -1.f : 1.f;
        s = 0.f;
    } else if (p == 0.f) {
        c = 0.f;
        s = q < 0.f ? 1.f : -1.f;
    } else if (fabsf(p) > fabsf(q)) {
        float t = q / p;
        float u = sqrtf(1.f + t * t);
        if (p < 0.f) u = -u;
        c = 1.f / u;
        s = -t * c;
    } else {
        float t = p / q;
        float u = sqrtf(1.f + t * t);
        if (q < 0.f) u = -u;
        s = -1.f / u;
        c = -t * s;
    }
}

__device__ __forceinline__ float eig_hypot(float x, float y)
{
    float ax = fabsf(x), ay = fabsf(y);
    float p, qp;
    if (ax > ay) {
        p = ax;
        qp = ay / p;
    } else {
        p = ay;
        qp = ax / p;
    }
    if (p == 0.f) return 0.f;
    return p * sqrtf(1.f + qp * qp);
}

// AXIS: also the column of the largest eigenvalue after the ascending sort (column 2) in axis[3] -- the principal axis of the
// shape features (pcpx_range.hip, k_range_features); the default form is what every other caller compiles.
template <bool AXIS = false>
__device__ void eig3_smallest(float a00, float a10, float a20, float a11, float a21, float a22, float normal[3],
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
    const float precision = 2.f * std::numeric_limits<float>::epsilon();
    int end = 2, start = 0, iter = 0;
    bool converged = true;
    auto rot_cols01 = [&](float c, float s) {
        float x, y;
        x = q00; y = q01; q00 = c * x - s * y; q01 = s * x + c * y;
        x = q10; y = q11; q10 = c * x - s * y; q11 = s * x + c * y;
        x = q20; y = q21; q20 = c * x - s * y; q21 = s * x + c * y;
    };
    auto rot_cols12 = [&](float c, float s) {
        float x, y;
        x = q01; y = q02; q01 = c * x - s * y; q02 = s * x + c * y;
        x = q11; y = q12; q11 = c * x - s * y; q12 = s * x + c * y;
        x = q21; y = q22; q21 = c * x - s * y; q22 = s * x + c * y;
    };
    while (end > 0) {
        if (start <= 0 && 0 < end)
            if (fabsf(e0) <= (fabsf(d0) + fabsf(d1)) * precision || fabsf(e0) <= tiny) e0 = 0.f;
        if (start <= 1 && 1 < end)
            if (fabsf(e1) <= (fabsf(d1) + fabsf(d2)) * precision || fabsf(e1) <= tiny) e1 = 0.f;
        while (end > 0 && (end == 2 ? e1 : e0) == 0.f) end--;
        if (end <= 0) break;
        iter++;
        if (iter > 90) { converged = false; break; }
        start = end - 1;
        while (start > 0 && (start == 1 ? e0 : 0.f) != 0.f) start--;
        // tridiagonal_qr_step(start, end)
        float dem1 = end == 2 ? d1 : d0, de = end == 2 ? d2 : d1, ee = end == 2 ? e1 : e0;
        float td = (dem1 - de) * 0.5f;
        float mu = de;
        if (td == 0.f) {
            mu -= fabsf(ee);
        } else {
            float e2 = ee * ee;
            float h = eig_hypot(td, ee);
            if (e2 == 0.f) mu -= (ee / (td + (td > 0.f ? 1.f : -1.f))) * (ee / h);
            else mu -= e2 / (td + (td > 0.f ? h : -h));
        }
        float x = (start == 0 ? d0 : d1) - mu;
        float z = start == 0 ? e0 : e1;
        for (int k = start; k < end; ++k) {
            float c, s;
            make_givens(x, z, c, s);
            float dk = k == 0 ? d0 : d1, dk1 = k == 0 ? d1 : d2, sk = k == 0 ? e0 : e1;
            float sdk = s * dk + c * sk;
            float dkp1 = s * sk + c * dk1;
            float ndk = c * (c * dk - s * sk) - s * (c * sk - s * dk1);
            float ndk1 = s * sdk + c * dkp1;
            float nsk = c * sdk - s * dkp1;
            if (k == 0) { d0 = ndk; d1 = ndk1; e0 = nsk; }
            else { d1 = ndk; d2 = ndk1; e1 = nsk; }
            if (k > start) e0 = c * e0 - s * z;  // k == 1, start == 0: sub[k-1] = sub[0]
            x = nsk;
            if (k < end - 1) {  // k == 0, end == 2
                z = -s * e1;
                e1 = c * e1;
            }
            if (k == 0) rot_cols01(c, s);
            else rot_cols12(c, s);
        }
    }
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
// ---- end of the unchanged text ----
#undef __device__
#undef __forceinline__
}  // namespace branching

namespace {

struct Counts {
    std::uint64_t finite_cases = 0, finite_differ = 0, nonfinite_cases = 0, nonfinite_differ = 0, nan_results = 0, not_diagonal = 0,
                  tied = 0, cap_failures = 0;
};

std::mt19937_64 rng(20260117u);
float uniform(float a, float b) { return a + (b - a) * static_cast<float>(rng() >> 40) * 0x1p-24f; }
std::uint32_t bits(float f)
{
    std::uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

// a = {a00, a10, a20, a11, a21, a22}
void check(const float* a, bool finite, Counts& n)
{
    float want[9], got[9];
    branching::eig3_smallest<true>(a[0], a[1], a[2], a[3], a[4], a[5], want, want + 3, want + 6);
    pcpx::eig3_smallest<true>(a[0], a[1], a[2], a[3], a[4], a[5], got, got + 3, got + 6);
    float plain[6];  // the default form gives the same normal and eigenvalues
    pcpx::eig3_smallest(a[0], a[1], a[2], a[3], a[4], a[5], plain, plain + 3);
    bool differ = false;
    for (int i = 0; i < 9; ++i) {
        const bool same = finite ? bits(want[i]) == bits(got[i]) : std::isnan(want[i]) ? std::isnan(got[i]) : bits(want[i]) == bits(got[i]);
        if (!same) differ = true;
        if (i < 6 && !(std::isnan(got[i]) ? std::isnan(plain[i]) : bits(got[i]) == bits(plain[i]))) differ = true;
        if (std::isnan(want[i])) ++n.nan_results;
    }
    if (a[1] != 0.f || a[2] != 0.f || a[4] != 0.f) ++n.not_diagonal;
    if (want[3] == want[4] || want[4] == want[5]) ++n.tied;
    ++(finite ? n.finite_cases : n.nonfinite_cases);
    if (differ) {
        if (++(finite ? n.finite_differ : n.nonfinite_differ) <= 10) {
            std::printf("differs: a (%a %a %a %a %a %a)\n  want", a[0], a[1], a[2], a[3], a[4], a[5]);
            for (float v : want) std::printf(" %a", v);
            std::printf("\n  got ");
            for (float v : got) std::printf(" %a", v);
            std::printf("\n");
        }
    }
}

// the scatter matrix of k points as the kernels form it: mean = sum / k, then sums of products of the centred coordinates
void scatter(const float (*p)[3], int k, float* a)
{
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int i = 0; i < k; ++i) {
        sx += p[i][0];
        sy += p[i][1];
        sz += p[i][2];
    }
    const float fn = static_cast<float>(k), mx = sx / fn, my = sy / fn, mz = sz / fn;
    float c00 = 0.f, c10 = 0.f, c11 = 0.f, c20 = 0.f, c21 = 0.f, c22 = 0.f;
    for (int i = 0; i < k; ++i) {
        const float vx = p[i][0] - mx, vy = p[i][1] - my, vz = p[i][2] - mz;
        c00 += vx * vx;
        c10 += vy * vx;
        c11 += vy * vy;
        c20 += vz * vx;
        c21 += vz * vy;
        c22 += vz * vz;
    }
    a[0] = c00; a[1] = c10; a[2] = c20; a[3] = c11; a[4] = c21; a[5] = c22;
}

enum Kind { FREE, PLANAR, COLLINEAR, LATTICE, COINCIDENT, KINDS };

void point_sets(int sets, Counts& n)
{
    for (int i = 0; i < sets; ++i) {
        const int k = 3 + static_cast<int>(rng() % 30u);  // 3 ... 32
        const int kind = static_cast<int>(rng() % KINDS);
        const float scale = std::ldexp(1.f, static_cast<int>(rng() % 41u) - 20);  // 2^-20 ... 2^20
        const std::uint64_t far = rng() % 4u;
        const float reach = far == 0 ? 0.f : far == 1 ? 1.f : far == 2 ? 30.f : 1000.f;
        float o[3], u[3], v[3];
        for (int a = 0; a < 3; ++a) {
            o[a] = uniform(-1.f, 1.f) * reach;
            u[a] = uniform(-1.f, 1.f);
            v[a] = uniform(-1.f, 1.f);
        }
        if (rng() % 4u == 0) u[rng() % 3u] = 0.f;  // axis-aligned planes and lines
        if (rng() % 4u == 0) v[rng() % 3u] = 0.f;
        float p[32][3];
        for (int j = 0; j < k; ++j) {
            const float s = uniform(-1.f, 1.f), t = uniform(-1.f, 1.f);
            for (int a = 0; a < 3; ++a) {
                float c;
                switch (kind) {
                case FREE: c = uniform(-1.f, 1.f); break;
                case PLANAR: c = s * u[a] + t * v[a]; break;
                case COLLINEAR: c = s * u[a]; break;
                case LATTICE: c = static_cast<float>(static_cast<int>(rng() % 5u) - 2); break;
                default: c = 0.f; break;
                }
                p[j][a] = o[a] + c * scale;
            }
        }
        float a[6];
        scatter(p, k, a);
        check(a, true, n);
    }
}

float raw_entry()
{
    const float sign = rng() & 1u ? -1.f : 1.f;
    switch (rng() % 6u) {
    case 0: return 0.f;
    case 1: return sign * 0x1p-140f;
    case 2: return sign * 0x1p100f;
    case 3: return sign * uniform(0.f, 1.f);
    default: return sign * std::ldexp(uniform(0.5f, 1.f), static_cast<int>(rng() % 277u) - 149);  // 2^-150 ... 2^127
    }
}

void raw_matrices(int count, bool finite, Counts& n)
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (int i = 0; i < count; ++i) {
        float a[6];
        const std::uint64_t form = rng() % 4u;
        const float common = raw_entry();
        for (float& e : a) e = form == 0 ? common * uniform(0.5f, 1.f) : raw_entry();  // form 0: entries of one magnitude
        if (form == 1) a[2] = 0.f;                                                       // already tridiagonal
        if (form == 2) a[1] = a[2] = 0.f;                                                // a 2x2 block
        if (!finite) {
            const int bad = 1 + static_cast<int>(rng() % 2u);
            for (int b = 0; b < bad; ++b) a[rng() % 6u] = rng() % 3u == 0 ? nan : rng() & 1u ? inf : -inf;
        }
        check(a, finite, n);
    }
}

// the per-lane cap: with 90 trips counted, a state that is not deflated stops where it is; with none counted, it converges
void trip_cap(Counts& n)
{
    const pcpx::Ql3 in = {1.f, 2.f, 3.f, 0.5f, 0.25f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    pcpx::Ql3 m = in;
    if (pcpx::ql3_iterate(m, pcpx::QL3_MAX_TRIPS) || std::memcmp(&m, &in, sizeof m) != 0) ++n.cap_failures;
    m = in;
    if (pcpx::ql3_iterate(m, pcpx::QL3_MAX_TRIPS - 1) || std::memcmp(&m, &in, sizeof m) == 0 || m.e0 == 0.f || m.e1 == 0.f) ++n.cap_failures;  // one trip, then the cap
    m = in;
    if (!pcpx::ql3_iterate(m) || m.e0 != 0.f || m.e1 != 0.f) ++n.cap_failures;
    m = in;
    m.e0 = 0x1p-30f;  // deflated in the trip that would have been the 91st: converged, nothing rotated
    m.e1 = 0.f;
    if (!pcpx::ql3_iterate(m, pcpx::QL3_MAX_TRIPS) || m.e0 != 0.f || m.d0 != in.d0 || m.d1 != in.d1 || m.d2 != in.d2 || m.q00 != 1.f) ++n.cap_failures;
}

}  // namespace

int main()
{
    Counts n;
    point_sets(1500000, n);
    raw_matrices(700000, true, n);
    raw_matrices(200000, false, n);
    trip_cap(n);
    std::printf("{\"finite_cases\": %" PRIu64 ", \"finite_differ\": %" PRIu64 ", \"nonfinite_cases\": %" PRIu64 ", \"nonfinite_differ\": %" PRIu64
                ", \"nan_results\": %" PRIu64 ", \"not_diagonal\": %" PRIu64 ", \"tied_eigenvalues\": %" PRIu64 ", \"cap_failures\": %" PRIu64 "}\n",
                n.finite_cases, n.finite_differ, n.nonfinite_cases, n.nonfinite_differ, n.nan_results, n.not_diagonal, n.tied, n.cap_failures);
    const bool ok = n.finite_differ == 0 && n.nonfinite_differ == 0 && n.cap_failures == 0 && n.finite_cases >= 2000000u && n.nan_results > 0 &&
                    n.not_diagonal > 0 && n.tied > 0;
    return ok ? 0 : 1;
}
