// pcpx_plane_solve.h -- the one-thread part of the point-to-plane step of include/pcpx_icp.h: the 6 x 6 normal equations by
// Cholesky, and the pose update T <- [dR R, dR (t - o) + o + tau] with dR the rotation of the unit quaternion (1, w/2) / |(1, w/2)|.
// float64; every index is a compile-time constant after unrolling.  Host and device, as pcpx_horn.h: tests/test_icp_cpu.py compiles
// it for the host against numpy.linalg.solve.
#ifndef PCPX_PLANE_SOLVE_H
#define PCPX_PLANE_SOLVE_H

#include "pcpx_horn.h"

#include <limits>

namespace pcpx {

constexpr int PLANE_A_TERMS = 21, PLANE_B_TERMS = 6;
constexpr double PLANE_PIVOT_FLOOR = 1.0 / 1099511627776.0;  // 2^-40 of the pivot's own original diagonal entry

// where entry (r, c), r <= c, of the symmetric 6 x 6 matrix sits among the 21 of its upper triangle, row by row
constexpr int plane_at(int r, int c) { return r * 6 - r * (r - 1) / 2 + (c - r); }

// a: the upper triangle of A, b: the right-hand side.  false when a pivot is not finite or too small (x is then not written).
PCPX_HORN_FN bool plane_cholesky(const double (&a)[PLANE_A_TERMS], const double (&b)[PLANE_B_TERMS], double (&x)[6])
{
    double l[6][6];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = a[plane_at(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= l[j][k] * l[j][k];
        // (false for a NaN pivot; an infinite one fails the second test)
        ok = ok && d > PLANE_PIVOT_FLOOR * a[plane_at(j, j)] && d < std::numeric_limits<double>::infinity();
        const double root = std::sqrt(d);
        l[j][j] = root;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double v = a[plane_at(j, i)];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= l[i][k] * l[j][k];
            l[i][j] = v / root;
        }
    }
    if (!ok) return false;
    double z[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double v = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) v -= l[i][k] * z[k];
        z[i] = v / l[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double v = z[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) v -= l[k][i] * x[k];
        x[i] = v / l[i][i];
    }
    return true;
}

// t: the pose, 16 doubles row-major; o: the centre of rotation; x = (w, tau).  out may not alias t.
PCPX_HORN_FN void plane_compose(const double* t, const double (&o)[3], const double (&x)[6], double* out)
{
    const double qx = x[0] / 2.0, qy = x[1] / 2.0, qz = x[2] / 2.0;
    const double norm = std::sqrt((1.0 + qx * qx) + (qy * qy + qz * qz));
    double dr[9];
    horn_quaternion_matrix(1.0 / norm, qx / norm, qy / norm, qz / norm, dr);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) out[4 * r + c] = (dr[3 * r] * t[c] + dr[3 * r + 1] * t[4 + c]) + dr[3 * r + 2] * t[8 + c];
        out[4 * r + 3] = (((dr[3 * r] * (t[3] - o[0]) + dr[3 * r + 1] * (t[7] - o[1])) + dr[3 * r + 2] * (t[11] - o[2])) + o[r]) + x[3 + r];
    }
    out[12] = out[13] = out[14] = 0.0;
    out[15] = 1.0;
}

}  // namespace pcpx

#endif
