// pcpx_horn.h -- the rotation that maximises sum (R p) . q for centred point pairs, from their 3 x 3 correlation matrix
// H = sum p q^T, by Horn's closed form (B. K. P. Horn, "Closed-form solution of absolute orientation using unit quaternions",
// JOSA A 4(4), 1987): the unit quaternion is the eigenvector of the largest eigenvalue of a symmetric 4 x 4 matrix of H's entries,
// found here by cyclic Jacobi sweeps.  float64, one thread; every index is a compile-time constant after unrolling, so the
// matrices live in registers.  Host and device: tests/test_register_cpu.py compiles it for the host against an SVD.
#ifndef PCPX_HORN_H
#define PCPX_HORN_H

#include <cmath>

#if defined(__HIPCC__)
#define PCPX_HORN_FN __host__ __device__ inline
#else
#define PCPX_HORN_FN inline
#endif

namespace pcpx {

constexpr int HORN_MAX_SWEEPS = 64;  // (convergence is quadratic: a dozen sweeps at the most in practice)

// one Jacobi rotation in the plane (P, Q) of the symmetric N x N a, accumulated into the eigenvector columns of v (N = 4: Horn's
// matrix below; N = 3: the scatter matrix of pcpx_plane_fit.h)
template <int N, int P, int Q>
PCPX_HORN_FN void jacobi_rotate(double (&a)[N][N], double (&v)[N][N])
{
    const double apq = a[P][Q];
    if (apq == 0.0) return;
    // an entry that no longer changes either diagonal neighbour in float64 is zero
    if (std::fabs(a[P][P]) + std::fabs(apq) == std::fabs(a[P][P]) && std::fabs(a[Q][Q]) + std::fabs(apq) == std::fabs(a[Q][Q])) {
        a[P][Q] = a[Q][P] = 0.0;
        return;
    }
    const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
    const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
#pragma unroll
    for (int k = 0; k < N; ++k) {  // a <- a J, v <- v J with J[P][P] = J[Q][Q] = c, J[P][Q] = s, J[Q][P] = -s
        const double akp = a[k][P], akq = a[k][Q];
        a[k][P] = c * akp - s * akq;
        a[k][Q] = s * akp + c * akq;
        const double vkp = v[k][P], vkq = v[k][Q];
        v[k][P] = c * vkp - s * vkq;
        v[k][Q] = s * vkp + c * vkq;
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {  // a <- J^T a
        const double apk = a[P][k], aqk = a[Q][k];
        a[P][k] = c * apk - s * aqk;
        a[Q][k] = s * apk + c * aqk;
    }
    a[P][Q] = a[Q][P] = 0.0;
}
template <int P, int Q>
PCPX_HORN_FN void horn_rotate(double (&a)[4][4], double (&v)[4][4])
{
    jacobi_rotate<4, P, Q>(a, v);
}

// the rotation matrix, row-major, of the unit quaternion (qw, qx, qy, qz)
PCPX_HORN_FN void horn_quaternion_matrix(double qw, double qx, double qy, double qz, double (&r)[9])
{
    r[0] = 1.0 - 2.0 * (qy * qy + qz * qz);
    r[1] = 2.0 * (qx * qy - qw * qz);
    r[2] = 2.0 * (qx * qz + qw * qy);
    r[3] = 2.0 * (qx * qy + qw * qz);
    r[4] = 1.0 - 2.0 * (qx * qx + qz * qz);
    r[5] = 2.0 * (qy * qz - qw * qx);
    r[6] = 2.0 * (qx * qz - qw * qy);
    r[7] = 2.0 * (qy * qz + qw * qx);
    r[8] = 1.0 - 2.0 * (qx * qx + qy * qy);
}

// h: H row-major, H[a][b] = sum p_a q_b.  r: the rotation, row-major.  Always a proper rotation (it is a unit quaternion's matrix);
// the identity for H = 0.
PCPX_HORN_FN void horn_rotation(const double (&h)[9], double (&r)[9])
{
    const double sxx = h[0], sxy = h[1], sxz = h[2], syx = h[3], syy = h[4], syz = h[5], szx = h[6], szy = h[7], szz = h[8];
    double a[4][4] = {{sxx + syy + szz, syz - szy, szx - sxz, sxy - syx},
                      {syz - szy, sxx - syy - szz, sxy + syx, szx + sxz},
                      {szx - sxz, sxy + syx, -sxx + syy - szz, syz + szy},
                      {sxy - syx, szx + sxz, syz + szy, -sxx - syy + szz}};
    double v[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    for (int sweep = 0; sweep < HORN_MAX_SWEEPS; ++sweep) {
        const double off = std::fabs(a[0][1]) + std::fabs(a[0][2]) + std::fabs(a[0][3]) + std::fabs(a[1][2]) + std::fabs(a[1][3]) + std::fabs(a[2][3]);
        if (!(off > 0.0)) break;  // (also for a NaN: nothing more can be done)
        horn_rotate<0, 1>(a, v);
        horn_rotate<0, 2>(a, v);
        horn_rotate<0, 3>(a, v);
        horn_rotate<1, 2>(a, v);
        horn_rotate<1, 3>(a, v);
        horn_rotate<2, 3>(a, v);
    }
    // the column of the largest eigenvalue (the first of equal ones), by selection rather than by a run-time index
    double best = a[0][0], qw = v[0][0], qx = v[1][0], qy = v[2][0], qz = v[3][0];
#pragma unroll
    for (int j = 1; j < 4; ++j) {
        const bool take = a[j][j] > best;
        best = take ? a[j][j] : best;
        qw = take ? v[0][j] : qw;
        qx = take ? v[1][j] : qx;
        qy = take ? v[2][j] : qy;
        qz = take ? v[3][j] : qz;
    }
    const double norm = std::sqrt((qw * qw + qx * qx) + (qy * qy + qz * qz));
    if (!(norm > 0.0)) {  // (a NaN in H)
        qw = 1.0, qx = qy = qz = 0.0;
    } else {
        qw /= norm, qx /= norm, qy /= norm, qz /= norm;
    }
    horn_quaternion_matrix(qw, qx, qy, qz, r);
}

}  // namespace pcpx

#endif
