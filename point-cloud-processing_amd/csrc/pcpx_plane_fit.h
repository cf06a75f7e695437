// pcpx_plane_fit.h -- the least-squares plane of a point set from its centroid and the six terms of its scatter matrix about the
// centroid (include/pcpx_planes.h, PLANE FIT): the unit eigenvector of the smallest eigenvalue, by the cyclic Jacobi sweeps of
// pcpx_horn.h on the symmetric 3 x 3 matrix.  float64, one thread; every index is a compile-time constant after unrolling.  Host and
// device: tests/test_planes_cpu.py compiles it for the host against numpy.linalg.eigh.
#ifndef PCPX_PLANE_FIT_H
#define PCPX_PLANE_FIT_H

#include "pcpx_horn.h"

namespace pcpx {

// s: the scatter's terms xx, xy, xz, yy, yz, zz.  n: the unit eigenvector of the smallest eigenvalue (the first of equal ones), its
// component of largest magnitude positive (the lowest index on ties); (0, 0, 1) where nothing can be normalised (a NaN in s).
// lambda: the three eigenvalues in the order the sweeps leave them on the diagonal (optional).
PCPX_HORN_FN void plane_normal_of_scatter(const double (&s)[6], double (&n)[3], double* lambda = nullptr)
{
    double a[3][3] = {{s[0], s[1], s[2]}, {s[1], s[3], s[4]}, {s[2], s[4], s[5]}};
    double v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < HORN_MAX_SWEEPS; ++sweep) {
        const double off = std::fabs(a[0][1]) + std::fabs(a[0][2]) + std::fabs(a[1][2]);
        if (!(off > 0.0)) break;  // (also for a NaN: nothing more can be done)
        jacobi_rotate<3, 0, 1>(a, v);
        jacobi_rotate<3, 0, 2>(a, v);
        jacobi_rotate<3, 1, 2>(a, v);
    }
    double best = a[0][0], x = v[0][0], y = v[1][0], z = v[2][0];
#pragma unroll
    for (int j = 1; j < 3; ++j) {
        const bool take = a[j][j] < best;
        best = take ? a[j][j] : best;
        x = take ? v[0][j] : x;
        y = take ? v[1][j] : y;
        z = take ? v[2][j] : z;
    }
    const double norm = std::sqrt((x * x + y * y) + z * z);
    if (!(norm > 0.0)) {
        x = 0.0, y = 0.0, z = 1.0;
    } else {
        x /= norm, y /= norm, z /= norm;
    }
    // the sign: the component of largest magnitude is positive, the lowest index on ties
    double big = x;
    if (std::fabs(y) > std::fabs(big)) big = y;
    if (std::fabs(z) > std::fabs(big)) big = z;
    if (big < 0.0) x = -x, y = -y, z = -z;
    n[0] = x, n[1] = y, n[2] = z;
    if (lambda) lambda[0] = a[0][0], lambda[1] = a[1][1], lambda[2] = a[2][2];
}

}  // namespace pcpx

#endif
