// pcp::common::regular_grid3d_t / regular_grid_containing (include/pcp/common/regular_grid3d.hpp of the reference): a
// box of sx x sy x sz voxels of size (dx, dy, dz) from the corner (x, y, z).  The layout matches pcpx_grid3d for Scalar = float.
#ifndef PCP_COMMON_REGULAR_GRID3D_HPP
#define PCP_COMMON_REGULAR_GRID3D_HPP

#include <array>
#include <cstddef>

namespace pcp {
namespace common {

template <class Scalar>
struct regular_grid3d_t
{
    using scalar_type = Scalar;

    // origin of the grid
    scalar_type x = static_cast<scalar_type>(0), y = static_cast<scalar_type>(0), z = static_cast<scalar_type>(0);
    // voxel size in x, y, z
    scalar_type dx = static_cast<scalar_type>(0), dy = static_cast<scalar_type>(0), dz = static_cast<scalar_type>(0);
    // number of voxels in x, y, z from the origin
    std::size_t sx = 0, sy = 0, sz = 0;
};

// A grid of dimensions + 2 voxels per axis around [min, max].  As in the reference the origin moves back by dx on EVERY
// axis (grid.y -= grid.dx, grid.z -= grid.dx): kept, since meshes depend on it.
template <class PointView, class Scalar = float>
regular_grid3d_t<Scalar> regular_grid_containing(PointView const& min, PointView const& max, std::array<std::size_t, 3> dimensions)
{
    regular_grid3d_t<Scalar> grid;
    grid.x  = min.x();
    grid.y  = min.y();
    grid.z  = min.z();
    grid.sx = dimensions[0];
    grid.sy = dimensions[1];
    grid.sz = dimensions[2];
    grid.dx = (max.x() - min.x()) / static_cast<Scalar>(grid.sx);
    grid.dy = (max.y() - min.y()) / static_cast<Scalar>(grid.sy);
    grid.dz = (max.z() - min.z()) / static_cast<Scalar>(grid.sz);
    grid.x -= grid.dx;
    grid.y -= grid.dx;
    grid.z -= grid.dx;
    grid.sx += 2;
    grid.sy += 2;
    grid.sz += 2;
    return grid;
}

} // namespace common
} // namespace pcp

#endif
