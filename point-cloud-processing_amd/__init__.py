"""pcp-mi355x: MI355X-native kNN / radius search / PCA normals behind the `pcp` API.

The compute path is libpcpx.so (hand-written HIP for gfx950, C ABI in include/pcpx.h); importing the
package does not load it, using any compute entry point does and fails loudly if it is missing.
"""
from . import match, objects, planes, ply, register, shapes, simplify, surface, synthetic, voxel  # noqa: F401
from ._capi import Grid3d  # noqa: F401
from .match import match_correspondences, match_correspondences_dev, match_nearest, match_nearest_dev, match_plan  # noqa: F401
from .objects import label_objects, label_objects_dev, objects_plan  # noqa: F401
from .planes import extract_planes, extract_planes_dev, plane_fit, plane_fit_dev, plane_plan, ransac_plane, ransac_plane_dev  # noqa: F401
from .register import ransac_plan, ransac_rigid, ransac_rigid_dev, rigid_fit, rigid_fit_dev  # noqa: F401
from .shapes import (cylinder_fit, ransac_cylinder, ransac_shape_dev, ransac_sphere, shape_fit_dev, shape_params, shape_plan,  # noqa: F401
                     sphere_fit)
from .simplify import hierarchy_simplification, hierarchy_simplification_dev  # noqa: F401
from .surface import regular_grid_containing, surface_nets, surface_nets_from_hint  # noqa: F401
from .voxel import voxel_grid, voxel_grid_dev, voxel_plan  # noqa: F401
from .filters import bilateral_filter_normals, bilateral_filter_points, wlop  # noqa: F401
from .index import (Index, KdTreeK, LinkedKdTree, LinkedOctree, PcpxError, bounding_box, device_count,  # noqa: F401
                    estimate_normal, estimate_normals, estimate_normals_batch, propagate_normal_orientations, propagate_normal_orientations_dev, shard_range, shard_cuts_by_cost)

__all__ = ["Index", "LinkedOctree", "LinkedKdTree", "KdTreeK", "PcpxError", "bounding_box", "device_count", "estimate_normal",
           "estimate_normals", "estimate_normals_batch", "propagate_normal_orientations", "propagate_normal_orientations_dev", "shard_range", "shard_cuts_by_cost", "ply", "synthetic",
           "bilateral_filter_points", "bilateral_filter_normals", "wlop",
           "Grid3d", "regular_grid_containing", "surface_nets", "surface_nets_from_hint", "surface",
           "hierarchy_simplification", "hierarchy_simplification_dev", "simplify",
           "match", "match_nearest", "match_nearest_dev", "match_correspondences", "match_correspondences_dev", "match_plan",
           "register", "ransac_plan", "ransac_rigid", "ransac_rigid_dev", "rigid_fit", "rigid_fit_dev",
           "planes", "plane_plan", "ransac_plane", "ransac_plane_dev", "plane_fit", "plane_fit_dev", "extract_planes", "extract_planes_dev",
           "voxel", "voxel_grid", "voxel_grid_dev", "voxel_plan",
           "objects", "label_objects", "label_objects_dev", "objects_plan",
           "shapes", "shape_params", "shape_plan", "ransac_sphere", "ransac_cylinder", "ransac_shape_dev", "sphere_fit", "cylinder_fit", "shape_fit_dev"]
