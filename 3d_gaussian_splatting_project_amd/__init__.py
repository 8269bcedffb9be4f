"""MI355X-native Gaussian-splat majority-vote labeler + rasterizer (host side of libgsx.so).

The directory name starts with a digit, so import it with
    importlib.import_module("3d_gaussian_splatting_project_amd")
"""
from . import _lib
from ._lib import Camera, GsxError, build, lib
from . import dist, scene
from .labeler import Context, assign_labels_from_maps, bind_to_gpu_numa_node, camera_array, load_cameras, project_gaussian, region_grow
from .labeler import assign_instances_from_maps, assoc_constants
from .labeler import debug_nn_grid
from .labeler import iou_best, iou_constants, iou_from_counts, iou_from_table
from .labeler import DepthFrame, depth_constants, depth_key_to_z, depth_maps
from .labeler import label_maps_from_labels, labelmap_constants
from .labeler import lift_constants, queries_constants, segmap_constants, segpack_constants, smooth_constants

__all__ = ["Camera", "Context", "DepthFrame", "GsxError", "assign_instances_from_maps", "assign_labels_from_maps", "assoc_constants", "bind_to_gpu_numa_node", "build", "camera_array", "debug_nn_grid", "depth_constants", "depth_key_to_z", "depth_maps", "dist", "iou_best", "iou_constants", "iou_from_counts", "iou_from_table", "label_maps_from_labels", "labelmap_constants", "lib", "lift_constants", "load_cameras",
           "project_gaussian", "queries_constants", "region_grow", "scene", "segmap_constants", "segpack_constants", "smooth_constants"]
