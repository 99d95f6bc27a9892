"""raytracer_2022_amd — MI355X-native path-tracing hot loop of Jerx2y/Raytracer-2022.

The product is `librt2022.so` (hand-written HIP kernels for gfx950 behind the C ABI
of include/rt2022.h, plus the C++ host mirror of the reference's scene-builder
API). This package is the thin Python plumbing over it: ctypes bindings, numpy /
torch buffer handling. Nothing here computes pixels.
"""
from . import _ffi
from ._ffi import RtError, lib, make_ref, ref_index, ref_kind  # noqa: F401
from .host import (DescBuilder, HostScene, camera_new, fill_image, load_image, make_params, shuffled_rows,  # noqa: F401
                   write_color, write_jpeg)
from .device import (DUAL_DEFAULTS, DeviceScene, DeviceSceneSet, denoise, denoise_device, denoise_dual, denoise_dual_device,  # noqa: F401
                     denoise_dual_params, denoise_dual_workspace_bytes, denoise_params, denoise_workspace_bytes, query_rays,
                     radiance_params, radiance_rays, two_frame_rows)
from .device import adaptive_merge_features_device, adaptive_resolve_features_device  # noqa: F401
from .device import (ADAPTIVE_LUMA_FLOOR, adaptive_merge_device, adaptive_params, adaptive_plan, adaptive_plan_device,  # noqa: F401
                     adaptive_resolve_device, adaptive_scale, adaptive_workspace_bytes, pixel_ids, plan_units, render_adaptive)
from .device import TEMPORAL_DEFAULTS, temporal, temporal_device, temporal_params, temporal_workspace_bytes  # noqa: F401
from ._ffi import FEATURE_DTYPE, HIT_DTYPE, QUERY_RAY_DTYPE, RADIANCE_RAY_DTYPE, TEMPORAL_PIXEL_DTYPE  # noqa: F401
from ._ffi import BVH_NODE_DTYPE  # noqa: F401
from .host import rebuild_bvh, ref_boxes, tree_leaves  # noqa: F401
from .device import bvh_build, bvh_build_device, bvh_workspace_bytes  # noqa: F401
from .device import (RAY_ORDER_DEFAULTS, intersect_ordered_workspace_bytes, ray_order, ray_order_device, ray_order_params,  # noqa: F401
                     ray_order_workspace_bytes)
from .device import path_key, radiance_by_steps, scatter_params, unwind  # noqa: F401
from ._ffi import SCATTER_REC_DTYPE  # noqa: F401

__all__ = ["DescBuilder", "HostScene", "DeviceScene", "DeviceSceneSet", "camera_new", "fill_image", "make_params", "shuffled_rows",
           "write_color", "write_jpeg", "load_image", "RtError", "lib", "make_ref", "ref_kind", "ref_index", "query_rays",
           "QUERY_RAY_DTYPE", "HIT_DTYPE", "radiance_rays", "radiance_params", "RADIANCE_RAY_DTYPE", "FEATURE_DTYPE",
           "denoise", "denoise_device", "denoise_params", "denoise_workspace_bytes", "denoise_dual", "denoise_dual_device",
           "denoise_dual_params", "denoise_dual_workspace_bytes", "two_frame_rows", "DUAL_DEFAULTS",
           "pixel_ids", "adaptive_params", "adaptive_workspace_bytes", "adaptive_plan", "adaptive_plan_device", "adaptive_merge_device",
           "adaptive_resolve_device", "adaptive_scale", "plan_units", "render_adaptive", "ADAPTIVE_LUMA_FLOOR",
           "adaptive_merge_features_device", "adaptive_resolve_features_device",
           "temporal", "temporal_device", "temporal_params", "temporal_workspace_bytes", "TEMPORAL_DEFAULTS", "TEMPORAL_PIXEL_DTYPE",
           "ref_boxes", "rebuild_bvh", "tree_leaves", "bvh_build", "bvh_build_device", "bvh_workspace_bytes", "BVH_NODE_DTYPE",
           "ray_order", "ray_order_device", "ray_order_params", "ray_order_workspace_bytes", "intersect_ordered_workspace_bytes",
           "RAY_ORDER_DEFAULTS", "scatter_params", "unwind", "radiance_by_steps", "path_key", "SCATTER_REC_DTYPE"]
