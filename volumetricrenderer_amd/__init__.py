"""volumetricrenderer_amd -- MI355X-native volumetric ray-march integrator.

The hot path of Raspy-Py/VolumetricRenderer (shaders/frag.glsl), re-built as
hand-written HIP kernels for gfx950 behind a C ABI (include/vr.h, libvr.so).
This package is the Python host side: ctypes bindings (_lib), the renderer
interface (renderer) and the multi-GPU band sharding (distributed).
"""
from ._lib import (FMT_R8_SRGB, FMT_R8_UNORM, FMT_R32F, FMT_RGBA8_SRGB, FMT_RGBA8_UNORM, FMT_RGBA32F,  # noqa: F401
                   GREY_OF, GlobalShaderData, MarchParams, ObjectShaderData, Target, VolumeRecipe, VRError)
from ._lib import VR_MAX_RECTS, Procedural, RayRecord, Rect  # noqa: F401
from ._lib import BLUR_MAX_HALF, BRUSH_ADD, BRUSH_MAX_RADIUS, BRUSH_SET, BRUSH_SUB, VR_MAX_DABS, Box, Brush  # noqa: F401
from ._lib import VOLUME_STATS_BYTES, StatsSummary, VolumeStats  # noqa: F401
from .renderer import Stats, Summary, box_stats_host, brush_stats_host, stats_summary, unpack_stats  # noqa: F401
from ._lib import MORPH_DILATE, MORPH_ERODE, MORPH_MAX_HALF  # noqa: F401
from .renderer import brush_morph_apply  # noqa: F401
from ._lib import RANK_MAX_HALF, RANK_MEDIAN  # noqa: F401
from .renderer import brush_rank_apply  # noqa: F401
from ._lib import FILL_REPORT_BYTES, FillReport, FillRule  # noqa: F401
from .renderer import Fill, brush_fill_apply, make_fill_rule, unpack_fill_report  # noqa: F401
from ._lib import CloneMap  # noqa: F401
from .renderer import brush_clone_apply, brush_stamp_apply, make_clone_map, stamp_box  # noqa: F401
from ._lib import AFFINE_MAX_COEFF, AFFINE_ONE, BORDER_CLAMP, BORDER_SKIP, FILTER_LINEAR, FILTER_NEAREST, Affine  # noqa: F401
from .renderer import (affine_direct, affine_identity, affine_place, brush_clone_affine_apply,  # noqa: F401
                       brush_stamp_affine_apply, make_affine)
from ._lib import WARP_MAX_DISP  # noqa: F401
from .renderer import brush_warp_apply, warp_push, warp_reach  # noqa: F401
from ._lib import LUT_BYTES, LUT_EQUALIZE, LUT_STRETCH, Lut  # noqa: F401
from .renderer import brush_remap_apply, lut_compose, lut_identity, lut_levels, stats_lut  # noqa: F401
from .renderer import brush_apply, brush_blur_apply, brush_box, brush_line, coalesce_boxes, make_brush  # noqa: F401
from .renderer import (RAY_RECORD_DTYPE, Renderer, band_rows_packed, coalesce_rects, march_defaults,  # noqa: F401
                       procedural_defaults, ray_records, reference_shader_data, scaled_recipe, shader_data_arrays,
                       volume_box_footprint,
                       volume_recipe_defaults)

__all__ = [
    "Renderer", "VRError", "march_defaults", "procedural_defaults", "Procedural", "reference_shader_data", "volume_recipe_defaults",
    "scaled_recipe", "band_rows_packed", "shader_data_arrays", "FMT_RGBA32F", "FMT_RGBA8_UNORM",
    "FMT_RGBA8_SRGB", "FMT_R8_UNORM", "FMT_R8_SRGB", "FMT_R32F", "GREY_OF", "ObjectShaderData", "GlobalShaderData", "MarchParams", "VolumeRecipe", "Target",
    "Rect", "volume_box_footprint", "coalesce_rects", "VR_MAX_RECTS", "RayRecord", "RAY_RECORD_DTYPE", "ray_records",
    "Brush", "BRUSH_SET", "BRUSH_ADD", "BRUSH_SUB", "BRUSH_MAX_RADIUS", "make_brush", "brush_box", "brush_apply",
    "brush_line", "coalesce_boxes", "VR_MAX_DABS", "Box", "brush_blur_apply", "BLUR_MAX_HALF",
    "brush_morph_apply", "MORPH_ERODE", "MORPH_DILATE", "MORPH_MAX_HALF",
    "brush_rank_apply", "RANK_MEDIAN", "RANK_MAX_HALF",
    "FillRule", "FillReport", "FILL_REPORT_BYTES", "Fill", "make_fill_rule", "brush_fill_apply", "unpack_fill_report",
    "CloneMap", "make_clone_map", "brush_clone_apply", "brush_stamp_apply", "stamp_box",
    "Affine", "FILTER_NEAREST", "FILTER_LINEAR", "BORDER_CLAMP", "BORDER_SKIP", "AFFINE_ONE", "AFFINE_MAX_COEFF",
    "make_affine", "affine_identity", "affine_place", "affine_direct", "brush_stamp_affine_apply",
    "brush_clone_affine_apply",
    "WARP_MAX_DISP", "brush_warp_apply", "warp_reach", "warp_push",
    "Lut", "LUT_BYTES", "LUT_EQUALIZE", "LUT_STRETCH", "lut_identity", "lut_levels", "lut_compose", "stats_lut",
    "brush_remap_apply",
    "VolumeStats", "StatsSummary", "VOLUME_STATS_BYTES", "Stats", "Summary", "brush_stats_host", "box_stats_host",
    "stats_summary", "unpack_stats",
]
