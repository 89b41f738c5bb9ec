"""Host-side interface of the ray-march path, over the C ABI (include/vr.h).

This mirrors the part of the reference interface that feeds shaders/frag.glsl:

==========================================  =====================================
reference (file:line)                       here
==========================================  =====================================
``vkc::Texture3D(data, extent)``            :meth:`Renderer.set_volume`
(VulkanTexture.h:55-60)
noise -> pixelData loops                    :meth:`Renderer.generate_volume`
(TestMain.cpp:43-92)
``UniformBuffer<T>::Update`` x2             :meth:`Renderer.set_shader_data`
(TestMain.cpp:248-249)
Model/View/Projection/W2L producer          :func:`reference_shader_data`
(TestMain.cpp:219-245)
frag.glsl constants (:29-32, :42, :63-69)   :func:`march_defaults`, :meth:`Renderer.set_march`
``EnqueueRenderPass("BasePass")`` + draw    :meth:`Renderer.render`
(TestMain.cpp:194-217)
``vkCmdSetScissor`` with a ``VkRect2D``     :meth:`Renderer.render_rect`
(TestMain.cpp:192, 204-205)                 :meth:`Renderer.render_rects` (a list)
==========================================  =====================================

torch is used only for device memory and streams.  All arithmetic runs in
libvr.so, and a missing library raises at import.  Errors are raised as
:class:`VRError`.  The reference throws from ``Error()`` instead (Utils.h:22-29).
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import (BRUSH_ADD, BRUSH_SET, BRUSH_SUB, BYTES_PER_PIXEL, CHANNELS, FLOAT_FORMATS, FMT_RGBA8_SRGB,  # noqa: F401
                   FMT_RGBA8_UNORM, FMT_RGBA32F, Brush, GREY_OF, RAY_RECORD_WORDS, GlobalShaderData, MarchParams, ObjectShaderData, Procedural, RayRecord,
                   Rect, Target, VolumeRecipe, VR_MAX_RECTS, VRError, call)
from ._lib import VOLUME_STATS_BYTES, StatsSummary, VolumeStats
from ._lib import Box, CloneMap
from ._lib import BORDER_CLAMP, FILTER_LINEAR, FILTER_NEAREST, Affine
from ._lib import RANK_MEDIAN
from ._lib import FILL_REPORT_BYTES, FillReport, FillRule
from ._lib import LUT_BYTES, LUT_EQUALIZE, LUT_STRETCH, Lut  # noqa: F401

_lib.load()  # fail at import if the HIP library is missing


def _stream_handle(stream) -> ctypes.c_void_p:
    if stream is None:
        stream = torch.cuda.current_stream()
    if isinstance(stream, torch.cuda.Stream):
        return ctypes.c_void_p(stream.cuda_stream)
    return ctypes.c_void_p(int(stream))


def march_defaults(**overrides) -> MarchParams:
    """The reference's frag.glsl constants, with field overrides."""
    m = MarchParams()
    call("vr_march_defaults", ctypes.byref(m))
    for k, v in overrides.items():
        if isinstance(v, (list, tuple)):
            getattr(m, k)[:] = list(v)
        else:
            setattr(m, k, v)
    return m


def volume_recipe_defaults(**overrides) -> VolumeRecipe:
    """TestMain.cpp:51-62: N=128, freqs (.01,.03,.19,.15), seeds 1..4, literal."""
    r = VolumeRecipe()
    call("vr_volume_recipe_defaults", ctypes.byref(r))
    for k, v in overrides.items():
        if isinstance(v, (list, tuple)):
            getattr(r, k)[:] = list(v)
        else:
            setattr(r, k, v)
    return r


def procedural_defaults(**overrides) -> Procedural:
    """BASELINE config 2 medium (enabled=1); shadow_steps=8 gives config 3."""
    p = Procedural()
    call("vr_procedural_defaults", ctypes.byref(p))
    p.enabled = 1
    for k, v in overrides.items():
        if isinstance(v, (list, tuple)):
            getattr(p, k)[:] = list(v)
        else:
            setattr(p, k, v)
    return p


def scaled_recipe(size: int, literal: bool = True) -> VolumeRecipe:
    """Reference recipe at N = size, with frequencies scaled by 128/size so that
    the continuous field matches the 128^3 one (BASELINE config 5)."""
    r = volume_recipe_defaults(size=size, literal_overwrite=int(literal))
    s = 128.0 / size
    r.freq[:] = [float(np.float32(f) * np.float32(s)) for f in (0.01, 0.03, 0.19, 0.15)]
    return r


def reference_shader_data(aspect: float = 1280.0 / 720.0, phi_deg: float = 0.0, theta_deg: float = 0.0,
                          frame_time: float = 0.0):
    """TestMain.cpp:219-245 computed by libvr's host code (GLM semantics)."""
    osd, gsd = ObjectShaderData(), GlobalShaderData()
    call("vr_reference_shader_data", ctypes.c_float(aspect), ctypes.c_float(phi_deg),
         ctypes.c_float(theta_deg), ctypes.c_float(frame_time), ctypes.byref(osd), ctypes.byref(gsd))
    return osd, gsd


def band_rows_packed(height: int, band_rows: int, band_stride: int = 1, band_first: int = 0,
                     band_flip: int = 0) -> int:
    """Rows vr_render writes for a band set (vr_band_rows_packed); band_flip
    shifts the set's odd bands (vr.h vr_target.band_flip)."""
    n = _lib.load().vr_band_rows_packed(height, band_rows, band_stride, band_first, band_flip)
    if n < 0:
        raise ValueError(f"bad band set: rows {band_rows}, stride {band_stride}, flip {band_flip}")
    return n


def volume_box_footprint(osd: ObjectShaderData, gsd: GlobalShaderData, march: MarchParams, dims, origin, extent,
                         width: int, height: int) -> tuple[int, int, int, int]:
    """vr_volume_box_footprint: the pixel rectangle (x, y, w, h) of the
    width x height frame whose rays can read the texel box `extent` = (bx, by,
    bz) at `origin` = (x0, y0, z0) of a volume of `dims` = (nx, ny, nz).  Host
    code only: needs no renderer and no device.  (0, 0, 0, 0) = no pixel."""
    r = Rect()
    nx, ny, nz = (int(v) for v in dims)
    x0, y0, z0 = (int(v) for v in origin)
    bx, by, bz = (int(v) for v in extent)
    call("vr_volume_box_footprint", ctypes.byref(osd), ctypes.byref(gsd), ctypes.byref(march), nx, ny, nz,
         int(width), int(height), x0, y0, z0, bx, by, bz, ctypes.byref(r))
    return r.x, r.y, r.width, r.height


def _rect_array(rects):
    """A ctypes array of vr_rect from (x, y, w, h) tuples or Rects."""
    rects = list(rects)
    arr = (Rect * len(rects))()
    for i, r in enumerate(rects):
        if isinstance(r, Rect):
            arr[i] = Rect(r.x, r.y, r.width, r.height)
        else:
            x, y, w, h = (int(v) for v in r)
            arr[i] = Rect(x, y, w, h)
    return arr


def coalesce_rects(rects, max_out: int = VR_MAX_RECTS) -> list[tuple[int, int, int, int]]:
    """vr_rects_coalesce: at most `max_out` rectangles (x, y, w, h) whose union
    contains the union of `rects`.  Empty and contained rectangles are dropped;
    then the pair whose bounding rectangle adds the least area is merged until
    the list fits.  Host code only: needs no renderer and no device."""
    arr = _rect_array(rects)
    out = (Rect * max(1, min(len(arr), max(int(max_out), 0))))()
    n = ctypes.c_int(0)
    call("vr_rects_coalesce", arr, len(arr), int(max_out), out, ctypes.byref(n))
    return [(out[i].x, out[i].y, out[i].width, out[i].height) for i in range(n.value)]


_BRUSH_OPS = {"set": BRUSH_SET, "add": BRUSH_ADD, "sub": BRUSH_SUB}


def make_brush(centre, radius, op=BRUSH_SET, falloff: int = 0, value=(255, 255, 255, 255),
               strength=(255, 255, 255, 255)) -> Brush:
    """A vr_brush: `centre` = texel (x, y, z), `radius` = semi-axes in texels (one
    int for a sphere of texels, or three), `op` BRUSH_SET / BRUSH_ADD / BRUSH_SUB
    (or "set" / "add" / "sub"), `falloff` 0 hard or 1 smooth, `value` and
    `strength` per channel R, G, B, A (one int = every channel)."""
    b = Brush()
    b.centre[:] = [int(v) for v in centre]
    b.radius[:] = [int(radius)] * 3 if np.isscalar(radius) else [int(v) for v in radius]
    b.op = _BRUSH_OPS[op] if isinstance(op, str) else int(op)
    b.falloff = int(falloff)
    b.value[:] = [int(value)] * 4 if np.isscalar(value) else [int(v) for v in value]
    b.strength[:] = [int(strength)] * 4 if np.isscalar(strength) else [int(v) for v in strength]
    return b


def brush_box(brush: Brush, dims):
    """vr_brush_box: ``(origin, extent)`` = ((x0, y0, z0), (bx, by, bz)) of the
    brush's bounding box clipped to a volume of `dims` = (nx, ny, nz) -- what
    :meth:`Renderer.paint` rewrites and what :meth:`Renderer.update_footprint`
    takes -- or None when the brush misses the volume.  Host code only."""
    nx, ny, nz = (int(v) for v in dims)
    o, e = (ctypes.c_int * 3)(), (ctypes.c_int * 3)()
    call("vr_brush_box", ctypes.byref(brush), nx, ny, nz, o, e)
    return (tuple(o), tuple(e)) if e[0] > 0 else None


def brush_apply(brush: Brush, rgba: np.ndarray) -> np.ndarray:
    """vr_brush_apply: the brush applied IN PLACE to a host RGBA8 volume shaped
    (nz, ny, nx, 4) (a contiguous uint8 array), the CPU statement of what
    :meth:`Renderer.paint` does on the device; returns `rgba`."""
    if (not isinstance(rgba, np.ndarray) or rgba.dtype != np.uint8 or rgba.ndim != 4 or rgba.shape[3] != 4
            or not rgba.flags.c_contiguous or not rgba.flags.writeable):
        raise ValueError("brush_apply: a writeable contiguous uint8 array shaped (nz, ny, nx, 4)")
    nz, ny, nx, _ = rgba.shape
    call("vr_brush_apply", ctypes.byref(brush), rgba.ctypes.data_as(ctypes.c_void_p), nx, ny, nz)
    return rgba


def brush_blur_apply(brush: Brush, half_width: int, rgba: np.ndarray) -> np.ndarray:
    """vr_brush_blur_apply: the smoothing brush applied to a host RGBA8 volume
    shaped (nz, ny, nx, 4) (a contiguous uint8 array) -- under the brush, each
    channel with a non-zero strength is SET towards the mean of its
    (2 half_width + 1)^3 neighbourhood as it was before the call.  The CPU
    statement of what :meth:`Renderer.blur` does on the device; `brush.op` must
    be BRUSH_SET and `brush.value` is not read.  Writes `rgba` and returns it."""
    if (not isinstance(rgba, np.ndarray) or rgba.dtype != np.uint8 or rgba.ndim != 4 or rgba.shape[3] != 4
            or not rgba.flags.c_contiguous or not rgba.flags.writeable):
        raise ValueError("brush_blur_apply: a writeable contiguous uint8 array shaped (nz, ny, nx, 4)")
    nz, ny, nx, _ = rgba.shape
    call("vr_brush_blur_apply", ctypes.byref(brush), int(half_width), rgba.ctypes.data_as(ctypes.c_void_p), nx, ny, nz)
    return rgba


class Stats(NamedTuple):
    """A vr_volume_stats on the host: `count` and `weight` as ints, `wsum` (4,) and
    `hist` (4, 256) as uint64 arrays."""
    count: int
    weight: int
    wsum: np.ndarray
    hist: np.ndarray


class Summary(NamedTuple):
    """vr_stats_summary's result: per channel, (4,) int64 arrays."""
    n: np.ndarray
    min: np.ndarray
    max: np.ndarray
    mean: np.ndarray
    wmean: np.ndarray
    median: np.ndarray


def unpack_stats(buf) -> Stats:
    """The :class:`Stats` in a vr_volume_stats given as a :class:`VolumeStats`, or as
    its 8240 bytes in a uint8 numpy array or tensor (a CUDA tensor is copied to
    the host, which waits for the work queued before the copy on the current
    stream)."""
    if isinstance(buf, VolumeStats):
        words = np.frombuffer(bytes(buf), np.uint64)
    else:
        if isinstance(buf, torch.Tensor):
            buf = buf.cpu().numpy()
        if not isinstance(buf, np.ndarray) or buf.dtype != np.uint8 or buf.size != VOLUME_STATS_BYTES:
            raise ValueError(f"unpack_stats: a VolumeStats or {VOLUME_STATS_BYTES} uint8 bytes")
        words = np.ascontiguousarray(buf).reshape(-1).view(np.uint64)
    return Stats(int(words[0]), int(words[1]), words[2:6].copy(), words[6:].reshape(4, 256).copy())


def _pack_stats(stats) -> VolumeStats:
    if isinstance(stats, VolumeStats):
        return stats
    if not isinstance(stats, Stats):
        stats = unpack_stats(stats)
    s = VolumeStats()
    words = np.concatenate([np.array([stats.count, stats.weight], np.uint64), np.asarray(stats.wsum, np.uint64).reshape(4),
                            np.asarray(stats.hist, np.uint64).reshape(1024)])
    ctypes.memmove(ctypes.byref(s), words.ctypes.data, VOLUME_STATS_BYTES)
    return s


def _host_volume(fn: str, rgba) -> tuple:
    if (not isinstance(rgba, np.ndarray) or rgba.dtype != np.uint8 or rgba.ndim != 4 or rgba.shape[3] != 4
            or not rgba.flags.c_contiguous):
        raise ValueError(f"{fn}: a contiguous uint8 array shaped (nz, ny, nx, 4)")
    nz, ny, nx, _ = rgba.shape
    return nx, ny, nz


def brush_stats_host(brush: Brush, rgba: np.ndarray) -> Stats:
    """vr_brush_stats_host: the statistics of a host RGBA8 volume shaped
    (nz, ny, nx, 4) under the brush -- the inside texels and their weights are
    :func:`brush_apply`'s, a channel is selected iff its strength is not 0, `op`
    and `value` are not used.  The CPU statement of :meth:`Renderer.brush_stats`."""
    nx, ny, nz = _host_volume("brush_stats_host", rgba)
    s = VolumeStats()
    call("vr_brush_stats_host", ctypes.byref(brush), rgba.ctypes.data_as(ctypes.c_void_p), nx, ny, nz, ctypes.byref(s))
    return unpack_stats(s)


def box_stats_host(rgba: np.ndarray, origin, extent, channels: int = 0xF) -> Stats:
    """vr_box_stats_host: the statistics of the texel box `extent` = (bx, by, bz)
    at `origin` = (x0, y0, z0) of a host RGBA8 volume shaped (nz, ny, nx, 4);
    bit c of `channels` selects channel c.  The CPU statement of
    :meth:`Renderer.box_stats`."""
    nx, ny, nz = _host_volume("box_stats_host", rgba)
    s = VolumeStats()
    call("vr_box_stats_host", rgba.ctypes.data_as(ctypes.c_void_p), nx, ny, nz, *(int(v) for v in origin),
         *(int(v) for v in extent), int(channels), ctypes.byref(s))
    return unpack_stats(s)


def stats_summary(stats) -> Summary:
    """vr_stats_summary: per channel the number of texels counted, the lowest and
    highest byte, the rounded mean, the weighted mean (the eyedropper's value:
    ``value=summary.wmean`` for the next paint) and the median -- all 0 for a
    channel with nothing counted.  `stats` is a :class:`Stats`, a
    :class:`VolumeStats` or whatever :func:`unpack_stats` takes."""
    s, out = _pack_stats(stats), StatsSummary()
    call("vr_stats_summary", ctypes.byref(s), ctypes.byref(out))
    return Summary(*(np.array(list(getattr(out, k)), np.int64) for k in Summary._fields))


def brush_morph_apply(brush: Brush, op: int, half_width: int, rgba: np.ndarray) -> np.ndarray:
    """vr_brush_morph_apply: the erode / dilate brush applied to a host RGBA8
    volume shaped (nz, ny, nx, 4) (a contiguous uint8 array) -- under the brush,
    each channel with a non-zero strength is SET towards the minimum
    (MORPH_ERODE) or maximum (MORPH_DILATE) of its (2 half_width + 1)^3 cube as
    it was before the call.  The CPU statement of what :meth:`Renderer.morph`
    does on the device; `brush.op` must be BRUSH_SET and `brush.value` is not
    read.  Writes `rgba` and returns it."""
    if (not isinstance(rgba, np.ndarray) or rgba.dtype != np.uint8 or rgba.ndim != 4 or rgba.shape[3] != 4
            or not rgba.flags.c_contiguous or not rgba.flags.writeable):
        raise ValueError("brush_morph_apply: a writeable contiguous uint8 array shaped (nz, ny, nx, 4)")
    nz, ny, nx, _ = rgba.shape
    call("vr_brush_morph_apply", ctypes.byref(brush), int(op), int(half_width), rgba.ctypes.data_as(ctypes.c_void_p),
         nx, ny, nz)
    return rgba


def brush_rank_apply(brush: Brush, rank: int, half_width: int, rgba: np.ndarray) -> np.ndarray:
    """vr_brush_rank_apply: the median / rank-filter brush applied to a host
    RGBA8 volume shaped (nz, ny, nx, 4) (a contiguous uint8 array) -- under the
    brush, each channel with a non-zero strength is SET towards the `rank`-th
    smallest byte (0-based; RANK_MEDIAN: the middle one) of its
    (2 half_width + 1)^3 cube as it was before the call.  The CPU statement of
    what :meth:`Renderer.rank` does on the device; `brush.op` must be BRUSH_SET
    and `brush.value` is not read.  Writes `rgba` and returns it."""
    if (not isinstance(rgba, np.ndarray) or rgba.dtype != np.uint8 or rgba.ndim != 4 or rgba.shape[3] != 4
            or not rgba.flags.c_contiguous or not rgba.flags.writeable):
        raise ValueError("brush_rank_apply: a writeable contiguous uint8 array shaped (nz, ny, nx, 4)")
    nz, ny, nx, _ = rgba.shape
    call("vr_brush_rank_apply", ctypes.byref(brush), int(rank), int(half_width), rgba.ctypes.data_as(ctypes.c_void_p),
         nx, ny, nz)
    return rgba


class Fill(NamedTuple):
    """A vr_fill_report on the host: the region's texel count, the passable texels
    under the brush, and the region's inclusive bounds (x, y, z) -- (nx, ny, nz) /
    (-1, -1, -1) when nothing was filled."""
    filled: int
    passable: int
    min: tuple
    max: tuple


def make_fill_rule(seed, lo, hi, select=(1, 0, 0, 0), relative: int = 1) -> FillRule:
    """A vr_fill_rule: `seed` = texel (x, y, z) inside the volume; `select` marks
    the channels R, G, B, A that take part in the test; with `relative` = 1 a
    texel passes when each selected byte lies within `lo` below and `hi` above
    the seed's byte of that channel (clamped to 0..255), with 0 when it lies in
    lo..hi as given.  `lo`, `hi` and `select` are per channel (one int = every
    channel)."""
    r = FillRule()
    r.seed[:] = [int(v) for v in seed]
    r.relative = int(relative)
    r.lo[:] = [int(lo)] * 4 if np.isscalar(lo) else [int(v) for v in lo]
    r.hi[:] = [int(hi)] * 4 if np.isscalar(hi) else [int(v) for v in hi]
    r.select[:] = [int(select)] * 4 if np.isscalar(select) else [int(v) for v in select]
    return r


def unpack_fill_report(buf) -> Fill:
    """The :class:`Fill` in a vr_fill_report given as a :class:`FillReport`, or as
    its 40 bytes in a uint8 numpy array or tensor (a CUDA tensor is copied to
    the host, which waits for the work queued before the copy on the current
    stream)."""
    if not isinstance(buf, FillReport):
        if isinstance(buf, torch.Tensor):
            buf = buf.cpu().numpy()
        if not isinstance(buf, np.ndarray) or buf.dtype != np.uint8 or buf.size != FILL_REPORT_BYTES:
            raise ValueError(f"unpack_fill_report: a FillReport or {FILL_REPORT_BYTES} uint8 bytes")
        buf = FillReport.from_buffer_copy(np.ascontiguousarray(buf).tobytes())
    return Fill(int(buf.filled), int(buf.passable), tuple(buf.min), tuple(buf.max))


def brush_fill_apply(brush: Brush, rule: FillRule, rgba: np.ndarray):
    """vr_brush_fill_apply: the flood-fill brush applied IN PLACE to a host RGBA8
    volume shaped (nz, ny, nx, 4) (a contiguous uint8 array) -- the brush is
    blended, as :func:`brush_apply` blends it, into the texels under it that
    pass `rule` and are connected to its seed by axis steps over such texels.
    The CPU statement of what :meth:`Renderer.fill` does on the device.
    Returns ``(rgba, report)`` with the report a :class:`Fill`."""
    if (not isinstance(rgba, np.ndarray) or rgba.dtype != np.uint8 or rgba.ndim != 4 or rgba.shape[3] != 4
            or not rgba.flags.c_contiguous or not rgba.flags.writeable):
        raise ValueError("brush_fill_apply: a writeable contiguous uint8 array shaped (nz, ny, nx, 4)")
    nz, ny, nx, _ = rgba.shape
    rep = FillReport()
    call("vr_brush_fill_apply", ctypes.byref(brush), ctypes.byref(rule), rgba.ctypes.data_as(ctypes.c_void_p), nx, ny, nz,
         ctypes.byref(rep))
    return rgba, unpack_fill_report(rep)


def make_clone_map(offset=(0, 0, 0), mirror=(0, 0, 0)) -> CloneMap:
    """A vr_clone_map: per axis the source of texel coordinate t is ``t + offset``,
    or ``offset - t`` where `mirror` is 1, clamped to the volume.  A mirror about
    the plane through x = cx is ``offset=(2 * cx, 0, 0), mirror=(1, 0, 0)``."""
    m = CloneMap()
    m.offset[:] = [int(v) for v in offset]
    m.mirror[:] = [int(v) for v in mirror]
    return m


def _host_box(v) -> Box:
    origin, extent = v
    return Box(*(int(x) for x in origin), *(int(x) for x in extent))


def brush_clone_apply(brush: Brush, clone_map: CloneMap, rgba: np.ndarray) -> np.ndarray:
    """vr_brush_clone_apply: the clone brush applied to a host RGBA8 volume shaped
    (nz, ny, nx, 4) (a contiguous uint8 array) -- `brush` blended as
    :func:`brush_apply` blends it, with the value of each texel read from the
    volume's own texel at the mapped position (:func:`make_clone_map`) as it
    was before the call; `brush.value` is not read.  The CPU statement of what
    :meth:`Renderer.clone` does on the device.  Writes `rgba` and returns it."""
    if (not isinstance(rgba, np.ndarray) or rgba.dtype != np.uint8 or rgba.ndim != 4 or rgba.shape[3] != 4
            or not rgba.flags.c_contiguous or not rgba.flags.writeable):
        raise ValueError("brush_clone_apply: a writeable contiguous uint8 array shaped (nz, ny, nx, 4)")
    nz, ny, nx, _ = rgba.shape
    call("vr_brush_clone_apply", ctypes.byref(brush), ctypes.byref(clone_map), rgba.ctypes.data_as(ctypes.c_void_p),
         nx, ny, nz)
    return rgba


def brush_stamp_apply(brush: Brush, stamp: np.ndarray, placement_origin, rgba: np.ndarray) -> np.ndarray:
    """vr_brush_stamp_apply: the stamp brush applied to a host RGBA8 volume shaped
    (nz, ny, nx, 4) -- `brush` blended as :func:`brush_apply` blends it, with
    the value of each texel read from the texel of `stamp` (a contiguous uint8
    array shaped (bz, by, bx, 4), its first texel on volume texel
    `placement_origin` = (x, y, z)) that lies on it; texels the stamp does not
    cover are left alone and `brush.value` is not read.  The CPU statement of
    what :meth:`Renderer.stamp` does on the device.  Writes `rgba` and returns
    it."""
    if (not isinstance(rgba, np.ndarray) or rgba.dtype != np.uint8 or rgba.ndim != 4 or rgba.shape[3] != 4
            or not rgba.flags.c_contiguous or not rgba.flags.writeable):
        raise ValueError("brush_stamp_apply: a writeable contiguous uint8 array shaped (nz, ny, nx, 4)")
    if (not isinstance(stamp, np.ndarray) or stamp.dtype != np.uint8 or stamp.ndim != 4 or stamp.shape[3] != 4
            or not stamp.flags.c_contiguous or stamp.size == 0):
        raise ValueError("brush_stamp_apply: the stamp is a non-empty contiguous uint8 array shaped (bz, by, bx, 4)")
    nz, ny, nx, _ = rgba.shape
    box = _host_box((placement_origin, stamp.shape[2::-1]))
    call("vr_brush_stamp_apply", ctypes.byref(brush), stamp.ctypes.data_as(ctypes.c_void_p), ctypes.byref(box),
         rgba.ctypes.data_as(ctypes.c_void_p), nx, ny, nz)
    return rgba


def stamp_box(brush: Brush, placement, dims):
    """vr_stamp_box: ``(origin, extent)`` of what a stamp edits in a volume of
    `dims` = (nx, ny, nz) -- the brush's clipped box (:func:`brush_box`)
    intersected with `placement` = ((x, y, z), (bx, by, bz)), the texels the
    stamp covers -- or None when it is empty.  What
    :meth:`Renderer.update_footprint` takes after :meth:`Renderer.stamp`."""
    nx, ny, nz = (int(v) for v in dims)
    box = _host_box(placement)
    o, e = (ctypes.c_int * 3)(), (ctypes.c_int * 3)()
    call("vr_stamp_box", ctypes.byref(brush), ctypes.byref(box), nx, ny, nz, o, e)
    return (tuple(o), tuple(e)) if e[0] > 0 else None


def make_affine(m=((65536, 0, 0), (0, 65536, 0), (0, 0, 65536)), pivot=(0, 0, 0), origin=(0, 0, 0),
                filter: int = FILTER_NEAREST, border: int = BORDER_CLAMP) -> Affine:
    """A vr_affine from its 16.16 tables, as they stand: per axis a the source
    position of destination texel t is ``origin[a] + sum_b m[a][b] * (t[b] -
    pivot[b])`` -- `m` and `origin` in 1/65536 of a source texel, `pivot` a
    destination texel.  :func:`affine_place` builds one from a rotation."""
    a = Affine()
    for i in range(3):
        a.m[i][:] = [int(v) for v in m[i]]
    a.pivot[:] = [int(v) for v in pivot]
    a.origin[:] = [int(v) for v in origin]
    a.filter, a.border = int(filter), int(border)
    return a


def affine_identity() -> Affine:
    """vr_affine_identity: the map that reads every texel at its own coordinates,
    FILTER_NEAREST and BORDER_CLAMP."""
    a = Affine()
    call("vr_affine_identity", ctypes.byref(a))
    return a


def affine_place(forward, src_centre, dst_centre, filter: int = FILTER_NEAREST, border: int = BORDER_CLAMP) -> Affine:
    """vr_affine_place: the map that pastes the source rotated / scaled by the
    3 x 3 matrix `forward` with the source position `src_centre` (texels, may
    be fractional) on the destination texel `dst_centre` -- the map stores the
    inverse, rounded to 16.16.  Raises VRError for a singular or non-finite
    matrix and for a coefficient above 256 in magnitude."""
    f = (ctypes.c_double * 9)(*np.asarray(forward, np.float64).reshape(9))
    s = (ctypes.c_double * 3)(*(float(v) for v in src_centre))
    d = (ctypes.c_int32 * 3)(*(int(v) for v in dst_centre))
    a = Affine()
    call("vr_affine_place", f, s, d, int(filter), int(border), ctypes.byref(a))
    return a


def affine_direct(brush: Brush, affine: Affine, dims) -> bool:
    """vr_affine_direct: True when :meth:`Renderer.clone_affine` of this brush
    and map in a volume of `dims` = (nx, ny, nz) takes the direct path (one
    launch, no scratch), False for the staged one."""
    nx, ny, nz = (int(v) for v in dims)
    d = ctypes.c_int()
    call("vr_affine_direct", ctypes.byref(brush), ctypes.byref(affine), nx, ny, nz, ctypes.byref(d))
    return bool(d.value)


def brush_stamp_affine_apply(brush: Brush, stamp: np.ndarray, affine: Affine, rgba: np.ndarray) -> np.ndarray:
    """vr_brush_stamp_affine_apply: the transform paste of `stamp` (a contiguous
    uint8 array shaped (bz, by, bx, 4)) into a host RGBA8 volume shaped
    (nz, ny, nx, 4) -- `brush` blended as :func:`brush_apply` blends it, with
    the value of each texel resampled from the stamp at the position `affine`
    maps it to (nearest or trilinear; outside the stamp clamped to its edge or,
    BORDER_SKIP, left alone).  The CPU statement of what
    :meth:`Renderer.stamp_affine` does on the device.  Writes `rgba` and
    returns it."""
    if (not isinstance(rgba, np.ndarray) or rgba.dtype != np.uint8 or rgba.ndim != 4 or rgba.shape[3] != 4
            or not rgba.flags.c_contiguous or not rgba.flags.writeable):
        raise ValueError("brush_stamp_affine_apply: a writeable contiguous uint8 array shaped (nz, ny, nx, 4)")
    if (not isinstance(stamp, np.ndarray) or stamp.dtype != np.uint8 or stamp.ndim != 4 or stamp.shape[3] != 4
            or not stamp.flags.c_contiguous or stamp.size == 0):
        raise ValueError("brush_stamp_affine_apply: the stamp is a non-empty contiguous uint8 array shaped (bz, by, bx, 4)")
    nz, ny, nx, _ = rgba.shape
    bz, by, bx, _ = stamp.shape
    call("vr_brush_stamp_affine_apply", ctypes.byref(brush), stamp.ctypes.data_as(ctypes.c_void_p), bx, by, bz,
         ctypes.byref(affine), rgba.ctypes.data_as(ctypes.c_void_p), nx, ny, nz)
    return rgba


def brush_clone_affine_apply(brush: Brush, affine: Affine, rgba: np.ndarray) -> np.ndarray:
    """vr_brush_clone_affine_apply: the same with the volume itself, as it was
    before the call, as the source.  The CPU statement of what
    :meth:`Renderer.clone_affine` does on the device.  Writes `rgba` and
    returns it."""
    if (not isinstance(rgba, np.ndarray) or rgba.dtype != np.uint8 or rgba.ndim != 4 or rgba.shape[3] != 4
            or not rgba.flags.c_contiguous or not rgba.flags.writeable):
        raise ValueError("brush_clone_affine_apply: a writeable contiguous uint8 array shaped (nz, ny, nx, 4)")
    nz, ny, nx, _ = rgba.shape
    call("vr_brush_clone_affine_apply", ctypes.byref(brush), ctypes.byref(affine), rgba.ctypes.data_as(ctypes.c_void_p),
         nx, ny, nz)
    return rgba


def brush_warp_apply(brush: Brush, affine: Affine, rgba: np.ndarray) -> np.ndarray:
    """vr_brush_warp_apply: the liquify brush on a host RGBA8 volume shaped
    (nz, ny, nx, 4) -- every texel under `brush` (op BRUSH_SET) resampled from
    the volume as it was at a position between its own and the one `affine`
    maps it to, by the brush weight.  The CPU statement of what
    :meth:`Renderer.warp` does on the device.  Writes `rgba` and returns it."""
    if (not isinstance(rgba, np.ndarray) or rgba.dtype != np.uint8 or rgba.ndim != 4 or rgba.shape[3] != 4
            or not rgba.flags.c_contiguous or not rgba.flags.writeable):
        raise ValueError("brush_warp_apply: a writeable contiguous uint8 array shaped (nz, ny, nx, 4)")
    nz, ny, nx, _ = rgba.shape
    call("vr_brush_warp_apply", ctypes.byref(brush), ctypes.byref(affine), rgba.ctypes.data_as(ctypes.c_void_p), nx, ny, nz)
    return rgba


def warp_reach(brush: Brush, affine: Affine):
    """vr_warp_reach: per axis the largest displacement ``|A - I|`` (16.16, as
    ints, saturated at 2**31 - 1) that `affine` asks for at the 8 corners of the
    brush's unclipped box; :meth:`Renderer.warp` refuses a map that passes
    ``WARP_MAX_DISP << 16`` on an axis."""
    r = (ctypes.c_int32 * 3)()
    call("vr_warp_reach", ctypes.byref(brush), ctypes.byref(affine), r)
    return tuple(r)


def warp_push(centre, d16, filter: int = FILTER_LINEAR, border: int = BORDER_CLAMP) -> Affine:
    """vr_warp_push: the map with which :meth:`Renderer.warp` pushes what is
    under a brush at `centre` by `d16` = (dx, dy, dz) in 1/65536 of a texel."""
    c = (ctypes.c_int32 * 3)(*(int(v) for v in centre))
    d = (ctypes.c_int32 * 3)(*(int(v) for v in d16))
    a = Affine()
    call("vr_warp_push", c, d, int(filter), int(border), ctypes.byref(a))
    return a


def _lut_struct(fn: str, lut) -> Lut:
    """The vr_lut of a (4, 256) uint8 array (or a Lut, as it is): a copy."""
    if isinstance(lut, Lut):
        return lut
    if not isinstance(lut, np.ndarray) or lut.dtype != np.uint8 or lut.shape != (4, 256):
        raise ValueError(f"{fn}: a table is a uint8 array shaped (4, 256)")
    s = Lut()
    ctypes.memmove(ctypes.byref(s), np.ascontiguousarray(lut).ctypes.data, LUT_BYTES)
    return s


def _lut_array(s: Lut) -> np.ndarray:
    return np.frombuffer(bytes(s), np.uint8).reshape(4, 256).copy()


def lut_identity() -> np.ndarray:
    """vr_lut_identity: the table that maps every byte to itself, a (4, 256)
    uint8 array -- ``lut[c, v]`` is the value for byte v of channel c, what
    :meth:`Renderer.remap` and :func:`brush_remap_apply` take."""
    s = Lut()
    call("vr_lut_identity", ctypes.byref(s))
    return _lut_array(s)


def lut_levels(in_lo: int, in_hi: int, out_lo: int, out_hi: int, channels: int = 0xF, lut=None) -> np.ndarray:
    """vr_lut_levels: a new table in which the channels of `channels` (bit c =
    channel c) map ``v <= in_lo`` to `out_lo`, ``v >= in_hi`` to `out_hi` and
    the bytes between them along the line through the two, rounded to the
    nearest; the other channels keep what `lut` holds (default: the
    identity), so calls stack per channel.  ``0 <= in_lo < in_hi <= 255``;
    `out_lo` and `out_hi` in 0..255 in either order: ``(0, 255, 255, 0)``
    inverts, ``(T - 1, T, 0, 255)`` is a threshold at T."""
    s = Lut()
    if lut is None:
        call("vr_lut_identity", ctypes.byref(s))
    else:
        ctypes.memmove(ctypes.byref(s), ctypes.byref(_lut_struct("lut_levels", lut)), LUT_BYTES)
    call("vr_lut_levels", ctypes.byref(s), int(channels), int(in_lo), int(in_hi), int(out_lo), int(out_hi))
    return _lut_array(s)


def lut_compose(first, then) -> np.ndarray:
    """vr_lut_compose: the table of `first` followed by `then`,
    ``out[c, v] = then[c, first[c, v]]``."""
    a, b, out = _lut_struct("lut_compose", first), _lut_struct("lut_compose", then), Lut()
    call("vr_lut_compose", ctypes.byref(a), ctypes.byref(b), ctypes.byref(out))
    return _lut_array(out)


def stats_lut(stats, kind: int, channels: int = 0xF) -> np.ndarray:
    """vr_stats_lut: a table from the histograms of `stats` (a :class:`Stats`,
    as :meth:`Renderer.brush_stats` returns it, a :class:`VolumeStats` or
    whatever :func:`unpack_stats` takes).  `kind` LUT_STRETCH maps the lowest
    non-empty bin to 0 and the highest to 255 linearly, LUT_EQUALIZE maps byte
    v by the cumulative count up to v; a channel outside `channels`, an empty
    one and one with a single non-empty bin get the identity.  The CPU
    statement of :meth:`Renderer.stats_lut`."""
    s, out = _pack_stats(stats), Lut()
    call("vr_stats_lut", ctypes.byref(s), int(kind), int(channels), ctypes.byref(out))
    return _lut_array(out)


def brush_remap_apply(brush: Brush, lut, rgba: np.ndarray) -> np.ndarray:
    """vr_brush_remap_apply: the lookup-table brush applied to a host RGBA8
    volume shaped (nz, ny, nx, 4) (a contiguous uint8 array) -- `brush` blended
    as :func:`brush_apply` blends it, with the value of each texel and channel
    read from `lut` (a (4, 256) uint8 array) at the texel's own old byte;
    `brush.value` is not read.  The CPU statement of what
    :meth:`Renderer.remap` does on the device.  Writes `rgba` and returns it."""
    if (not isinstance(rgba, np.ndarray) or rgba.dtype != np.uint8 or rgba.ndim != 4 or rgba.shape[3] != 4
            or not rgba.flags.c_contiguous or not rgba.flags.writeable):
        raise ValueError("brush_remap_apply: a writeable contiguous uint8 array shaped (nz, ny, nx, 4)")
    nz, ny, nx, _ = rgba.shape
    s = _lut_struct("brush_remap_apply", lut)
    call("vr_brush_remap_apply", ctypes.byref(brush), ctypes.byref(s), rgba.ctypes.data_as(ctypes.c_void_p), nx, ny, nz)
    return rgba


def _brush_copy(b: Brush) -> Brush:
    c = Brush()
    ctypes.memmove(ctypes.byref(c), ctypes.byref(b), ctypes.sizeof(Brush))
    return c


def brush_line(brush: Brush, to, spacing: int, skip_first: bool = False) -> list[Brush]:
    """vr_brush_line: the dabs of a drag from ``brush.centre`` to the texel `to`
    = (x, y, z), copies of `brush` at most `spacing` texels apart on the longest
    axis, the first on the brush's own centre (omitted with `skip_first`, so
    that the joint of two segments is not dabbed twice) and the last on `to`.
    What :meth:`Renderer.paint_stroke` takes.  Host code only."""
    t = (ctypes.c_int32 * 3)(*(int(v) for v in to))
    n = ctypes.c_int(0)
    lib = _lib.load()
    st = lib.vr_brush_line(ctypes.byref(brush), t, int(spacing), int(skip_first), None, 0, ctypes.byref(n))
    if n.value <= 0:   # refused for another reason than the room
        _lib.check(st, "vr_brush_line")
    out = (Brush * n.value)()
    call("vr_brush_line", ctypes.byref(brush), t, int(spacing), int(skip_first), out, n.value, ctypes.byref(n))
    return [_brush_copy(out[i]) for i in range(n.value)]


def coalesce_boxes(boxes, max_out: int):
    """vr_boxes_coalesce: at most `max_out` texel boxes ``(origin, extent)`` =
    ((x, y, z), (bx, by, bz)) whose union contains the union of `boxes` (the
    same pairs).  Empty and contained boxes are dropped; then the pair whose
    bounding box adds the least volume is merged until the list fits.  Host
    code only: needs no renderer and no device."""
    boxes = list(boxes)
    arr = (_lib.Box * len(boxes))()
    for i, (o, e) in enumerate(boxes):
        arr[i] = _lib.Box(*(int(v) for v in o), *(int(v) for v in e))
    out = (_lib.Box * max(1, min(len(arr), max(int(max_out), 0))))()
    n = ctypes.c_int(0)
    call("vr_boxes_coalesce", arr, len(arr), int(max_out), out, ctypes.byref(n))
    return [((out[i].x, out[i].y, out[i].z), (out[i].bx, out[i].by, out[i].bz)) for i in range(n.value)]


# vr_ray_record as a numpy structured type (the layout of _lib.RayRecord)
RAY_RECORD_DTYPE = np.dtype([("steps", "<i4"), ("hit_step", "<i4"), ("value", "<f4"), ("optical_depth", "<f4"),
                             ("entry", "<f4", (3,)), ("reserved0", "<f4"), ("step", "<f4", (3,)), ("reserved1", "<f4"),
                             ("hit", "<f4", (3,)), ("reserved2", "<f4")])
assert RAY_RECORD_DTYPE.itemsize == ctypes.sizeof(RayRecord) == 4 * RAY_RECORD_WORDS


def ray_records(words) -> np.ndarray:
    """:meth:`Renderer.query_rect`'s int32 tensor (or array) [..., 16] on the
    host, viewed as records with named fields (``steps``, ``hit_step``,
    ``value``, ``optical_depth``, ``entry``, ``step``, ``hit``): shape [...]."""
    a = words.cpu().numpy() if isinstance(words, torch.Tensor) else np.asarray(words)
    if a.dtype != np.int32 or a.shape[-1] != RAY_RECORD_WORDS:
        raise ValueError(f"ray records are int32 [..., {RAY_RECORD_WORDS}], got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a).view(RAY_RECORD_DTYPE).reshape(a.shape[:-1])


def shader_data_arrays(osd: ObjectShaderData, gsd: GlobalShaderData):
    """(obj48, glob36) float32 arrays, the layout the oracle takes."""
    obj = np.ctypeslib.as_array(ctypes.cast(ctypes.byref(osd), ctypes.POINTER(ctypes.c_float)), (48,)).copy()
    glob = np.ctypeslib.as_array(ctypes.cast(ctypes.byref(gsd), ctypes.POINTER(ctypes.c_float)), (36,)).copy()
    return obj, glob


class Renderer:
    """Offscreen ray-march renderer on one HIP device (one per process/rank)."""

    def __init__(self, device: int = 0):
        self._ctx = ctypes.c_void_p()
        call("vr_create", int(device), ctypes.byref(self._ctx))
        self.device = int(device)
        self.march = march_defaults()

    # -- lifetime --------------------------------------------------------
    def close(self) -> None:
        if self._ctx:
            _lib.load().vr_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass

    # -- volume (Texture3D) ------------------------------------------------
    def set_volume(self, rgba) -> None:
        """Upload an RGBA8 volume shaped (nz, ny, nx, 4), x fastest (TestMain.cpp:69-87)."""
        if isinstance(rgba, torch.Tensor) and rgba.is_cuda:
            return self.set_volume_device(rgba)
        a = np.ascontiguousarray(rgba, dtype=np.uint8)
        if a.ndim != 4 or a.shape[3] != 4:
            raise ValueError("volume must be shaped (nz, ny, nx, 4)")
        nz, ny, nx, _ = a.shape
        call("vr_set_volume", self._ctx, a.ctypes.data_as(ctypes.c_void_p), nx, ny, nz)

    def set_volume_device(self, t: torch.Tensor, stream=None) -> None:
        if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 4 or not t.is_contiguous():
            raise ValueError("device volume must be a contiguous uint8 tensor (nz, ny, nx, 4)")
        nz, ny, nx, _ = t.shape
        h = _stream_handle(stream)
        call("vr_set_volume_device", self._ctx, ctypes.c_void_p(t.data_ptr()), nx, ny, nz, h)
        (stream if stream is not None else torch.cuda.current_stream()).synchronize()

    def update_volume(self, box, origin, stream=None) -> None:
        """Overwrite the texel box shaped (bz, by, bx, 4) at origin = (x0, y0, z0)
        of the installed volume (vr_update_volume): the renderer then holds the
        patched volume, bit for bit, at a cost that follows the box.  A numpy
        array goes through the synchronous host call.  A CUDA uint8 tensor is
        queued on `stream` (default: the current stream); with a stream given
        nothing waits, so update and render queue back to back on it, and the
        caller keeps the tensor alive until the update has run."""
        x0, y0, z0 = (int(v) for v in origin)
        if isinstance(box, torch.Tensor) and box.is_cuda:
            if box.dtype != torch.uint8 or box.dim() != 4 or box.shape[3] != 4 or not box.is_contiguous():
                raise ValueError("device box must be a contiguous uint8 tensor (bz, by, bx, 4)")
            bz, by, bx, _ = box.shape
            call("vr_update_volume_device", self._ctx, ctypes.c_void_p(box.data_ptr()), x0, y0, z0, bx, by, bz,
                 _stream_handle(stream))
            if stream is None:
                torch.cuda.current_stream().synchronize()
            return
        a = np.ascontiguousarray(box, dtype=np.uint8)
        if a.ndim != 4 or a.shape[3] != 4:
            raise ValueError("box must be shaped (bz, by, bx, 4)")
        bz, by, bx, _ = a.shape
        call("vr_update_volume", self._ctx, a.ctypes.data_as(ctypes.c_void_p), x0, y0, z0, bx, by, bz)

    def paint(self, centre, radius, op=BRUSH_SET, falloff: int = 0, value=(255, 255, 255, 255),
              strength=(255, 255, 255, 255), stream=None):
        """Blend an ellipsoidal brush into the installed volume on the device
        (vr_paint; the arguments are :func:`make_brush`'s): the renderer then
        holds the painted volume, bit for bit what :func:`brush_apply` gives on
        the host.  Returns ``(origin, extent)`` of the clipped bounding box it
        rewrote -- what :meth:`update_footprint` takes -- or None when the brush
        misses the volume.  Queued on `stream` (default: the current stream);
        with a stream given nothing waits, so pick, paint and render queue
        back to back on it."""
        b = make_brush(centre, radius, op, falloff, value, strength)
        call("vr_paint", self._ctx, ctypes.byref(b), _stream_handle(stream))
        if stream is None:
            torch.cuda.current_stream().synchronize()
        return brush_box(b, self.volume_dims())

    def paint_stroke(self, brushes, stream=None):
        """Apply a list of at most VR_MAX_DABS :class:`Brush` dabs, in order, in
        one paint launch (vr_paint_stroke): the renderer then holds, bit for bit,
        what :meth:`paint` of each in turn would leave, with every texel loaded
        and stored once and the device layouts rebuilt over a few boxes instead
        of per dab.  Returns the list of ``(origin, extent)`` of the clipped
        boxes of the dabs that reach the volume -- what
        :meth:`update_footprints` takes, so an editor's loop is
        ``pick -> brush_line -> paint_stroke -> update_footprints ->
        render_rects``.  Queued on `stream` as :meth:`paint` is."""
        brushes = list(brushes)
        arr = (Brush * max(1, len(brushes)))()
        for i, b in enumerate(brushes):
            ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(b), ctypes.sizeof(Brush))
        call("vr_paint_stroke", self._ctx, arr if brushes else None, len(brushes), _stream_handle(stream))
        if stream is None:
            torch.cuda.current_stream().synchronize()
        if not brushes:
            return []
        dims = self.volume_dims()
        return [box for box in (brush_box(b, dims) for b in brushes) if box is not None]

    def blur(self, centre, radius, half_width: int = 1, falloff: int = 0, strength=(255, 255, 255, 255), stream=None):
        """Soften the installed volume under an ellipsoidal brush on the device
        (vr_blur): each channel with a non-zero strength is SET towards the
        mean of its (2 half_width + 1)^3 neighbourhood (half_width 1..3,
        clamp-to-edge) as it was before the call, weighted as :meth:`paint`
        weights a SET brush -- bit for bit what :func:`brush_blur_apply` gives
        on the host.  Returns ``(origin, extent)`` of the clipped bounding box
        it rewrote, or None when the brush misses the volume, and queues on
        `stream` as :meth:`paint` does.  The staging scratch grows (after a
        device synchronisation) only when a call needs more than the renderer
        holds; ``set_option("blur_scratch_kib", k)`` reserves it beforehand."""
        b = make_brush(centre, radius, BRUSH_SET, falloff, 0, strength)
        call("vr_blur", self._ctx, ctypes.byref(b), int(half_width), _stream_handle(stream))
        if stream is None:
            torch.cuda.current_stream().synchronize()
        return brush_box(b, self.volume_dims())

    def _stats_out(self, fn: str, out):
        if out is None:
            return torch.empty(VOLUME_STATS_BYTES, dtype=torch.uint8, device=torch.device("cuda", self.device))
        if (not isinstance(out, torch.Tensor) or not out.is_cuda or out.device.index != self.device
                or out.dtype != torch.uint8 or out.numel() != VOLUME_STATS_BYTES or not out.is_contiguous()):
            raise ValueError(f"{fn}: out must be a contiguous uint8 tensor of {VOLUME_STATS_BYTES} bytes on cuda:{self.device}")
        return out

    def brush_stats(self, centre, radius, falloff: int = 0, strength=(255, 255, 255, 255), stream=None, out=None):
        """What is in the installed volume under an ellipsoidal brush
        (vr_brush_stats): the number of inside texels, the sum of their weights
        and, per channel with a non-zero strength, the weighted byte sum and
        the 256-bin histogram -- bit for bit what :func:`brush_stats_host`
        gives on the host.  The brush is :meth:`paint`'s; nothing is written
        but the result.  Without `out`: a :class:`Stats` on the host, after a
        synchronise of `stream` (default: the current stream).  With `out`, a
        CUDA uint8 tensor of 8240 bytes (8-byte aligned): the call is queued on
        `stream`, nothing waits and `out` is returned -- :func:`unpack_stats`
        reads it later, :func:`stats_summary` gives min / max / mean / median
        and the eyedropper's value."""
        b = make_brush(centre, radius, BRUSH_SET, falloff, 0, strength)
        buf = self._stats_out("brush_stats", out)
        call("vr_brush_stats", self._ctx, ctypes.byref(b), ctypes.c_void_p(buf.data_ptr()), _stream_handle(stream))
        return buf if out is not None else self._stats_host(buf, stream)

    def box_stats(self, origin, extent, channels: int = 0xF, stream=None, out=None):
        """The same over the texel box `extent` = (bx, by, bz) at `origin` =
        (x0, y0, z0) (vr_box_stats): every texel counts with weight 256; bit c
        of `channels` selects channel c.  ``box_stats((0, 0, 0),
        volume_dims())`` with min == max in its summary says a channel is
        constant again.  `stream` and `out` as for :meth:`brush_stats`."""
        buf = self._stats_out("box_stats", out)
        call("vr_box_stats", self._ctx, *(int(v) for v in origin), *(int(v) for v in extent), int(channels),
             ctypes.c_void_p(buf.data_ptr()), _stream_handle(stream))
        return buf if out is not None else self._stats_host(buf, stream)

    @staticmethod
    def _stats_host(buf, stream) -> Stats:
        s = torch.cuda.current_stream() if stream is None else stream
        if isinstance(s, torch.cuda.Stream):
            s.synchronize()
        else:
            torch.cuda.synchronize()
        return unpack_stats(buf)

    def morph(self, centre, radius, op, half_width: int = 1, falloff: int = 0, strength=(255, 255, 255, 255),
              stream=None):
        """Grow or shrink the installed volume under an ellipsoidal brush on the
        device (vr_morph): each channel with a non-zero strength is SET towards
        the minimum (`op` = MORPH_ERODE) or maximum (MORPH_DILATE) of its
        (2 half_width + 1)^3 cube (half_width 1..3, clamp-to-edge) as it was
        before the call, weighted as :meth:`paint` weights a SET brush -- bit
        for bit what :func:`brush_morph_apply` gives on the host.  Returns
        ``(origin, extent)`` of the clipped bounding box it rewrote, or None
        when the brush misses the volume, and queues on `stream` as
        :meth:`paint` does.  The staging scratch is :meth:`blur`'s
        (``blur_scratch_kib``) and grows by the same rule."""
        b = make_brush(centre, radius, BRUSH_SET, falloff, 0, strength)
        call("vr_morph", self._ctx, ctypes.byref(b), int(op), int(half_width), _stream_handle(stream))
        if stream is None:
            torch.cuda.current_stream().synchronize()
        return brush_box(b, self.volume_dims())

    def rank(self, centre, radius, rank: int = RANK_MEDIAN, half_width: int = 1, falloff: int = 0,
             strength=(255, 255, 255, 255), stream=None):
        """Remove speckle under an ellipsoidal brush on the device and leave
        edges where they are (vr_rank): each channel with a non-zero strength
        is SET towards the `rank`-th smallest byte (0-based; RANK_MEDIAN, the
        default, is the median; 0 is :meth:`morph`'s erode and the last rank
        its dilate) of its (2 half_width + 1)^3 cube (half_width 1..3,
        clamp-to-edge) as it was before the call, weighted as :meth:`paint`
        weights a SET brush -- bit for bit what :func:`brush_rank_apply` gives
        on the host.  Returns ``(origin, extent)`` of the clipped bounding box
        it rewrote, or None when the brush misses the volume, and queues on
        `stream` as :meth:`paint` does.  The staging scratch is :meth:`blur`'s
        (``blur_scratch_kib``) and grows by the same rule."""
        b = make_brush(centre, radius, BRUSH_SET, falloff, 0, strength)
        call("vr_rank", self._ctx, ctypes.byref(b), int(rank), int(half_width), _stream_handle(stream))
        if stream is None:
            torch.cuda.current_stream().synchronize()
        return brush_box(b, self.volume_dims())

    def fill(self, seed, centre, radius, op=BRUSH_SET, falloff: int = 0, value=(255, 255, 255, 255),
             strength=(255, 255, 255, 255), rule: FillRule | None = None, report=None, stream=None):
        """Bucket fill / magic wand on the device (vr_fill): the brush of
        :meth:`paint` blended into the texels under it that pass `rule` (a
        :func:`make_fill_rule`; its seed is replaced by `seed` when that is
        not None) and are connected to the seed texel by steps of one texel
        along an axis over such texels, never leaving the ellipsoid -- bit for
        bit what :func:`brush_fill_apply` gives on the host.  Returns
        ``(origin, extent)`` of the brush's clipped bounding box (the edited
        box, what :meth:`update_footprint` takes) or None when the brush misses
        the volume, and queues on `stream` as :meth:`paint` does.  With
        ``report=True`` a CUDA uint8 tensor of 40 bytes is allocated for the
        vr_fill_report, with ``report=`` such a tensor (8-byte aligned) that one
        is used; either way the result is ``((origin, extent), tensor)`` and
        :func:`unpack_fill_report` reads the tensor later.  With every strength
        0 and a report the call only measures.  The labels live in
        :meth:`blur`'s scratch (``blur_scratch_kib``), 4 bytes per texel of the
        clipped box, grown by the same rule."""
        if rule is None:
            raise ValueError("fill: a rule is needed (make_fill_rule)")
        r = FillRule.from_buffer_copy(bytes(rule))
        if seed is not None:
            r.seed[:] = [int(v) for v in seed]
        b = make_brush(centre, radius, op, falloff, value, strength)
        buf = None
        if report is True:
            buf = torch.empty(FILL_REPORT_BYTES, dtype=torch.uint8, device=torch.device("cuda", self.device))
        elif report is not None and report is not False:
            if (not isinstance(report, torch.Tensor) or not report.is_cuda or report.device.index != self.device
                    or report.dtype != torch.uint8 or report.numel() != FILL_REPORT_BYTES or not report.is_contiguous()):
                raise ValueError(f"fill: report must be a contiguous uint8 tensor of {FILL_REPORT_BYTES} bytes on cuda:{self.device}")
            buf = report
        call("vr_fill", self._ctx, ctypes.byref(b), ctypes.byref(r), ctypes.c_void_p(buf.data_ptr()) if buf is not None else None,
             _stream_handle(stream))
        if stream is None:
            torch.cuda.current_stream().synchronize()
        box = brush_box(b, self.volume_dims())
        return box if buf is None else (box, buf)

    def clone(self, centre, radius, offset, mirror=(0, 0, 0), op=BRUSH_SET, falloff: int = 0,
              strength=(255, 255, 255, 255), stream=None):
        """Paint the installed volume under an ellipsoidal brush with its own
        texels from elsewhere, on the device (vr_clone): the brush is
        :meth:`paint`'s, with the value of texel t read from the texel at
        ``t + offset`` (per axis ``offset - t`` where `mirror` is 1), clamped to
        the volume, as it was before the call -- a clone stamp for an offset
        larger than the brush, a push for an offset of a texel, a mirror about
        the plane x = cx for ``offset=(2 * cx, 0, 0), mirror=(1, 0, 0)``.  Bit
        for bit what :func:`brush_clone_apply` gives on the host.  Returns
        ``(origin, extent)`` of the clipped bounding box it rewrote, or None
        when the brush misses the volume, and queues on `stream` as
        :meth:`paint` does.  A source that does not meet the box costs one
        launch and no scratch; one that does goes through :meth:`blur`'s
        staging scratch (``blur_scratch_kib``), which grows by the same rule."""
        b = make_brush(centre, radius, op, falloff, 0, strength)
        m = make_clone_map(offset, mirror)
        call("vr_clone", self._ctx, ctypes.byref(b), ctypes.byref(m), _stream_handle(stream))
        if stream is None:
            torch.cuda.current_stream().synchronize()
        return brush_box(b, self.volume_dims())

    def stamp(self, stamp_tensor, placement_origin, centre, radius, op=BRUSH_SET, falloff: int = 0,
              strength=(255, 255, 255, 255), stream=None):
        """Paint the installed volume under an ellipsoidal brush with the texels
        of a device box (vr_stamp): `stamp_tensor` is a contiguous CUDA uint8
        tensor shaped (bz, by, bx, 4) -- what :meth:`get_volume_box` returns on
        the device -- whose first texel lies on volume texel `placement_origin`
        = (x, y, z); the brush is :meth:`paint`'s, with the value of a texel
        read from the stamp texel on it, and texels the stamp does not cover
        are left alone.  Bit for bit what :func:`brush_stamp_apply` gives on
        the host.  Returns ``(origin, extent)`` of the box it edited
        (:func:`stamp_box`), or None when that is empty.  One launch queued on
        `stream` as :meth:`paint` is: no scratch, no host wait; the tensor must
        be 4-byte aligned and stay alive until the launch has run."""
        if (not isinstance(stamp_tensor, torch.Tensor) or not stamp_tensor.is_cuda
                or stamp_tensor.device.index != self.device or stamp_tensor.dtype != torch.uint8
                or stamp_tensor.dim() != 4 or stamp_tensor.shape[3] != 4 or not stamp_tensor.is_contiguous()):
            raise ValueError(f"stamp: a contiguous uint8 tensor shaped (bz, by, bx, 4) on cuda:{self.device}")
        bz, by, bx, _ = stamp_tensor.shape
        b = make_brush(centre, radius, op, falloff, 0, strength)
        placement = (placement_origin, (bx, by, bz))
        box = _host_box(placement)
        # an empty stamp has no buffer to hand over: the library refuses the extent either way
        ptr = ctypes.c_void_p(stamp_tensor.data_ptr()) if stamp_tensor.numel() else ctypes.c_void_p(4)
        call("vr_stamp", self._ctx, ctypes.byref(b), ptr, ctypes.byref(box), _stream_handle(stream))
        if stream is None:
            torch.cuda.current_stream().synchronize()
        return stamp_box(b, placement, self.volume_dims())

    def stamp_affine(self, stamp_tensor, affine: Affine, centre, radius, op=BRUSH_SET, falloff: int = 0,
                     strength=(255, 255, 255, 255), stream=None):
        """Paste a device box rotated, scaled, sheared or shifted by a fraction
        of a texel (vr_stamp_affine): `stamp_tensor` is a contiguous CUDA uint8
        tensor shaped (bz, by, bx, 4) -- what :meth:`get_volume_box` returns on
        the device; the brush is :meth:`paint`'s, with the value of a texel
        resampled from the stamp at the position `affine`
        (:func:`affine_place`, :func:`make_affine`) maps it to, nearest or
        trilinear; a position outside the stamp reads its edge (BORDER_CLAMP)
        or leaves the texel alone (BORDER_SKIP).  Bit for bit what
        :func:`brush_stamp_affine_apply` gives on the host.  Returns
        ``(origin, extent)`` of the brush's clipped box, or None when it misses
        the volume.  One launch queued on `stream` as :meth:`paint` is: no
        scratch, no host wait; the tensor must be 4-byte aligned and stay alive
        until the launch has run."""
        if (not isinstance(stamp_tensor, torch.Tensor) or not stamp_tensor.is_cuda
                or stamp_tensor.device.index != self.device or stamp_tensor.dtype != torch.uint8
                or stamp_tensor.dim() != 4 or stamp_tensor.shape[3] != 4 or not stamp_tensor.is_contiguous()):
            raise ValueError(f"stamp_affine: a contiguous uint8 tensor shaped (bz, by, bx, 4) on cuda:{self.device}")
        bz, by, bx, _ = stamp_tensor.shape
        b = make_brush(centre, radius, op, falloff, 0, strength)
        # an empty stamp has no buffer to hand over: the library refuses the extent either way
        ptr = ctypes.c_void_p(stamp_tensor.data_ptr()) if stamp_tensor.numel() else ctypes.c_void_p(4)
        call("vr_stamp_affine", self._ctx, ctypes.byref(b), ptr, bx, by, bz, ctypes.byref(affine), _stream_handle(stream))
        if stream is None:
            torch.cuda.current_stream().synchronize()
        return brush_box(b, self.volume_dims())

    def clone_affine(self, centre, radius, affine: Affine, op=BRUSH_SET, falloff: int = 0, strength=(255, 255, 255, 255),
                     stream=None):
        """The same with the installed volume itself, as it was before the
        call, as the source (vr_clone_affine): :meth:`clone` through an affine
        map and a filter.  Bit for bit what :func:`brush_clone_affine_apply`
        gives on the host.  A read range that does not meet the brush's box
        costs one launch and no scratch (:func:`affine_direct`); one that does
        goes through :meth:`blur`'s staging scratch (``blur_scratch_kib``),
        which grows by the same rule."""
        b = make_brush(centre, radius, op, falloff, 0, strength)
        call("vr_clone_affine", self._ctx, ctypes.byref(b), ctypes.byref(affine), _stream_handle(stream))
        if stream is None:
            torch.cuda.current_stream().synchronize()
        return brush_box(b, self.volume_dims())

    def warp(self, centre, radius, affine: Affine, falloff: int = 1, strength=(255, 255, 255, 255), stream=None):
        """Liquify (vr_warp): move what is under the brush -- push
        (:func:`warp_push`), pinch, bloat or twirl (:func:`affine_place` with
        `centre` as both centres) -- by an amount that fades out towards the
        rim.  Every texel under the brush is resampled from the volume as it
        was before the call at a position between its own and the one `affine`
        maps it to, blended by the brush weight; `strength` sets how much of
        the resampled value replaces the old byte.  Bit for bit what
        :func:`brush_warp_apply` gives on the host.  Returns ``(origin,
        extent)`` of the brush's clipped box, or None when it misses the
        volume.  Two launches through :meth:`blur`'s staging scratch
        (``blur_scratch_kib``), which grows by the same rule; queued on
        `stream` as :meth:`paint` is."""
        b = make_brush(centre, radius, BRUSH_SET, falloff, 0, strength)
        call("vr_warp", self._ctx, ctypes.byref(b), ctypes.byref(affine), _stream_handle(stream))
        if stream is None:
            torch.cuda.current_stream().synchronize()
        return brush_box(b, self.volume_dims())

    def remap(self, centre, radius, lut, op=BRUSH_SET, falloff: int = 0, strength=(255, 255, 255, 255), stream=None):
        """Paint the installed volume under an ellipsoidal brush with a function
        of each texel's own byte, on the device (vr_remap): the brush is
        :meth:`paint`'s, with the value of a texel's channel c read from
        ``lut[c, old byte]`` -- levels, invert, threshold, posterise
        (:func:`lut_levels`, :func:`lut_compose`), stretch and equalise
        (:func:`stats_lut`, :meth:`stats_lut`).  `lut` is a (4, 256) uint8 numpy
        array, copied during the call (vr_remap: it may be overwritten as soon
        as this returns), or a contiguous CUDA uint8 tensor of 1024 elements
        (4-byte aligned), read when the kernel runs (vr_remap_device: a table
        written earlier on `stream` is the one applied, and the tensor must
        stay alive until then).  Bit for bit what :func:`brush_remap_apply`
        gives on the host.  Returns ``(origin, extent)`` of the clipped
        bounding box it rewrote, or None when the brush misses the volume, and
        queues on `stream` as :meth:`paint` does: one launch, no scratch, no
        host wait."""
        b = make_brush(centre, radius, op, falloff, 0, strength)
        if isinstance(lut, torch.Tensor):
            if (not lut.is_cuda or lut.device.index != self.device or lut.dtype != torch.uint8
                    or lut.numel() != LUT_BYTES or not lut.is_contiguous()):
                raise ValueError(f"remap: a device table is a contiguous uint8 tensor of {LUT_BYTES} elements on cuda:{self.device}")
            call("vr_remap_device", self._ctx, ctypes.byref(b), ctypes.c_void_p(lut.data_ptr()), _stream_handle(stream))
        else:
            s = _lut_struct("remap", lut)
            call("vr_remap", self._ctx, ctypes.byref(b), ctypes.byref(s), _stream_handle(stream))
        if stream is None:
            torch.cuda.current_stream().synchronize()
        return brush_box(b, self.volume_dims())

    def stats_lut(self, stats_tensor, kind: int, channels: int = 0xF, stream=None, out=None):
        """A table from the histograms of a device vr_volume_stats, on the device
        (vr_stats_lut_device): `stats_tensor` is what :meth:`brush_stats` /
        :meth:`box_stats` wrote with `out` (a CUDA uint8 tensor of 8240 bytes,
        8-byte aligned); the result -- bit for bit :func:`stats_lut`'s -- goes
        to `out`, a contiguous CUDA uint8 tensor of 1024 elements (4-byte
        aligned; default: a new one shaped (4, 256)), which is returned and is
        what :meth:`remap` takes.  One launch queued on `stream`, nothing
        waits: ``brush_stats -> stats_lut -> remap -> update_footprint ->
        render_rect`` runs on one stream with no host round trip.  No volume
        is needed."""
        dev = torch.device("cuda", self.device)
        if (not isinstance(stats_tensor, torch.Tensor) or not stats_tensor.is_cuda or stats_tensor.device.index != self.device
                or stats_tensor.dtype != torch.uint8 or stats_tensor.numel() != VOLUME_STATS_BYTES
                or not stats_tensor.is_contiguous()):
            raise ValueError(f"stats_lut: stats must be a contiguous uint8 tensor of {VOLUME_STATS_BYTES} bytes on cuda:{self.device}")
        if out is None:
            out = torch.empty((4, 256), dtype=torch.uint8, device=dev)
        elif (not isinstance(out, torch.Tensor) or not out.is_cuda or out.device.index != self.device
                or out.dtype != torch.uint8 or out.numel() != LUT_BYTES or not out.is_contiguous()):
            raise ValueError(f"stats_lut: out must be a contiguous uint8 tensor of {LUT_BYTES} elements on cuda:{self.device}")
        call("vr_stats_lut_device", self._ctx, ctypes.c_void_p(stats_tensor.data_ptr()), int(kind), int(channels),
             ctypes.c_void_p(out.data_ptr()), _stream_handle(stream))
        return out

    def get_volume_box(self, origin, extent, out=None, stream=None):
        """The texel box `extent` = (bx, by, bz) at `origin` = (x0, y0, z0) of the
        installed volume, shaped (bz, by, bx, 4) -- what :meth:`update_volume`
        takes back (undo: save the box, paint, update_volume the saved box).
        With no `out` and no `stream`: a numpy array, through the synchronous
        host call (vr_get_volume_box).  With `out` a CUDA uint8 tensor of that
        shape, or a `stream`: a CUDA tensor, written on `stream` (default: the
        current stream, which is then waited for) by vr_get_volume_box_device."""
        x0, y0, z0 = (int(v) for v in origin)
        bx, by, bz = (int(v) for v in extent)
        shape = (max(bz, 0), max(by, 0), max(bx, 0), 4)
        if isinstance(out, torch.Tensor) or (out is None and stream is not None):
            if out is None:
                out = torch.empty(shape, dtype=torch.uint8, device=torch.device("cuda", self.device))
            if (not out.is_cuda or out.device.index != self.device or out.dtype != torch.uint8
                    or tuple(out.shape) != shape or not out.is_contiguous()):
                raise ValueError(f"get_volume_box: out must be a contiguous uint8 tensor {shape} on cuda:{self.device}")
            # an empty box has no buffer to hand over: the library refuses the extent either way
            ptr = ctypes.c_void_p(out.data_ptr()) if out.numel() else ctypes.c_void_p(1)
            call("vr_get_volume_box_device", self._ctx, x0, y0, z0, bx, by, bz, ptr, _stream_handle(stream))
            if stream is None:
                torch.cuda.current_stream().synchronize()
            return out
        if out is None:
            out = np.empty(shape, np.uint8)
        if (not isinstance(out, np.ndarray) or out.dtype != np.uint8 or out.shape != shape
                or not out.flags.c_contiguous or not out.flags.writeable):
            raise ValueError(f"get_volume_box: out must be a writeable contiguous uint8 array {shape}")
        call("vr_get_volume_box", self._ctx, x0, y0, z0, bx, by, bz, out.ctypes.data_as(ctypes.c_void_p))
        return out

    def generate_volume(self, recipe: VolumeRecipe | None = None) -> None:
        """Build the TestMain.cpp:43-92 volume on the GPU."""
        r = recipe if recipe is not None else volume_recipe_defaults()
        call("vr_generate_volume", self._ctx, ctypes.byref(r), _stream_handle(None))

    def get_volume(self) -> np.ndarray:
        nx, ny, nz = self.volume_dims()
        out = np.empty((nz, ny, nx, 4), np.uint8)
        call("vr_get_volume", self._ctx, out.ctypes.data_as(ctypes.c_void_p))
        return out

    def volume_dims(self):
        nx, ny, nz = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        call("vr_volume_dims", self._ctx, ctypes.byref(nx), ctypes.byref(ny), ctypes.byref(nz))
        return nx.value, ny.value, nz.value

    def noise_grid(self, kind: int, nx: int, ny: int, nz: int, freq: float, seed: int,
                   origin=(0, 0, 0), out: torch.Tensor | None = None):
        """One GenUniformGrid3D on the GPU -> (tensor or None, min, max)."""
        mn, mx = ctypes.c_float(), ctypes.c_float()
        ptr = ctypes.c_void_p(out.data_ptr()) if out is not None else None
        call("vr_noise_grid", self._ctx, int(kind), ptr, origin[0], origin[1], origin[2], nx, ny, nz,
             ctypes.c_float(freq), int(seed), ctypes.byref(mn), ctypes.byref(mx), _stream_handle(None))
        return out, mn.value, mx.value

    # -- uniforms / constants ----------------------------------------------
    def set_shader_data(self, osd: ObjectShaderData, gsd: GlobalShaderData) -> None:
        call("vr_set_shader_data", self._ctx, ctypes.byref(osd), ctypes.byref(gsd))
        self.osd, self.gsd = osd, gsd

    def set_march(self, m: MarchParams | None = None, **overrides) -> None:
        m = m if m is not None else march_defaults(**overrides)
        call("vr_set_march", self._ctx, ctypes.byref(m))
        self.march = m

    def selftest(self, name: str) -> int:
        """Mismatch count of a device arithmetic shortcut (vr_selftest)."""
        n = ctypes.c_longlong()
        call("vr_selftest", self._ctx, name.encode(), ctypes.byref(n))
        return int(n.value)

    def set_procedural(self, p: Procedural | None = None, **overrides) -> None:
        """Enable the procedural medium (configs 2/3); pass enabled=0 to return to the volume."""
        p = p if p is not None else procedural_defaults(**overrides)
        call("vr_set_procedural", self._ctx, ctypes.byref(p))
        self.procedural = p

    def set_layout_preference(self, pref: int) -> None:
        call("vr_set_layout_preference", self._ctx, int(pref))

    def set_option(self, name: str, value: int) -> None:
        """Tuning knobs of vr_set_option: "layout", "schedule", "waves_per_simd"."""
        call("vr_set_option", self._ctx, name.encode(), int(value))

    def get_option(self, name: str) -> int:
        return _lib.load().vr_get_option(self._ctx, name.encode())

    @property
    def kernel_variant(self) -> str:
        return _lib.load().vr_kernel_variant(self._ctx).decode()

    def measure_copy_bandwidth(self, nbytes: int = 2 << 30, reps: int = 10, stream=None) -> tuple[float, float]:
        """(best, median) GB/s of the device's 16-B-per-lane streaming copy
        (read + written bytes): the measured HBM roofline (vr.h)."""
        best, med = ctypes.c_double(), ctypes.c_double()
        _lib.call("vr_measure_copy_bandwidth", self._ctx, nbytes, reps, _stream_handle(stream), ctypes.byref(best),
                  ctypes.byref(med))
        return best.value, med.value

    def measure_bandwidth(self, kind: str = "read", loads_per_lane: int = 0, nbytes: int = 2 << 30, reps: int = 10,
                          stream=None) -> tuple[float, float, int]:
        """(best, median GB/s, loads per lane of the best) of a one-pass 16-B-per-lane
        stream over `nbytes` (vr_measure_bandwidth): kind "read" (loads only, bytes
        read / time) or "copy" (read + written bytes / time); loads_per_lane 4, 8,
        16, or 0 = each of them."""
        k = {"copy": 0, "read": 1}[kind]
        best, med, pl = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
        _lib.call("vr_measure_bandwidth", self._ctx, k, int(loads_per_lane), nbytes, reps, _stream_handle(stream),
                  ctypes.byref(best), ctypes.byref(med), ctypes.byref(pl))
        return best.value, med.value, pl.value

    # -- the hot path ------------------------------------------------------
    def alloc_target(self, width: int, height: int, fmt: int = FMT_RGBA8_UNORM, band_rows: int = 0,
                     band_stride: int = 1, band_first: int = 0, band_flip: int = 0) -> torch.Tensor:
        """(rows, width, 4) for the RGBA formats, (rows, width) for the grey ones."""
        rows = band_rows_packed(height, band_rows, band_stride, band_first, band_flip)
        dev = torch.device("cuda", self.device)
        if fmt not in BYTES_PER_PIXEL:
            raise ValueError(f"unknown format {fmt}")
        shape = (rows, width, 4) if CHANNELS[fmt] == 4 else (rows, width)
        return torch.empty(shape, dtype=torch.float32 if fmt in FLOAT_FORMATS else torch.uint8, device=dev)

    def _check_target(self, width: int, height: int, fmt: int, out: torch.Tensor, band_rows: int,
                      band_stride: int, band_first: int, step_counter: torch.Tensor | None = None,
                      band_flip: int = 0) -> None:
        """The kernel writes band_rows_packed(...) rows of `width` pixels of
        BYTES_PER_PIXEL[fmt] bytes through a raw pointer: refuse any tensor it
        would write past, or that lives on another device."""
        if fmt not in BYTES_PER_PIXEL:
            raise ValueError(f"unknown format {fmt}")
        if not isinstance(out, torch.Tensor) or not out.is_cuda or out.device.index != self.device:
            raise ValueError(f"render target must be a tensor on cuda:{self.device}")
        want_dtype = torch.float32 if fmt in FLOAT_FORMATS else torch.uint8
        if out.dtype != want_dtype:
            raise ValueError(f"format {fmt} needs a {want_dtype} target, got {out.dtype}")
        rows = band_rows_packed(height, band_rows, band_stride, band_first, band_flip)
        if CHANNELS[fmt] == 4:
            if out.dim() != 3 or out.shape[0] < rows or out.shape[1] != width or out.shape[2] != 4:
                raise ValueError(f"render target must be shaped ({rows}, {width}, 4) (at least {rows} rows), "
                                 f"got {tuple(out.shape)}")
            if out.stride(2) != 1 or out.stride(1) != 4 or out.stride(0) < 4 * width:
                raise ValueError("render target rows must be contiguous RGBA pixels (strides (>=4*width, 4, 1))")
        else:
            if out.dim() != 2 or out.shape[0] < rows or out.shape[1] != width:
                raise ValueError(f"grey render target must be shaped ({rows}, {width}) (at least {rows} rows), "
                                 f"got {tuple(out.shape)}")
            if out.stride(1) != 1 or out.stride(0) < width:
                raise ValueError("grey render target rows must be contiguous (strides (>=width, 1))")
        if step_counter is not None and (step_counter.dtype != torch.int64 or not step_counter.is_cuda
                                         or step_counter.device.index != self.device
                                         or step_counter.numel() < 1):
            raise ValueError(f"step_counter must be an int64 tensor on cuda:{self.device}")

    def render(self, width: int, height: int, fmt: int = FMT_RGBA8_UNORM, out: torch.Tensor | None = None,
               band_rows: int = 0, band_stride: int = 1, band_first: int = 0, stream=None,
               step_counter: torch.Tensor | None = None, band_flip: int = 0) -> torch.Tensor:
        """Launch the march kernel (asynchronous on `stream`); returns `out`.
        band_flip: the set's odd bands shifted (vr.h vr_target.band_flip)."""
        if out is None:
            out = self.alloc_target(width, height, fmt, band_rows, band_stride, band_first, band_flip)
        self._check_target(width, height, fmt, out, band_rows, band_stride, band_first, step_counter, band_flip)
        t = Target(width=width, height=height, format=fmt, band_rows=band_rows, band_stride=band_stride,
                   band_first=band_first, pixels=out.data_ptr(), row_pitch=out.stride(0) * out.element_size(),
                   step_counter=step_counter.data_ptr() if step_counter is not None else None,
                   band_flip=band_flip)
        call("vr_render", self._ctx, ctypes.byref(t), _stream_handle(stream))
        return out

    def render_pair(self, width: int, height: int, fmt: int, out0: torch.Tensor, out1: torch.Tensor, cameras=None,
                    band_rows: int = 0, band_stride: int = 1, band_first: int = 0, stream=None,
                    step_counter: torch.Tensor | None = None, band_flip: int = 0, row_pitch: int | None = None):
        """Two queued frames in one launch (vr_render_pair): frame i into `outi`
        with cameras[i] = (ObjectShaderData, GlobalShaderData); cameras None =
        both with the current shader data.  The same bytes as set_shader_data +
        render per frame; the renderer ends holding cameras[1]."""
        for out in (out0, out1):
            self._check_target(width, height, fmt, out, band_rows, band_stride, band_first, step_counter, band_flip)
        ts = [Target(width=width, height=height, format=fmt, band_rows=band_rows, band_stride=band_stride,
                     band_first=band_first, pixels=out.data_ptr(),
                     row_pitch=out.stride(0) * out.element_size() if row_pitch is None else row_pitch,
                     step_counter=step_counter.data_ptr() if step_counter is not None else None, band_flip=band_flip)
              for out in (out0, out1)]
        osd = gsd = None
        if cameras is not None:
            cams = list(cameras)
            if len(cams) != 2:
                raise ValueError(f"render_pair: two cameras, got {len(cams)}")
            osd = (ObjectShaderData * 2)(cams[0][0], cams[1][0])
            gsd = (GlobalShaderData * 2)(cams[0][1], cams[1][1])
        call("vr_render_pair", self._ctx, ctypes.byref(ts[0]), ctypes.byref(ts[1]), osd, gsd, _stream_handle(stream))
        return out0, out1

    def render_group(self, width: int, height: int, fmt: int, outs, cameras=None, band_rows: int = 0,
                     band_stride: int = 1, band_first: int = 0, stream=None, step_counter: torch.Tensor | None = None,
                     band_flip: int = 0, row_pitch: int | None = None):
        """len(outs) = 1..4 queued frames (vr_render_group): frame i into outs[i] with
        cameras[i] = (ObjectShaderData, GlobalShaderData); cameras None = all with the
        current shader data.  Four frames are one launch where a grouped kernel applies,
        three a pair and a plain render.  The same bytes as set_shader_data + render per
        frame; the renderer ends holding the last camera."""
        outs = list(outs)
        n = len(outs)
        if not 1 <= n <= 4:
            raise ValueError(f"render_group: 1 to 4 targets, got {n}")
        for out in outs:
            self._check_target(width, height, fmt, out, band_rows, band_stride, band_first, step_counter, band_flip)
        ts = (Target * n)(*[Target(width=width, height=height, format=fmt, band_rows=band_rows, band_stride=band_stride,
                                   band_first=band_first, pixels=out.data_ptr(),
                                   row_pitch=out.stride(0) * out.element_size() if row_pitch is None else row_pitch,
                                   step_counter=step_counter.data_ptr() if step_counter is not None else None,
                                   band_flip=band_flip) for out in outs])
        osd = gsd = None
        if cameras is not None:
            cams = list(cameras)
            if len(cams) != n:
                raise ValueError(f"render_group: {n} cameras, got {len(cams)}")
            osd = (ObjectShaderData * n)(*[c[0] for c in cams])
            gsd = (GlobalShaderData * n)(*[c[1] for c in cams])
        call("vr_render_group", self._ctx, ts, n, osd, gsd, _stream_handle(stream))
        return tuple(outs)

    def render_rect(self, out: torch.Tensor, rect, fmt: int = FMT_RGBA8_UNORM,
                    step_counter: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        """Render the pixels rect = (x, y, w, h) of the whole-frame target `out`
        (vr_render_rect, the scissor): they get what :meth:`render` writes
        there, bit for bit, and nothing else of `out` is touched.  The frame
        size is `out`'s.  Asynchronous on `stream`; the cost follows the
        rectangle."""
        if not isinstance(out, torch.Tensor) or out.dim() < 2:
            raise ValueError("render_rect needs a whole-frame target tensor (height, width[, 4])")
        height, width = int(out.shape[0]), int(out.shape[1])
        self._check_target(width, height, fmt, out, 0, 1, 0, step_counter)
        x, y, w, h = (int(v) for v in rect)
        t = Target(width=width, height=height, format=fmt, band_rows=0, band_stride=1, band_first=0,
                   pixels=out.data_ptr(), row_pitch=out.stride(0) * out.element_size(),
                   step_counter=step_counter.data_ptr() if step_counter is not None else None)
        r = Rect(x, y, w, h)
        call("vr_render_rect", self._ctx, ctypes.byref(t), ctypes.byref(r), _stream_handle(stream))
        return out

    def render_rects(self, out: torch.Tensor, rects, fmt: int = FMT_RGBA8_UNORM,
                     step_counter: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        """Render the union of `rects` -- a sequence of (x, y, w, h) tuples or
        :class:`Rect` -- into the whole-frame target `out` in one launch
        (vr_render_rects).  The rectangles may overlap, repeat, contain one
        another and be empty; a pixel several of them cover is marched, stored
        and counted once.  At most VR_MAX_RECTS of them: :func:`coalesce_rects`
        shortens a longer list.  Otherwise as :meth:`render_rect`."""
        if not isinstance(out, torch.Tensor) or out.dim() < 2:
            raise ValueError("render_rects needs a whole-frame target tensor (height, width[, 4])")
        height, width = int(out.shape[0]), int(out.shape[1])
        self._check_target(width, height, fmt, out, 0, 1, 0, step_counter)
        arr = _rect_array(rects)
        t = Target(width=width, height=height, format=fmt, band_rows=0, band_stride=1, band_first=0,
                   pixels=out.data_ptr(), row_pitch=out.stride(0) * out.element_size(),
                   step_counter=step_counter.data_ptr() if step_counter is not None else None)
        call("vr_render_rects", self._ctx, ctypes.byref(t), arr, len(arr), _stream_handle(stream))
        return out

    def update_footprints(self, boxes, width: int, height: int) -> list[tuple[int, int, int, int]]:
        """:meth:`update_footprint` of every (origin, extent) pair of `boxes`:
        one rectangle per box, in order.  `update_volume` each box, then one
        `render_rects` of these into a frame rendered before the updates,
        gives the patched volume's whole frame."""
        return [self.update_footprint(origin, extent, width, height) for origin, extent in boxes]

    def update_footprint(self, origin, extent, width: int, height: int) -> tuple[int, int, int, int]:
        """vr_update_footprint: the rectangle (x, y, w, h) of the width x height
        frame that an :meth:`update_volume` of the texel box `extent` = (bx, by,
        bz) at `origin` = (x0, y0, z0) can change, for the current shader data
        and march constants.  `update_volume(box)`, then `render_rect` of it
        into a frame rendered before the update, gives the patched volume's
        whole frame."""
        x0, y0, z0 = (int(v) for v in origin)
        bx, by, bz = (int(v) for v in extent)
        r = Rect()
        call("vr_update_footprint", self._ctx, int(width), int(height), x0, y0, z0, bx, by, bz, ctypes.byref(r))
        return r.x, r.y, r.width, r.height

    def query_rect(self, rect, width: int, height: int, threshold: float = 0.0, stream=None,
                   out: torch.Tensor | None = None) -> torch.Tensor:
        """vr_query_rect: the ray records of the pixels rect = (x, y, w, h) of
        the width x height frame, as a ``torch.int32`` tensor [h, w, 16] on the
        GPU (one vr_ray_record per pixel; :func:`ray_records` names its fields
        on the host).  ``value`` is :meth:`render`'s FMT_R32F pixel bit for bit;
        ``threshold`` (a transmittance, as march.early_out; 0 = off) selects
        ``hit_step`` / ``hit``.  `out`: an int32 tensor [>= h, >= w, 16] on this
        device with contiguous records to write into (its rows may be wider
        than the rectangle; only the rectangle's records are written).
        Asynchronous on `stream`."""
        x, y, w, h = (int(v) for v in rect)
        if out is None:
            out = torch.empty((max(h, 0), max(w, 0), RAY_RECORD_WORDS), dtype=torch.int32,
                              device=torch.device("cuda", self.device))
            if out.numel() == 0:   # no buffer to hand over: validate with a one-record stand-in, which stays unwritten
                spare = torch.empty((1, 1, RAY_RECORD_WORDS), dtype=torch.int32, device=out.device)
                call("vr_query_rect", self._ctx, int(width), int(height), ctypes.byref(Rect(x, y, w, h)),
                     ctypes.c_float(threshold), ctypes.c_void_p(spare.data_ptr()), 0, _stream_handle(stream))
                return out
        if (not isinstance(out, torch.Tensor) or not out.is_cuda or out.device.index != self.device
                or out.dtype != torch.int32 or out.dim() != 3 or out.shape[2] != RAY_RECORD_WORDS
                or out.stride(2) != 1 or out.stride(1) != RAY_RECORD_WORDS or out.stride(0) % RAY_RECORD_WORDS != 0
                or out.shape[0] < h or out.shape[1] < w or out.stride(0) < out.shape[1] * RAY_RECORD_WORDS):
            raise ValueError(f"query_rect: out must be an int32 tensor (>= {h}, >= {w}, {RAY_RECORD_WORDS}) on "
                             f"cuda:{self.device} with contiguous records")
        call("vr_query_rect", self._ctx, int(width), int(height), ctypes.byref(Rect(x, y, w, h)),
             ctypes.c_float(threshold), ctypes.c_void_p(out.data_ptr()), out.stride(0) // RAY_RECORD_WORDS,
             _stream_handle(stream))
        return out

    def pick(self, x: int, y: int, width: int, height: int, threshold: float):
        """The ray of pixel (x, y) of the width x height frame (a 1 x 1
        :meth:`query_rect`; waits for it): ``(record, texel)``.  `record` is
        the pixel's vr_ray_record as a numpy record.  `texel` is None unless the
        ray has a hit (``hit_step >= 0``) and a volume is installed; then it is
        the texel (ix, iy, iz) of tap 0 (frag.glsl:66: Pin + MediaScroll[.].x *
        tap_weight[0], scaled by tap_scale[0]) that ``hit`` falls in, clamped to
        the volume -- where an editor paints."""
        rec = ray_records(self.query_rect((x, y, 1, 1), width, height, threshold))[0, 0]
        if rec["hit_step"] < 0:
            return rec, None
        try:
            dims = self.volume_dims()
        except VRError:
            return rec, None
        if min(dims) <= 0:
            return rec, None
        gsd = getattr(self, "gsd", None)
        texel = []
        for ax in range(3):
            off = float(gsd.media_scroll[ax * 4 + 0]) * float(self.march.tap_weight[0]) if gsd is not None else 0.0
            u = float(rec["hit"][ax]) * float(self.march.tap_scale[0]) + off
            texel.append(int(min(max(np.floor(u * dims[ax]), 0), dims[ax] - 1)))
        return rec, tuple(texel)

    def render_rows(self, width: int, height: int, fmt: int, first_row: int, rows: int,
                    out: torch.Tensor | None = None, in_place: bool = False, stream=None) -> torch.Tensor:
        """Frame rows [first_row, first_row + rows) of the width x height frame
        (vr.h VR_TARGET_ROW_RANGE; first_row a multiple of 8): packed from row
        0 of `out`, or at their own rows of a whole-frame `out` (in_place)."""
        n = max(0, min(rows, height - first_row))
        if out is None:
            out = self.alloc_target(width, height if in_place else n, fmt)
        self._check_target(width, height if in_place else n, fmt, out, 0, 1, 0)
        flags = _lib.TARGET_ROW_RANGE | (_lib.TARGET_BANDS_IN_PLACE if in_place else 0)
        t = Target(width=width, height=height, format=fmt | flags, band_rows=rows, band_stride=1,
                   band_first=first_row, pixels=out.data_ptr(), row_pitch=out.stride(0) * out.element_size(),
                   step_counter=None)
        call("vr_render", self._ctx, ctypes.byref(t), _stream_handle(stream))
        return out

    def row_partition(self, width: int, height: int, parts: int) -> list[int]:
        """vr_row_partition: parts + 1 row starts of contiguous ranges of equal
        estimated march work for the current camera."""
        rb = (ctypes.c_int * (parts + 1))()
        call("vr_row_partition", self._ctx, width, height, parts, rb)
        return list(rb)

    def row_work(self, width: int, height: int) -> list[float]:
        """The estimated march work of every 8-row strip (vr_row_work: the
        model vr_row_partition splits and vr_shard_balance_lead sizes rank 0's
        lead rows from)."""
        ns = (height + 7) // 8
        out = (ctypes.c_double * ns)()
        call("vr_row_work", self._ctx, width, height, out, ns)
        return list(out)

    def row_partition_measured(self, width: int, height: int, prev: list[int], prev_ms: list[float]) -> list[int]:
        """vr_row_partition_measured: the split again, range k of `prev` having
        taken prev_ms[k]."""
        parts = len(prev) - 1
        rb = (ctypes.c_int * (parts + 1))()
        call("vr_row_partition_measured", self._ctx, width, height, parts, (ctypes.c_int * (parts + 1))(*prev),
             (ctypes.c_double * parts)(*prev_ms), rb)
        return list(rb)

    def render_sequence(self, width: int, height: int, fmt: int, out: torch.Tensor, cameras, band_rows: int = 0,
                        band_stride: int = 1, band_first: int = 0, stream=None) -> torch.Tensor:
        """The reference's frame loop with a moving camera (TestMain.cpp:173-256):
        one render per (ObjectShaderData, GlobalShaderData) of `cameras`, all
        into `out`, queued natively (vr_render_sequence) without host waits."""
        self._check_target(width, height, fmt, out, band_rows, band_stride, band_first)
        cams = list(cameras)
        osd = (ObjectShaderData * max(1, len(cams)))(*[c[0] for c in cams])
        gsd = (GlobalShaderData * max(1, len(cams)))(*[c[1] for c in cams])
        t = Target(width=width, height=height, format=fmt, band_rows=band_rows, band_stride=band_stride,
                   band_first=band_first, pixels=out.data_ptr(), row_pitch=out.stride(0) * out.element_size(),
                   step_counter=None)
        call("vr_render_sequence", self._ctx, ctypes.byref(t), len(cams), osd, gsd, _stream_handle(stream))
        return out

    def prepare_render(self, width: int, height: int, fmt: int, out: torch.Tensor, band_rows: int = 0,
                       band_stride: int = 1, band_first: int = 0, stream=None):
        """A zero-argument launcher for one fixed render (target, bands,
        stream): the ctypes arguments are built once, so a frame loop pays
        only the call (host time per frame bounds multi-GPU strong scaling)."""
        self._check_target(width, height, fmt, out, band_rows, band_stride, band_first)
        t = Target(width=width, height=height, format=fmt, band_rows=band_rows, band_stride=band_stride,
                   band_first=band_first, pixels=out.data_ptr(), row_pitch=out.stride(0) * out.element_size(),
                   step_counter=None)
        fn, ctx, tref, sh = _lib.load().vr_render, self._ctx, ctypes.byref(t), _stream_handle(stream)

        def launch():
            st = fn(ctx, tref, sh)
            if st:
                _lib.check(st, "vr_render")
        launch.target = t   # keep the struct and the target tensor alive with the closure
        launch.out = out
        return launch

    def prepare_assemble(self, gathered: torch.Tensor, nranks: int, width: int, height: int, band_rows: int,
                         frame: torch.Tensor, stream=None):
        """Zero-argument launcher for one fixed vr_assemble_bands call."""
        self._check_assemble(gathered, nranks, width, height, band_rows, frame)
        bpp = gathered.element_size() * gathered.shape[-1]
        args = (self._ctx, ctypes.c_void_p(gathered.data_ptr()), gathered.shape[1], nranks, width, height, band_rows,
                bpp, ctypes.c_void_p(frame.data_ptr()), _stream_handle(stream))
        fn = _lib.load().vr_assemble_bands

        def launch():
            st = fn(*args)
            if st:
                _lib.check(st, "vr_assemble_bands")
        launch.keep = (gathered, frame)
        return launch

    def _check_assemble_frame(self, gathered: torch.Tensor, gfmt: int, nranks: int, width: int, height: int,
                              frame: torch.Tensor, ffmt: int) -> None:
        for name, t in (("gathered", gathered), ("frame", frame)):
            if not t.is_cuda or t.device.index != self.device or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous tensor on cuda:{self.device}")
        if gfmt != ffmt and GREY_OF.get(ffmt) != gfmt:
            raise ValueError(f"band sets in format {gfmt} do not expand into format {ffmt}")
        gshape = (width, 4) if CHANNELS[gfmt] == 4 else (width,)
        gdtype = torch.float32 if gfmt in FLOAT_FORMATS else torch.uint8
        if gathered.dim() != 2 + len(gshape) or gathered.shape[0] < nranks or tuple(gathered.shape[2:]) != gshape \
                or gathered.dtype != gdtype:
            raise ValueError(f"gathered must be a {gdtype} tensor shaped (>= {nranks}, rows, {gshape}), "
                             f"got {gathered.dtype} {tuple(gathered.shape)}")
        fdtype = torch.float32 if ffmt in FLOAT_FORMATS else torch.uint8
        fshape = (height, width, 4) if CHANNELS[ffmt] == 4 else (height, width)
        if frame.dtype != fdtype or tuple(frame.shape) != fshape:
            raise ValueError(f"frame must be a {fdtype} tensor shaped {fshape}")

    def assemble_frame(self, gathered: torch.Tensor, gathered_fmt: int, nranks: int, width: int, height: int,
                       band_rows: int, frame_fmt: int, frame: torch.Tensor | None = None, stream=None,
                       serpentine: bool = False) -> torch.Tensor:
        """vr_assemble_frame: [rank][packed rows] band sets in `gathered_fmt`
        (e.g. grey) scattered and expanded into a `frame_fmt` frame.
        serpentine: rank r rendered with band_flip nranks-1-2r
        (VR_ASSEMBLE_SERPENTINE)."""
        if frame is None:
            shape = (height, width, 4) if CHANNELS[frame_fmt] == 4 else (height, width)
            frame = torch.empty(shape, dtype=torch.float32 if frame_fmt in FLOAT_FORMATS else torch.uint8,
                                device=gathered.device)
        self._check_assemble_frame(gathered, gathered_fmt, nranks, width, height, frame, frame_fmt)
        call("vr_assemble_frame", self._ctx, ctypes.c_void_p(gathered.data_ptr()), gathered_fmt, gathered.shape[1],
             nranks, width, height, band_rows, frame_fmt | (_lib.ASSEMBLE_SERPENTINE if serpentine else 0),
             ctypes.c_void_p(frame.data_ptr()), _stream_handle(stream))
        return frame

    def prepare_assemble_frame(self, gathered: torch.Tensor, gathered_fmt: int, nranks: int, width: int, height: int,
                               band_rows: int, frame_fmt: int, frame: torch.Tensor, stream=None):
        """Zero-argument launcher for one fixed vr_assemble_frame call."""
        self._check_assemble_frame(gathered, gathered_fmt, nranks, width, height, frame, frame_fmt)
        args = (self._ctx, ctypes.c_void_p(gathered.data_ptr()), gathered_fmt, gathered.shape[1], nranks, width,
                height, band_rows, frame_fmt, ctypes.c_void_p(frame.data_ptr()), _stream_handle(stream))
        fn = _lib.load().vr_assemble_frame

        def launch():
            st = fn(*args)
            if st:
                _lib.check(st, "vr_assemble_frame")
        launch.keep = (gathered, frame)
        return launch

    def _check_assemble(self, gathered: torch.Tensor, nranks: int, width: int, height: int, band_rows: int,
                        frame: torch.Tensor) -> None:
        for name, t in (("gathered", gathered), ("frame", frame)):
            if not t.is_cuda or t.device.index != self.device or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous tensor on cuda:{self.device}")
        if gathered.dim() != 4 or gathered.shape[0] < nranks or gathered.shape[2] != width or gathered.shape[3] != 4:
            raise ValueError(f"gathered must be shaped (>= {nranks}, rows, {width}, 4), got {tuple(gathered.shape)}")
        if frame.dtype != gathered.dtype or tuple(frame.shape) != (height, width, 4):
            raise ValueError(f"frame must be a {gathered.dtype} tensor shaped ({height}, {width}, 4)")

    def assemble_bands(self, gathered: torch.Tensor, nranks: int, width: int, height: int, band_rows: int,
                       frame: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        """Scatter [rank][packed rows] band sets into one frame (SURVEY.md e)."""
        bpp = gathered.element_size() * gathered.shape[-1]
        rows_per_rank = gathered.shape[1]
        if frame is None:
            frame = torch.empty((height, width, gathered.shape[-1]), dtype=gathered.dtype, device=gathered.device)
        self._check_assemble(gathered, nranks, width, height, band_rows, frame)
        call("vr_assemble_bands", self._ctx, ctypes.c_void_p(gathered.data_ptr()), rows_per_rank, nranks,
             width, height, band_rows, bpp, ctypes.c_void_p(frame.data_ptr()), _stream_handle(stream))
        return frame
