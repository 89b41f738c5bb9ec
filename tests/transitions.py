"""State-transition harness shared by test_gpu_transitions.py (one long-lived
Renderer against the oracle) and test_transitions_cpu.py (the harness's own
conditions, oracle only).

A Scene is a plain record of everything that determines a frame.  apply()
calls only the setters whose inputs differ between two scenes, expected()
cuts a target's rows out of the oracle's whole frame, and check() renders one
scene into a sentinel-filled, padded buffer and compares every byte.

Nothing here needs a GPU to import: the parameter lists are the same on every
machine.
"""
from __future__ import annotations

import ctypes
import zlib
from dataclasses import dataclass, field, replace

import numpy as np

from volumetricrenderer_amd import _lib
from volumetricrenderer_amd._lib import BYTES_PER_PIXEL, CHANNELS, FLOAT_FORMATS

W0, H0, STEPS0 = 96, 112, 48
ASPECT0 = W0 / H0
SRGB_FORMATS = (_lib.FMT_RGBA8_SRGB, _lib.FMT_R8_SRGB)
RGBA_OF = {0: 0, 1: 1, 2: 2, 3: 1, 4: 2, 5: 0}   # the RGBA format whose R a grey format holds (vr.h)
COUNTER_START = 1_000_003                         # check(): the step counter's value before the render
BYTE_SENTINEL = 0xAB

# options the walks change, with the library's defaults (vr_ctx.h)
OPTION_DEFAULTS = {"wedges": 0, "supertile": 2, "split": 0, "region_order": 2, "tiles_per_wave": 0, "uniform_skip": 1,
                   "empty_fill": 1, "region_gpu": 1, "schedule": -1, "shadow_defer": 1, "lattice": 1, "shadow_cache": 0,
                   "count": 0, "sort_reuse": 0, "wg_waves": 4}
EXPERIMENT_OPTIONS = ("sort_reuse", "wg_waves")   # non-default values: VR_EXPERIMENTS builds only


# ---- the record ---------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Target:
    W: int = W0
    H: int = H0
    fmt: int = 0
    band_rows: int = 16      # 0 = the whole frame; mode "range": the number of rows
    band_stride: int = 3
    band_first: int = 0      # mode "range": the first frame row
    band_flip: int = 0
    mode: str = "packed"     # "packed", "inplace" (VR_TARGET_BANDS_IN_PLACE), "range" (VR_TARGET_ROW_RANGE)
    pad: int = 0             # pixels per row between the rows of the buffer
    buf: int = 0             # which output buffer (same shape, another address)


@dataclass(frozen=True)
class Cam:
    """reference_shader_data(aspect, phi, theta) with edits.  The aspect is a
    field of its own (the base frame's), so that a width or height change of
    the target is a change of the target alone."""
    phi: float = 20.0
    theta: float = 15.0
    aspect: float = ASPECT0
    campos: tuple | None = None      # CameraPosition off the View eye
    translate: tuple | None = None   # Model = translate(t), W2L its inverse (test_ring_schedule_off_centre)
    scroll: tuple = ()               # ((axis, tap, value), ...) entries of MediaScroll


@dataclass(frozen=True)
class Scene:
    vol: str = "A"
    layout: int = 0
    cam: Cam = Cam()
    march: tuple = ()        # sorted (field, value) overrides of march_defaults(max_steps=48)
    proc: tuple | None = None   # None = the grid; else sorted overrides of procedural_defaults()
    opts: tuple = ()         # sorted (name, value) where it is not OPTION_DEFAULTS
    target: Target = field(default_factory=Target)


SCROLL_IN = ((1, 1, 0.01), (2, 2, -0.02))      # inside the clamp-exact range (the fast layouts stay)
SCROLL_OUT = ((0, 1, 3.7), (0, 2, -2.2), (1, 1, -0.6), (1, 3, -7.9), (2, 2, 0.4))   # far outside: planar mirror


def march_params(scene: Scene) -> _lib.MarchParams:
    m = _lib.MarchParams()
    _lib.call("vr_march_defaults", ctypes.byref(m))
    m.max_steps = STEPS0
    for k, v in scene.march:
        if isinstance(v, tuple):
            getattr(m, k)[:] = list(v)
        else:
            setattr(m, k, v)
    return m


def procedural_params(scene: Scene) -> _lib.Procedural:
    p = _lib.Procedural()
    _lib.call("vr_procedural_defaults", ctypes.byref(p))
    if scene.proc is None:
        p.enabled = 0
        return p
    p.enabled = 1
    for k, v in scene.proc:
        if isinstance(v, tuple):
            getattr(p, k)[:] = list(v)
        else:
            setattr(p, k, v)
    return p


def shader_data(cam: Cam):
    """(ObjectShaderData, GlobalShaderData) by the library's host producer."""
    osd, gsd = _lib.ObjectShaderData(), _lib.GlobalShaderData()
    phi, theta = (0.0, 0.0) if cam.translate else (cam.phi, cam.theta)
    _lib.call("vr_reference_shader_data", ctypes.c_float(cam.aspect), ctypes.c_float(phi), ctypes.c_float(theta),
              ctypes.c_float(0.0), ctypes.byref(osd), ctypes.byref(gsd))
    if cam.translate:
        for i, t in enumerate(cam.translate):
            osd.model[12 + i] = t
            gsd.world_to_local[12 + i] = -t
    if cam.campos:
        gsd.camera_position[:] = list(cam.campos)
    for axis, tap, v in cam.scroll:
        gsd.media_scroll[axis * 4 + tap] = v
    return osd, gsd


def shader_arrays(cam: Cam):
    osd, gsd = shader_data(cam)
    obj = np.frombuffer(bytes(osd), np.float32).copy()
    glob = np.frombuffer(bytes(gsd), np.float32).copy()
    return obj, glob


# ---- volumes ------------------------------------------------------------------------------------------------------

BOX_ORIGIN, BOX_SHAPE = (5, 3, 7), (9, 5, 7, 4)   # (x0, y0, z0), (bz, by, bx, 4): no edge on a 4- or 8-texel grid line
_volumes: dict[str, np.ndarray] = {}


def volume(name: str) -> np.ndarray:
    """A: random 24x20x28 RGBA, no uniform channel.  B: the same dimensions,
    other bytes.  C: 17x9x30.  AuG: A with G made uniform.  A+box: A with the
    off-grid sub-box overwritten (reached from A by update_volume)."""
    if not _volumes:
        rng = np.random.default_rng(20240)
        a = rng.integers(0, 256, size=(28, 20, 24, 4), dtype=np.uint8)
        _volumes["A"] = a
        _volumes["B"] = rng.integers(0, 256, size=(28, 20, 24, 4), dtype=np.uint8)
        _volumes["C"] = rng.integers(0, 256, size=(30, 9, 17, 4), dtype=np.uint8)
        g = a.copy()
        g[..., 1] = 57
        _volumes["AuG"] = g
        _volumes["box"] = rng.integers(0, 256, size=BOX_SHAPE, dtype=np.uint8)
        b = a.copy()
        x0, y0, z0 = BOX_ORIGIN
        bz, by, bx, _ = BOX_SHAPE
        b[z0:z0 + bz, y0:y0 + by, x0:x0 + bx] = _volumes["box"]
        _volumes["A+box"] = b
        for v in _volumes.values():
            v.setflags(write=False)
    return _volumes[name]


# ---- row mapping (vr.h vr_target; the model is serpentine_rows in test_gpu_parity.py) ------------------------------

def target_rows(t: Target) -> np.ndarray:
    """Frame row of each packed row the target writes, -1 for the rows of a
    partial last band past the frame (left untouched)."""
    if t.mode == "range":
        return np.arange(t.band_first, min(t.band_first + t.band_rows, t.H))
    if t.band_rows <= 0:
        return np.arange(t.H)
    nb = (t.H + t.band_rows - 1) // t.band_rows
    out, k = [], 0
    while True:
        b = t.band_first + k * t.band_stride + (t.band_flip if k % 2 else 0)
        if b >= nb:
            break
        out += [y if y < t.H else -1 for y in range(b * t.band_rows, (b + 1) * t.band_rows)]
        k += 1
    return np.array(out, dtype=np.int64)


def target_valid(t: Target) -> bool:
    """The conditions of vr_render on a target (and: it selects rows)."""
    if t.mode == "range":
        ok = t.band_rows > 0 and t.band_stride == 1 and t.band_first % 8 == 0 and t.band_flip == 0
    elif t.band_rows <= 0:
        ok = t.band_flip == 0 and t.mode == "packed"
    else:
        ok = t.band_stride >= 1 and t.band_first >= 0 and \
            (t.band_flip == 0 or (t.band_stride >= 2 and abs(t.band_flip) < t.band_stride))
    return bool(ok) and (target_rows(t) >= 0).any()


def in_place(t: Target) -> bool:
    return t.mode == "inplace" and t.band_rows > 0


def target_format_word(t: Target) -> int:
    return t.fmt | (_lib.TARGET_BANDS_IN_PLACE if in_place(t) else 0) | (_lib.TARGET_ROW_RANGE if t.mode == "range" else 0)


# ---- the oracle's whole frame, cached per distinct scene content ----------------------------------------------------

_frames: dict = {}
_strips: dict = {}


def _frame_key(scene: Scene, fmt3: int):
    m, p = march_params(scene), procedural_params(scene)
    obj, glob = shader_arrays(scene.cam)
    vol = None if scene.proc is not None else zlib.crc32(volume(scene.vol).tobytes())
    return (vol, obj.tobytes(), glob.tobytes(), bytes(m), bytes(p) if scene.proc is not None else None,
            scene.target.W, scene.target.H, fmt3)


def _oracle_render(oracle, scene: Scene, **band):
    """(image, steps, density evaluations or None) of the oracle, all H rows
    or one of its own band sets."""
    t = scene.target
    obj, glob = shader_arrays(scene.cam)
    m = oracle.from_params(march_params(scene))
    if scene.proc is None:
        return oracle.render(volume(scene.vol), obj, glob, m, t.W, t.H, RGBA_OF[t.fmt], **band) + (None,)
    p = oracle.procedural_from(procedural_params(scene))
    return oracle.render_procedural(p, obj, glob, m, t.W, t.H, RGBA_OF[t.fmt], with_evals=True, **band)


def oracle_strips(oracle, scene: Scene):
    """(steps, evaluations or None) per 8-row strip of the frame, counted by
    the oracle's own band renders (8 rows per band, one band per render): what
    early-out saves and what the shadow rays add depends on the medium, so
    oracle.step_counts does not give these."""
    t = scene.target
    key = _frame_key(scene, RGBA_OF[t.fmt])
    if key not in _strips:
        assert t.H % 8 == 0
        ns = t.H // 8
        parts = [_oracle_render(oracle, scene, band_rows=8, band_stride=ns, band_first=s) for s in range(ns)]
        img = _frames[key][0]   # (oracle_frame comes first)
        assert np.array_equal(np.concatenate([p[0] for p in parts]), img)
        steps = np.array([p[1] for p in parts], np.int64)
        evals = None if scene.proc is None else np.array([p[2] for p in parts], np.int64)
        _strips[key] = (steps, evals)
    return _strips[key]


def oracle_frame(oracle, scene: Scene):
    """(whole frame in the scene's RGBA format, executed steps per 8-row
    strip), cached per distinct scene content.  The oracle knows nothing of
    band_flip, in-place rows or pitch: it renders all H rows."""
    t = scene.target
    key = _frame_key(scene, RGBA_OF[t.fmt])
    if key not in _frames:
        assert t.H % 8 == 0
        img, total, _ = _oracle_render(oracle, scene)
        img.setflags(write=False)
        m = march_params(scene)
        if m.early_out == 0.0:
            # every covered ray runs its n steps (frag.glsl:46)
            obj, glob = shader_arrays(scene.cam)
            n = oracle.step_counts(obj, glob, oracle.from_params(m), t.W, t.H)
            steps = np.maximum(n, 0).sum(axis=1, dtype=np.int64).reshape(-1, 8).sum(axis=1)
        else:
            _frames[key] = (img, None)
            steps = oracle_strips(oracle, scene)[0]
        assert int(steps.sum()) == total
        _frames[key] = (img, steps)
    return _frames[key]


def option(scene: Scene, name: str) -> int:
    return dict(scene.opts).get(name, OPTION_DEFAULTS[name])


def expected(oracle, scene: Scene):
    """(rows, pixels, counter increment): the frame row of each packed row of
    the target (-1: past the frame), the selected rows' pixels (n x W x 4, or
    n x W for a grey format) and the executed steps over those rows -- density
    evaluations where option count is 1."""
    t = scene.target
    img, steps = oracle_frame(oracle, scene)
    rows = target_rows(t)
    sel = rows[rows >= 0]
    px = img[sel]
    if CHANNELS[t.fmt] == 1:
        px = px[..., 0]
    if option(scene, "count") == 1 and scene.proc is not None:
        steps = oracle_strips(oracle, scene)[1]
    strips = np.unique(sel // 8)
    assert np.array_equal(np.sort(sel), (strips[:, None] * 8 + np.arange(8)).ravel()), "whole 8-row strips only"
    return rows, px, int(steps[strips].sum())


def coverage(oracle, scene: Scene) -> float:
    obj, glob = shader_arrays(scene.cam)
    n = oracle.step_counts(obj, glob, oracle.from_params(march_params(scene)), scene.target.W, scene.target.H)
    return float((n >= 0).mean())


# ---- mutations ------------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Mutation:
    name: str
    part: str                # "target", "cam", "march", "proc", "opts", "vol", "layout", "medium"
    values: tuple            # the fields it sets, as sorted (field, value) pairs; "vol"/"layout"/"medium": the value
    pixels: bool = True      # False: the selected rows' expected pixels stay as they are

    def __call__(self, s: Scene) -> Scene:
        if self.part == "target":
            return replace(s, target=replace(s.target, **dict(self.values)))
        if self.part == "cam":
            return replace(s, cam=replace(s.cam, **dict(self.values)))
        if self.part in ("march", "proc", "opts"):
            cur = dict(getattr(s, self.part) or ())
            cur.update(dict(self.values))
            if self.part == "opts":
                cur = {k: v for k, v in cur.items() if v != OPTION_DEFAULTS[k]}
            return replace(s, **{self.part: tuple(sorted(cur.items()))})
        if self.part == "medium":   # grid <-> procedural on the same context
            return replace(s, proc=self.values)
        return replace(s, **{self.part: self.values})

    def is_set(self, s: Scene) -> bool:
        return self(s) == s


def _m(name, part, pixels=True, **kw):
    return Mutation(name, part, tuple(sorted(kw.items())), pixels)


TARGET_MUTATIONS = [
    _m("W97", "target", W=97), _m("H104", "target", H=104), _m("first1", "target", band_first=1),
    _m("stride2", "target", band_stride=2), _m("rows8", "target", band_rows=8), _m("flip2", "target", band_flip=2),
    _m("whole", "target", band_rows=0, band_stride=1, band_first=0, band_flip=0, mode="packed"),
    _m("inplace", "target", pixels=False, mode="inplace"),
    # rows [16, 64): 48 packed rows, like the base set (out_rows collides)
    _m("range16_64", "target", mode="range", band_rows=48, band_stride=1, band_first=16, band_flip=0),
    _m("fmt1", "target", fmt=1), _m("fmt2", "target", fmt=2), _m("fmt3", "target", fmt=3), _m("fmt4", "target", fmt=4),
    _m("fmt5", "target", fmt=5),
    _m("pad3", "target", pixels=False, pad=3), _m("otherbuf", "target", pixels=False, buf=1),
]
FLIP_BACK = _m("flip-2", "target", band_flip=-2)    # on the band_first = 2 bases
FLIP_OFF = _m("flip0", "target", band_flip=0)       # on the band_flip = 2 bases: the other direction
CAMERA_MUTATIONS = [
    _m("phi+1.6", "cam", phi=21.6), _m("theta-35", "cam", theta=-20.0), _m("campos", "cam", campos=(4.0, 2.0, 2.5)),
    _m("translate", "cam", translate=(0.9, -0.4, 0.2)),
]
SCROLL_MUTATIONS = [_m("scroll_in", "cam", scroll=SCROLL_IN), _m("scroll_out", "cam", scroll=SCROLL_OUT)]   # grid only
MARCH_MUTATIONS = [
    _m("steps47", "march", max_steps=47), _m("stepscale3", "march", step_scale=3.0), _m("density", "march", density=2.5),
    _m("scale", "march", scale=0.35), _m("boxmax", "march", box_max=(1.0, 0.75, 1.0)),
]
TAP_SCALE = _m("tapscale", "march", tap_scale=(1.0, 0.8, 0.6, 0.7))     # grid only: the procedural medium has no taps
TAP_WEIGHT = _m("tapweight", "march", tap_weight=(0.0, 0.2, 0.4, 0.3))   # on the scroll bases: it scales MediaScroll
EARLY_OUT = _m("early0.3", "march", early_out=0.3)                       # on the dense bases (see BASES)
VOLUME_MUTATIONS = [Mutation("volB", "vol", "B"), Mutation("volC", "vol", "C"), Mutation("volAuG", "vol", "AuG"),
                    Mutation("update_box", "vol", "A+box")]
LAYOUTS = (0, 1, 12, 14, 15)
GRID_OPTION_MUTATIONS = [
    _m("wedges3", "opts", False, wedges=3), _m("supertile1", "opts", False, supertile=1), _m("split2", "opts", False, split=2),
    _m("region_order0", "opts", False, region_order=0), _m("tpw1", "opts", False, tiles_per_wave=1),
    _m("uniform_skip0", "opts", False, uniform_skip=0), _m("empty_fill0", "opts", False, empty_fill=0),
    _m("region_gpu0", "opts", False, region_gpu=0), _m("schedule0", "opts", False, schedule=0),
    _m("schedule4", "opts", False, schedule=4),
]
GRID_EXPERIMENTS = [_m("wg_waves8", "opts", False, wg_waves=8), _m("wg_waves16", "opts", False, wg_waves=16)]
PROC_FIELD_MUTATIONS = [
    _m("grid_scale", "proc", grid_scale=96.0), _m("octaves", "proc", octaves=3), _m("freq0", "proc", freq0=0.23),
    _m("lacunarity", "proc", lacunarity=2.3), _m("gain", "proc", gain=0.6), _m("seed_fbm", "proc", seed_fbm=11),
    _m("worley_freq", "proc", worley_freq=0.04), _m("seed_worley", "proc", seed_worley=9),
]
SUN_DIR = _m("sun_dir", "proc", sun_dir=(-1.0, 0.5, 0.25))              # read only with shadow rays
PROC_OPTION_MUTATIONS = [
    _m("lattice0", "opts", False, lattice=0), _m("count1", "opts", False, count=1), _m("schedule0", "opts", False, schedule=0),
    _m("schedule4", "opts", False, schedule=4),
]
SHADOW_OPTION_MUTATIONS = [_m("shadow_defer0", "opts", False, shadow_defer=0), _m("shadow_cache1", "opts", False, shadow_cache=1)]
PROC_EXPERIMENTS = [_m("sort_reuse31", "opts", False, sort_reuse=31)]
TO_GRID = Mutation("to_grid", "medium", None)
TO_PROC = Mutation("to_procedural", "medium", ())
TO_SHADOW = Mutation("to_procedural_shadow", "medium", (("shadow_steps", 8),))


def _layout_mutations(base_layout):
    return [Mutation(f"layout{p}", "layout", p, False) for p in LAYOUTS if p != base_layout]


# ---- bases ----------------------------------------------------------------------------------------------------------

# Derived bases, where a mutation would change nothing on the plain one:
#  *first2: band_flip -2 needs band_first + stride - 2 >= 0 rows to differ: (16, 3, 2) holds bands 2, 5 and, with
#   flip -2, bands 2, 3 -- 32 rows either way.
#  *flip2:  the way from flip 2 to flip 0.  The sets hold bands 0, 5, 6 and 0, 3, 6, and every pixel band 5 covers
#   (rows 80-95, the narrow lower end of the cube) band 3 covers too (rows 48-63): state built for the flip-0 set
#   happens to serve the flip-2 set, and only the way from 2 to 0 shows a reuse keyed without band_flip.
#  *scroll: tap_weight only scales MediaScroll, which the reference camera leaves at 0.
#  *dense:  at density 1 no ray's transmittance falls below 0.3, so early_out = 0.3 would end none; the dense bases'
#   densities put a good share of the covered rays below it (test_transitions_cpu.py checks that steps are saved).
_PS = (("shadow_steps", 8),)
BASES = {
    "G0": Scene(layout=0), "G12": Scene(layout=12), "G15": Scene(layout=15), "G1": Scene(layout=1),
    "P": Scene(proc=()), "PS": Scene(proc=_PS),
}
DERIVED = {
    "G0first2": replace(BASES["G0"], target=Target(band_first=2)),
    "Pfirst2": replace(BASES["P"], target=Target(band_first=2)),
    "PSfirst2": replace(BASES["PS"], target=Target(band_first=2)),
    "G0flip2": replace(BASES["G0"], target=Target(band_flip=2)),
    "Pflip2": replace(BASES["P"], target=Target(band_flip=2)),
    "PSflip2": replace(BASES["PS"], target=Target(band_flip=2)),
    "G0scroll": replace(BASES["G0"], cam=Cam(scroll=SCROLL_IN)),
    "G15scroll": replace(BASES["G15"], cam=Cam(scroll=SCROLL_IN)),
    "G0dense": replace(BASES["G0"], march=(("density", 12.0),)),
    "G15dense": replace(BASES["G15"], march=(("density", 12.0),)),
    "Pdense": replace(BASES["P"], march=(("density", 400.0),)),
    "PSdense": replace(BASES["PS"], march=(("density", 400.0),)),
}
ALL_BASES = {**BASES, **DERIVED}


def grid_mutations(layout):
    return (TARGET_MUTATIONS + CAMERA_MUTATIONS + SCROLL_MUTATIONS + MARCH_MUTATIONS + [TAP_SCALE] + VOLUME_MUTATIONS
            + GRID_OPTION_MUTATIONS + _layout_mutations(layout))


def proc_mutations(shadow):
    ms = TARGET_MUTATIONS + CAMERA_MUTATIONS + MARCH_MUTATIONS + PROC_FIELD_MUTATIONS + PROC_OPTION_MUTATIONS
    if shadow:
        ms = ms + [SUN_DIR, _m("shadow8to0", "proc", shadow_steps=0), _m("shadow8to5", "proc", shadow_steps=5)] \
            + SHADOW_OPTION_MUTATIONS
    else:
        ms = ms + [_m("shadow0to8", "proc", shadow_steps=8)]
    return ms


def _cases():
    out = []
    for b in ("G0", "G12", "G15", "G1"):
        out += [(b, m) for m in grid_mutations(BASES[b].layout)]
    out += [("G0", TO_PROC), ("G0", TO_SHADOW), ("G15", TO_PROC)]
    out += [("G15", m) for m in GRID_EXPERIMENTS]
    out += [("P", m) for m in proc_mutations(False)] + [("P", TO_GRID)] + [("P", m) for m in PROC_EXPERIMENTS]
    out += [("PS", m) for m in proc_mutations(True)] + [("PS", TO_GRID)] + [("PS", m) for m in PROC_EXPERIMENTS]
    out += [(b, FLIP_BACK) for b in ("G0first2", "Pfirst2", "PSfirst2")]
    out += [(b, FLIP_OFF) for b in ("G0flip2", "Pflip2", "PSflip2")]
    out += [(b, TAP_WEIGHT) for b in ("G0scroll", "G15scroll")]
    out += [(b, EARLY_OUT) for b in ("G0dense", "G15dense", "Pdense", "PSdense")]
    return out


CASES = _cases()
CASE_IDS = [f"{b}-{m.name}" for b, m in CASES]
assert len(set(CASE_IDS)) == len(CASE_IDS)


def needs_experiments(scene: Scene) -> bool:
    return any(option(scene, k) != OPTION_DEFAULTS[k] for k in EXPERIMENT_OPTIONS)


# ---- random walks ---------------------------------------------------------------------------------------------------

WALK_STEPS = 40
WALKS = {
    "grid": ("G0", grid_mutations(None) + [FLIP_BACK, TAP_WEIGHT, EARLY_OUT, _m("density12", "march", density=12.0)]),
    "procedural": ("P", [m for m in proc_mutations(False) if m.name != "shadow0to8"]
                   + [FLIP_BACK, EARLY_OUT, _m("density400", "march", density=400.0)]),
    "procedural_shadow": ("PS", [m for m in proc_mutations(True) if m.name != "shadow8to0"]
                          + [FLIP_BACK, EARLY_OUT, _m("density400", "march", density=400.0)]),
}


def _unset(m: Mutation, s: Scene, base: Scene) -> Scene:
    """The way back: the mutation's fields at the base's values."""
    if m.part == "target":
        return replace(s, target=replace(s.target, **{k: getattr(base.target, k) for k, _ in m.values}))
    if m.part == "cam":
        return replace(s, cam=replace(s.cam, **{k: getattr(base.cam, k) for k, _ in m.values}))
    if m.part in ("march", "proc", "opts"):
        cur, b = dict(getattr(s, m.part) or ()), dict(getattr(base, m.part) or ())
        for k, _ in m.values:
            cur.pop(k, None)
            if k in b:
                cur[k] = b[k]
        return replace(s, **{m.part: tuple(sorted(cur.items()))})
    part = "proc" if m.part == "medium" else m.part
    return replace(s, **{part: getattr(base, part)})


def walk(family: str, seed: int = 7):
    """The family's seeded walk: WALK_STEPS scenes, each one or two random
    mutations (set, or put back where already set) away from the one before."""
    base_name, muts = WALKS[family]
    base = BASES[base_name]
    rng = np.random.default_rng(seed + zlib.crc32(family.encode()))
    s, out = base, []
    while len(out) < WALK_STEPS:
        nxt = s
        for _ in range(int(rng.integers(1, 3))):
            m = muts[int(rng.integers(len(muts)))]
            nxt = _unset(m, nxt, base) if m.is_set(nxt) else m(nxt)
        if nxt == s or not target_valid(nxt.target) or needs_experiments(nxt):
            continue
        out.append(nxt)
        s = nxt
    return base, out


# ---- GPU side: apply() and check() ----------------------------------------------------------------------------------

class Harness:
    """One long-lived Renderer and what is installed in it."""

    def __init__(self, r, oracle):
        self.r, self.oracle = r, oracle
        self.cur: Scene | None = None
        self.buffers: dict = {}
        self.counter = None
        self.calls: list[str] = []     # the setters apply() called, for the tests of apply() itself

    def _call(self, name, *args):
        self.calls.append(name)
        getattr(self.r, name)(*args)

    def apply(self, new: Scene, full: bool = False) -> None:
        """Call only the setters whose inputs differ between the installed
        scene and `new` (all of them with full = True or on a fresh context)."""
        prev = None if full else self.cur
        self.calls = []
        if prev is None or prev.vol != new.vol:
            if prev is not None and (prev.vol, new.vol) == ("A", "A+box"):
                self._call("update_volume", volume("box"), BOX_ORIGIN)
            else:
                self._call("set_volume", volume(new.vol))
        if prev is None or prev.layout != new.layout:
            self._call("set_layout_preference", new.layout)
        if prev is None or prev.cam != new.cam:
            self._call("set_shader_data", *shader_data(new.cam))
        if prev is None or prev.march != new.march:
            self._call("set_march", march_params(new))
        if prev is None or prev.proc != new.proc:
            self._call("set_procedural", procedural_params(new))
        for name in OPTION_DEFAULTS:
            if prev is None or option(prev, name) != option(new, name):
                self.calls.append("set_option:" + name)
                self.r.set_option(name, option(new, name))
        self.cur = new

    def _buffer(self, t: Target, rows: int):
        import torch
        c = CHANNELS[t.fmt]
        shape = (rows, t.W + t.pad, 4) if c == 4 else (rows, t.W + t.pad)
        dtype = torch.float32 if t.fmt in FLOAT_FORMATS else torch.uint8
        key = (t.buf, shape, dtype)
        if key not in self.buffers:
            if len(self.buffers) > 64:
                self.buffers.clear()
            self.buffers[key] = torch.empty(shape, dtype=dtype, device="cuda")
        if self.counter is None:
            self.counter = torch.zeros(1, dtype=torch.int64, device="cuda")
        return self.buffers[key]

    def check(self, scene: Scene | None = None) -> None:
        """Render the installed scene into a sentinel-filled buffer with the
        target's pad; every selected pixel equals the oracle (sRGB: <= 1 LSB),
        every other byte keeps the sentinel, and the counter, pre-set to
        COUNTER_START, ends at COUNTER_START + the selected rows' steps."""
        import torch
        scene = scene or self.cur
        assert scene == self.cur, "check() renders what apply() installed"
        t = scene.target
        rows, want, steps = expected(self.oracle, scene)
        buf = self._buffer(t, t.H if in_place(t) else len(rows))
        isfloat = t.fmt in FLOAT_FORMATS
        buf.fill_(float("nan") if isfloat else BYTE_SENTINEL)
        self.counter.fill_(COUNTER_START)
        tgt = _lib.Target(width=t.W, height=t.H, format=target_format_word(t),
                          band_rows=t.band_rows, band_stride=t.band_stride, band_first=t.band_first,
                          pixels=buf.data_ptr(), row_pitch=buf.stride(0) * buf.element_size(),
                          step_counter=self.counter.data_ptr(), band_flip=t.band_flip)
        assert tgt.row_pitch == (t.W + t.pad) * BYTES_PER_PIXEL[t.fmt]
        _lib.call("vr_render", self.r._ctx, ctypes.byref(tgt), None)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        sel = rows >= 0
        at = rows[sel] if in_place(t) else np.nonzero(sel)[0]   # buffer rows that are written
        written = np.zeros(got.shape[:2], bool)
        written[at, :t.W] = True
        px = got[at][:, :t.W]
        assert px.shape == want.shape
        if t.fmt in SRGB_FORMATS:
            d = np.abs(px.astype(np.int16) - want.astype(np.int16))
            assert d.max() <= 1, f"sRGB differs by {d.max()} LSB at {np.argwhere(d > 1)[:5].tolist()}"
        else:
            bad = np.argwhere(px != want)
            assert bad.size == 0, f"{len(bad)} mismatches, first {bad[:5].tolist()}: " \
                                  f"{px[tuple(bad[0])]} vs {want[tuple(bad[0])]}"
        rest = got[~written]
        untouched = np.isnan(rest) if isfloat else rest == BYTE_SENTINEL
        assert untouched.all(), f"{int((~untouched).sum())} values outside the target's rows and columns were written"
        assert int(self.counter.item()) == COUNTER_START + steps, (int(self.counter.item()) - COUNTER_START, steps)
