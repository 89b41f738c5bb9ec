"""One chain of volume edits, one per member of the brush family, shared by
test_gpu_edit_chain.py (one long-lived Renderer per layout and variant, every
render call after every edit against the oracle) and test_edit_chain_cpu.py (the
chain's own conditions, oracle and numpy only).

The volume is paint_spec.base_volume(), 37 x 22 x 45 (no axis a multiple of a brick
edge), in five variants: no uniform channel, or exactly channel c of R, G, B, A set to
UVAL.  The expected volume after an edit is the existing numpy restatement of that
brush applied to the expected volume before it; nothing here calls the library's
brushes.

The order of the twelve edits (q is the variant's uniform channel, A for `none`):
   1  stamp_affine  interior     strength 0 on q             (b) q stays uniform
   2  paint_stroke  far_corner, straddle, interior, corner   (b)
   3  blur          wide         staged, large               (b)
   4  morph         interior     staged, small               (b)
   5  paint         wide         SET, full strength, value[q] = UVAL: (c) q is still uniform
   6  stamp         straddle     random bytes, full strength: (d) q breaks
   7  rank          wide         staged, large
   8  clone         interior     from (2, 1, -1) texels away: staged, small
   9  remap         tall
  10  fill          wide         staged, large (4 bytes per texel)
  11  clone_affine  interior     a shift by texels and a fraction, trilinear: staged, small
  12  update        the whole volume, q constant again:       (e) the mask stays lost
The staged brushes (they share the blur scratch) alternate between the large box and
the small one, and every edit's box meets the box of the edit before it (the stroke's
boxes count together): `wide` and `tall` are the two brushes added to paint_spec's
for that, since straddle, corner, far_corner and interior are disjoint.  The taps of G, B
and A sample the volume at 0.8, 0.75 and 0.7 of the ray point, so texels past x 25,
y 15, z 31 show in R alone and `corner` lies behind the 16 steps: far_corner and corner
are dabs of the stroke only, where get_volume sees them.

Nothing here needs a GPU to import.
"""
from __future__ import annotations

import ctypes
import zlib
from typing import Callable, NamedTuple

import numpy as np

import affine_spec as af
import blur_spec as bs
import clone_spec as cs
import fill_spec as fs
import morph_spec as ms
import paint_spec as ps
import rank_spec as rs
import remap_spec as rm
from volumetricrenderer_amd import _lib

W, H, STEPS = 70, 37, 16        # quads fall off the right and the bottom edge
FMT = _lib.FMT_RGBA8_UNORM
DIMS = (ps.NX, ps.NY, ps.NZ)
UVAL, UVAL_AGAIN = 102, 57      # the uniform channel's byte; the byte the last edit makes it constant at
VARIANTS = [None, 0, 1, 2, 3]
VARIANT_IDS = ["none", "R", "G", "B", "A"]
# ends rays after 4k + 1, 4k + 2, 4k + 3 and 4k + 4 steps at every step of every variant's chain
# (test_edit_chain_cpu.py test_early_out_lands_on_every_step_of_a_round tried it; 0.98 of the 40^3 volume does too)
EARLY = 0.98
CAMERAS = [(20.0, -35.0), (21.6, -35.0), (23.2, -35.0), (24.8, -35.0)]   # test_gpu_dispatch's four

BRUSHES = {k: ps.BRUSHES[k] for k in ("straddle", "corner", "far_corner", "interior")}
BRUSHES["wide"] = ((19, 10, 27), (16, 4, 6))    # x 3..35, y 6..14, z 21..33: meets straddle and interior
BRUSHES["tall"] = ((17, 11, 27), (4, 6, 9))     # x 13..21, y 5..17, z 18..36: meets straddle, interior and wide
FULL = (255, 255, 255, 255)
CLONE_OFFSET = (2, 1, -1)
AFFINE_SHIFT = (5 * af.ONE + 0x8000, -3 * af.ONE + 0x4000, 7 * af.ONE)   # 16.16: 5.5, -2.75 and 7 texels
PHASES = ["b", "b", "b", "b", "c", "d", "", "", "", "", "", "e"]
STAGED = {"blur": "large", "morph": "small", "rank": "large", "clone": "small", "fill": "large", "clone_affine": "small"}


class Edit(NamedTuple):
    name: str                 # the family member
    brush: str                # the brush's name (the stroke: its dabs'), for the messages
    phase: str                # "b", "c", "d", "e" of the module docstring, or ""
    boxes: list               # the (origin, extent) boxes it rewrites, as the specification clips them
    returns: object           # what the Renderer method returns: a box, a list of boxes, or None (update_volume)
    apply: Callable           # expected volume -> expected volume
    run: Callable             # (renderer, vr, torch) -> what the Renderer method returned


def quiet(variant):
    """The channel the first four edits leave alone."""
    return 3 if variant is None else variant


def base(variant):
    v = ps.base_volume()
    if variant is not None:
        v[..., variant] = UVAL
    for c in range(4):
        assert (v[..., c].min() == v[..., c].max()) == (c == variant)
    return v


def _without(q, strength=(255, 200, 230, 255)):
    return tuple(0 if c == q else s for c, s in enumerate(strength))


def fill_rule(centre):
    """R within [0, seed's byte + 60] around the brush centre: the seed itself always passes."""
    return fs.Rule(tuple(centre), (255, 0, 0, 0), (60, 0, 0, 0), (1, 0, 0, 0), 1)


def chain(variant):
    q = quiet(variant)
    s0 = _without(q)
    B = BRUSHES
    edits = []

    def add(name, brush, boxes, returns, apply, run):
        edits.append(Edit(name, brush, PHASES[len(edits)], boxes, returns, apply, run))

    def box_of(name):
        return ps.spec_box(*B[name])

    # 1 stamp_affine
    c, r = B["interior"]
    stamp = af.stamp_bytes()
    table = af.MAPS["rot30_axis"](c, af.STAMP_CENTRE)
    add("stamp_affine", "interior", [box_of("interior")], box_of("interior"),
        lambda v, c=c, r=r: af.spec_affine(v, stamp, table, af.LINEAR, af.CLAMP, c, r, ps.SET, 0, s0),
        lambda rr, vr, torch, c=c, r=r: rr.stamp_affine(torch.from_numpy(stamp).cuda(), vr.make_affine(*table, af.LINEAR, af.CLAMP),
                                                        c, r, ps.SET, 0, s0))
    # 2 paint_stroke
    dabs = [("far_corner", ps.ADD, 1), ("straddle", ps.SET, 1), ("interior", ps.SUB, 0), ("corner", ps.SET, 0)]

    def stroke(v):
        for name, op, falloff in dabs:
            v = ps.spec_apply(v, *B[name], op, falloff, ps.VALUE, s0)
        return v
    add("paint_stroke", "+".join(n for n, _, _ in dabs), [box_of(n) for n, _, _ in dabs], [box_of(n) for n, _, _ in dabs], stroke,
        lambda rr, vr, torch: rr.paint_stroke([vr.make_brush(*B[n], op, fo, ps.VALUE, s0) for n, op, fo in dabs]))
    # 3 blur, 4 morph
    c, r = B["wide"]
    add("blur", "wide", [box_of("wide")], box_of("wide"), lambda v, c=c, r=r: bs.spec_blur(v, c, r, 2, 1, s0),
        lambda rr, vr, torch, c=c, r=r: rr.blur(c, r, 2, 1, s0))
    c, r = B["interior"]
    add("morph", "interior", [box_of("interior")], box_of("interior"), lambda v, c=c, r=r: ms.spec_morph(v, c, r, ms.DILATE, 1, 0, s0),
        lambda rr, vr, torch, c=c, r=r: rr.morph(c, r, ms.DILATE, 1, 0, s0))
    # 5 paint: the uniform byte itself into q, SET at full strength
    c, r = B["wide"]
    value = tuple(UVAL if ch == q else x for ch, x in enumerate(ps.VALUE))
    add("paint", "wide", [box_of("wide")], box_of("wide"), lambda v, c=c, r=r: ps.spec_apply(v, c, r, ps.SET, 1, value, FULL),
        lambda rr, vr, torch, c=c, r=r: rr.paint(c, r, ps.SET, 1, value, FULL))
    # 6 stamp: random bytes on every channel
    c, r = B["straddle"]
    s_extent, s_origin = (20, 7, 4), (10, 7, 29)
    bytes6 = cs.stamp_bytes(s_extent)
    sbox = cs.spec_stamp_box(c, r, s_origin, s_extent)
    add("stamp", "straddle", [sbox], sbox, lambda v, c=c, r=r: cs.spec_stamp(v, bytes6, s_origin, c, r, ps.SET, 0, FULL),
        lambda rr, vr, torch, c=c, r=r: rr.stamp(torch.from_numpy(bytes6).cuda(), s_origin, c, r, ps.SET, 0, FULL))
    # 7 rank, 8 clone
    c, r = B["wide"]
    add("rank", "wide", [box_of("wide")], box_of("wide"), lambda v, c=c, r=r: rs.spec_rank(v, c, r, rs.MEDIAN, 1, 1, FULL),
        lambda rr, vr, torch, c=c, r=r: rr.rank(c, r, rs.MEDIAN, 1, 1, FULL))
    c, r = B["interior"]
    assert not cs.spec_direct(c, r, CLONE_OFFSET, (0, 0, 0))   # the staged path
    add("clone", "interior", [box_of("interior")], box_of("interior"),
        lambda v, c=c, r=r: cs.spec_clone(v, c, r, CLONE_OFFSET, (0, 0, 0), ps.SET, 0, FULL),
        lambda rr, vr, torch, c=c, r=r: rr.clone(c, r, CLONE_OFFSET, (0, 0, 0), ps.SET, 0, FULL))
    # 9 remap
    c, r = B["tall"]
    lut = rm.TABLES["perm"]
    add("remap", "tall", [box_of("tall")], box_of("tall"), lambda v, c=c, r=r: rm.spec_remap(v, lut, c, r, ps.SET, 1, FULL),
        lambda rr, vr, torch, c=c, r=r: rr.remap(c, r, lut, ps.SET, 1, FULL))
    # 10 fill
    c, r = B["wide"]
    rule = fill_rule(c)
    add("fill", "wide", [box_of("wide")], box_of("wide"), lambda v, c=c, r=r: fs.spec_fill(v, c, r, ps.ADD, 1, rule, ps.VALUE, FULL)[0],
        lambda rr, vr, torch, c=c, r=r: rr.fill(None, c, r, ps.ADD, 1, ps.VALUE, FULL,
                                                rule=vr.make_fill_rule(rule.seed, rule.lo, rule.hi, rule.select, rule.relative)))
    # 11 clone_affine
    c, r = B["interior"]
    half = (af.I3, c, tuple(int(x) * af.ONE + d for x, d in zip(c, AFFINE_SHIFT)))
    assert not af.spec_direct(half, af.LINEAR, c, r)        # the staged path
    add("clone_affine", "interior", [box_of("interior")], box_of("interior"),
        lambda v, c=c, r=r: af.spec_affine(v, None, half, af.LINEAR, af.CLAMP, c, r, ps.SET, 1, FULL),
        lambda rr, vr, torch, c=c, r=r: rr.clone_affine(c, r, vr.make_affine(*half, af.LINEAR, af.CLAMP), ps.SET, 1, FULL))
    # 12 update: the whole volume, q constant again
    whole = ((0, 0, 0), DIMS)

    def again(v):
        out = v.copy()
        out[..., q] = UVAL_AGAIN
        return out
    state = {}

    def apply12(v):
        state["box"] = again(v)
        return state["box"]
    add("update_volume", "whole", [whole], None, apply12, lambda rr, vr, torch: rr.update_volume(state["box"], (0, 0, 0)))
    assert len(edits) == len(PHASES) == 12
    return edits


_expected: dict = {}


def expected(variant):
    """(the chain, the 13 expected volumes: the base, then the volume after each edit), once per variant; read-only."""
    if variant not in _expected:
        edits = chain(variant)
        vols = [base(variant)]
        for e in edits:
            vols.append(np.ascontiguousarray(e.apply(vols[-1])))
        for v in vols:
            v.setflags(write=False)
        _expected[variant] = (edits, vols)
    return _expected[variant]


def truly_uniform(vol):
    """Bit c set = every texel of channel c of `vol` holds one byte."""
    return sum(1 << c for c in range(4) if vol[..., c].min() == vol[..., c].max())


def expected_mask(variant, step):
    """The uniform mask a context may hold after `step` edits (0 = the install): channel c is set iff it is uniform in
    the expected volume then and was at every earlier step -- the mask can only be lost (vr.h vr_update_volume)."""
    vols = expected(variant)[1]
    m = 15
    for v in vols[:step + 1]:
        m &= truly_uniform(v)
    return m


def boxes_meet(a, b):
    return all(ao < bo + be and bo < ao + ae for ao, ae, bo, be in zip(a[0], a[1], b[0], b[1]))


# ---- cameras, march constants, the oracle's frames -----------------------------------------------------------------

def shader_data(cam):
    """(ObjectShaderData, GlobalShaderData) of CAMERAS[cam] by the library's host producer."""
    osd, gsd = _lib.ObjectShaderData(), _lib.GlobalShaderData()
    phi, theta = CAMERAS[cam]
    _lib.call("vr_reference_shader_data", ctypes.c_float(W / H), ctypes.c_float(phi), ctypes.c_float(theta), ctypes.c_float(0.0),
              ctypes.byref(osd), ctypes.byref(gsd))
    return osd, gsd


def shader_arrays(cam):
    osd, gsd = shader_data(cam)
    return np.frombuffer(bytes(osd), np.float32).copy(), np.frombuffer(bytes(gsd), np.float32).copy()


def march_params(early=0.0, **overrides):
    m = _lib.MarchParams()
    _lib.call("vr_march_defaults", ctypes.byref(m))
    m.max_steps, m.step_scale, m.early_out = STEPS, 1.0, early
    for k, v in overrides.items():
        setattr(m, k, v)
    return m


_frames: dict = {}


def oracle_frame(oracle, vol, cam=0, early=0.0):
    """The oracle's RGBA8 frame of `vol`, once per (volume bytes, camera, early-out); read-only."""
    key = (zlib.crc32(vol.tobytes()), hash(vol.tobytes()), cam, early)
    if key not in _frames:
        obj, glob = shader_arrays(cam)
        img, _ = oracle.render(vol, obj, glob, oracle.from_params(march_params(early)), W, H, FMT)
        img.setflags(write=False)
        _frames[key] = img
    return _frames[key]


def early_out_cuts(oracle, vol, cam, early):
    """(cuts, full): cuts[k], k = 0..STEPS, is a LOWER bound of the number of rays that the early-out ends after
    exactly k steps, short of their own last step; full is oracle.step_counts' frame (the steps without early-out).
    Only the oracle's step totals are used.  A march of j steps with step_scale j / STEPS takes the first j steps of
    the full march (the step size is the same float, asserted), so with e the steps a ray executes under the
    early-out and n those without, its total is sum(min(e, j)) and sum(min(n, j)) comes from `full`.  The
    difference `saved[j]` grows from j - 1 to j by alive[j] = the rays with e < j <= n, and
    alive[k + 1] - alive[k] = (rays with e = k < n) - (rays with e < k = n) <= the rays cut after exactly k steps."""
    obj, glob = shader_arrays(cam)
    full = np.maximum(oracle.step_counts(obj, glob, oracle.from_params(march_params()), W, H), 0)
    saved = [0]
    for j in range(1, STEPS + 1):
        scale = np.float32(j) / np.float32(STEPS)
        assert (np.float32(1.0) / np.float32(j)) * scale == np.float32(1.0) / np.float32(STEPS), j
        m = oracle.from_params(march_params(early, max_steps=j, step_scale=float(scale)))
        _, total = oracle.render(vol, obj, glob, m, W, H, FMT)
        saved.append(int(np.minimum(full, j).sum()) - total)
    alive = [0] + [saved[j] - saved[j - 1] for j in range(1, STEPS + 1)]   # alive[j], j = 1..STEPS
    assert alive[1] == 0 and all(a >= 0 for a in alive)
    cuts = [0] + [max(0, alive[k + 1] - alive[k]) for k in range(1, STEPS)] + [0]
    return cuts, full
