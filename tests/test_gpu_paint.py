"""vr_paint on the GPU: the painted volume against the numpy restatement of the
brush (tests/paint_spec.py), the painted context's frame against a fresh
install of the painted volume and against the CPU oracle, per layout; uniform
channels; stream order; the pick -> paint -> footprint -> re-render loop; undo
through vr_get_volume_box; refusals.  Everything is exact (volumes byte for
byte, frames bit for bit, step counters equal).

The volume, frame and march are tests/brush_harness.py's: 37 x 22 x 45 (no axis
a multiple of a brick edge), the reference camera at 64 x 64, 32 steps.  As in
test_gpu_update.py, a march that sparse sees a small edit from few angles only, so the two
small brushes render from the (phi, theta) of a 30-degree grid at which the
ORACLE's frame changes in the most pixels under both tested blends: `corner`
from (210, 60) (120 and 134 pixels; 27 and 29 at (0, 0)) and `outside_centre`
from (210, 0) (28 pixels; 4 at (0, 0)).  `straddle` (337 / 396 pixels) and
`whole` (1452) render from (0, 0).
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import paint_spec as ps  # noqa: E402
from brush_harness import (H, LAYOUT_IDS, LAYOUTS, W, assert_exact, assert_marches, base, check_frame,  # noqa: E402,F401
                           check_fresh_install, check_needs_a_volume, frame, fresh, oracle_frame, r, setup)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import volumetricrenderer_amd as vr
from volumetricrenderer_amd import _lib  # noqa: E402
from volumetricrenderer_amd._lib import FMT_RGBA32F  # noqa: E402

NX, NY, NZ = ps.NX, ps.NY, ps.NZ
UNIFORM_VARIANTS = {12, 14, 15}   # the layouts whose march has the _uX (no loads for one channel) kernels
RENDER_BRUSHES = {"straddle": (0.0, 0.0), "corner": (210.0, 60.0), "outside_centre": (210.0, 0.0),
                  "whole": (0.0, 0.0)}
RENDER_MODES = [(ps.SET, 1, "smooth_set"), (ps.ADD, 0, "hard_add")]


def paint(rr, name, op, falloff, value=ps.VALUE, strength=ps.STRENGTH, stream=None):
    centre, radius = ps.BRUSHES[name]
    return rr.paint(centre, radius, op, falloff, value, strength, stream=stream)


# ---- 1. the painted volume is the specification's --------------------------------------------
@pytest.mark.parametrize("falloff,fname", ps.FALLOFFS, ids=[n for _, n in ps.FALLOFFS])
@pytest.mark.parametrize("op,oname", ps.OPS, ids=[n for _, n in ps.OPS])
@pytest.mark.parametrize("name", list(ps.BRUSHES))
def test_painted_volume_equals_the_specification(r, base, name, op, oname, falloff, fname):
    r.set_layout_preference(14)
    r.set_volume(base)
    centre, radius = ps.BRUSHES[name]
    got_box = paint(r, name, op, falloff)
    assert got_box == ps.spec_box(centre, radius)
    assert got_box == vr.brush_box(vr.make_brush(centre, radius, op, falloff, ps.VALUE, ps.STRENGTH), (NX, NY, NZ))
    want = ps.spec_apply(base, centre, radius, op, falloff)
    assert (want != base).any() == (name != "miss")
    assert_exact(r.get_volume(), want)
    assert_exact(vr.brush_apply(vr.make_brush(centre, radius, op, falloff, ps.VALUE, ps.STRENGTH), base.copy()), want)


# ---- 2. the painted context renders what a fresh install of the painted volume renders ------
@pytest.mark.parametrize("op,falloff,mode", RENDER_MODES, ids=[m for _, _, m in RENDER_MODES])
@pytest.mark.parametrize("name", list(RENDER_BRUSHES))
@pytest.mark.parametrize("pref,lname", LAYOUTS, ids=LAYOUT_IDS)
def test_painted_render_equals_fresh_install(r, fresh, oracle, base, pref, lname, name, op, falloff, mode):
    angles = RENDER_BRUSHES[name]
    centre, radius = ps.BRUSHES[name]
    painted = ps.spec_apply(base, centre, radius, op, falloff)
    ref, ref_steps = oracle_frame(oracle, painted, angles)
    before, _ = oracle_frame(oracle, base, angles)
    assert (ref != before).any(), "the brush does not change the oracle's frame from this camera"
    setup(r, pref, base, angles)
    assert_marches(r, lname)
    pre, _ = frame(r)
    assert_exact(pre, before)
    paint(r, name, op, falloff)
    assert_marches(r, lname)
    img, steps = check_frame(r, oracle, painted, angles)
    check_fresh_install(fresh, pref, lname, painted, img, steps, angles)


# ---- 3. uniform channels ---------------------------------------------------------------------
@pytest.mark.parametrize("pref,lname", LAYOUTS, ids=LAYOUT_IDS)
def test_uniform_channel(r, oracle, base, pref, lname):
    """G is the constant 77.  A brush that leaves G alone (strength 0) and an ADD of 0 keep the
    uniform bit and the _uG kernel; a SET towards 200 clears both before the next render."""
    vol = base.copy()
    vol[..., 1] = 77
    centre, radius = ps.BRUSHES["straddle"]
    cases = [("strength0", ps.SET, 1, ps.VALUE, (255, 0, 255, 255), True),
             ("add0", ps.ADD, 0, (200, 0, 255, 10), (255, 255, 255, 255), True),
             ("set200", ps.SET, 1, (200, 200, 255, 10), (255, 255, 255, 255), False)]
    for what, op, falloff, value, strength, keeps in cases:
        setup(r, pref, vol)
        assert r.get_option("uniform_mask") & 2, what
        assert r.kernel_variant.endswith("_uG") == (pref in UNIFORM_VARIANTS), what
        r.paint(centre, radius, op, falloff, value, strength)
        painted = ps.spec_apply(vol, centre, radius, op, falloff, value, strength)
        assert (painted != vol).any(), what
        assert ((painted[..., 1] == 77).all()) == keeps, what
        assert bool(r.get_option("uniform_mask") & 2) == keeps, what
        assert r.kernel_variant.endswith("_uG") == (keeps and pref in UNIFORM_VARIANTS), what
        assert_marches(r, lname)
        check_frame(r, oracle, painted)


# ---- 4. one stream, no host wait -------------------------------------------------------------
@pytest.mark.parametrize("pref,lname", LAYOUTS, ids=LAYOUT_IDS)
def test_stream_order(r, oracle, base, pref, lname):
    """Three dabs, each directly followed by a render on the same side stream, one synchronise at
    the end: every frame is the oracle's for the volume painted so far."""
    dabs = [("straddle", ps.SET, 1), ("corner", ps.ADD, 0), ("far_corner", ps.SUB, 1)]
    outs = [r.alloc_target(W, H, FMT_RGBA32F) for _ in dabs]
    cnts = [torch.zeros(1, dtype=torch.int64, device="cuda") for _ in dabs]
    setup(r, pref, base)
    assert_marches(r, lname)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    for k, (name, op, falloff) in enumerate(dabs):
        paint(r, name, op, falloff, stream=s)
        r.render(W, H, FMT_RGBA32F, out=outs[k], stream=s, step_counter=cnts[k])
    s.synchronize()
    painted = base
    for k, (name, op, falloff) in enumerate(dabs):
        painted = ps.spec_apply(painted, *ps.BRUSHES[name], op, falloff)
        ref, ref_steps = oracle_frame(oracle, painted)
        assert_exact(outs[k].cpu().numpy(), ref)
        assert int(cnts[k].item()) == ref_steps
    assert_exact(r.get_volume(), painted)


# ---- 5. the loop: pick -> paint -> footprint -> re-render ------------------------------------
@pytest.mark.parametrize("pref,lname", LAYOUTS, ids=LAYOUT_IDS)
def test_pick_paint_footprint_rerender(r, oracle, base, pref, lname):
    density = 32.0   # dense enough for rays to pass the 0.5 transmittance threshold (a hit)
    setup(r, pref, base, density=density)
    assert_marches(r, lname)
    rec = vr.ray_records(r.query_rect((0, 0, W, H), W, H, 0.5))
    hits = np.argwhere(rec["hit_step"] >= 0)
    assert len(hits) > 0, "no ray has a hit"
    py, px = (int(v) for v in hits[np.argmin(((hits - (H // 2, W // 2)) ** 2).sum(axis=1))])
    one, texel = r.pick(px, py, W, H, 0.5)
    assert one["hit_step"] >= 0 and texel is not None
    buf = r.render(W, H, FMT_RGBA32F)
    box = r.paint(texel, (3, 3, 3), ps.SET, 0, (255, 255, 255, 255), (255, 255, 255, 255))
    assert box is not None
    fx, fy, fw, fh = r.update_footprint(box[0], box[1], W, H)
    assert fx <= px < fx + fw and fy <= py < fy + fh
    r.render_rect(buf, (fx, fy, fw, fh), FMT_RGBA32F)
    torch.cuda.synchronize()
    painted = ps.spec_apply(base, texel, (3, 3, 3), ps.SET, 0, (255,) * 4, (255,) * 4)
    want, _ = oracle_frame(oracle, painted, density=density)
    before, _ = oracle_frame(oracle, base, density=density)
    assert want[py, px, 0] != before[py, px, 0], "the dab does not change the picked pixel"
    assert_exact(buf.cpu().numpy(), want)
    assert_exact(frame(r)[0], want)


# ---- 6. undo and the box read-back -----------------------------------------------------------
@pytest.mark.parametrize("pref,lname", LAYOUTS, ids=LAYOUT_IDS)
def test_undo(r, oracle, base, pref, lname):
    setup(r, pref, base)
    assert_marches(r, lname)
    centre, radius = ps.BRUSHES["straddle"]
    origin, extent = vr.brush_box(vr.make_brush(centre, radius), (NX, NY, NZ))
    saved = r.get_volume_box(origin, extent)
    assert paint(r, "straddle", ps.SET, 1) == (origin, extent)
    img, _ = frame(r)
    assert (img != oracle_frame(oracle, base)[0]).any()
    r.update_volume(saved, origin)
    assert_exact(r.get_volume(), base)
    img, steps = frame(r)
    ref, ref_steps = oracle_frame(oracle, base)
    assert_exact(img, ref)
    assert steps == ref_steps


def test_get_volume_box(r, base):
    r.set_layout_preference(0)
    r.set_volume(base)
    centre, radius = ps.BRUSHES["straddle"]
    boxes = [vr.brush_box(vr.make_brush(centre, radius), (NX, NY, NZ)), ((0, 0, 0), (NX, NY, NZ)), ((5, 0, 44), (32, 22, 1))]
    boxes += [((x, y, z), (1, 1, 1)) for x in (0, NX - 1) for y in (0, NY - 1) for z in (0, NZ - 1)]
    s = torch.cuda.Stream()
    for (x0, y0, z0), (bx, by, bz) in boxes:
        want = base[z0:z0 + bz, y0:y0 + by, x0:x0 + bx]
        assert_exact(r.get_volume_box((x0, y0, z0), (bx, by, bz)), want)
        guard = torch.full((bz + 2, by, bx, 4), 0xA5, dtype=torch.uint8, device="cuda")   # a guard slice on either side
        out = guard[1:bz + 1]
        assert r.get_volume_box((x0, y0, z0), (bx, by, bz), out=out) is out
        assert_exact(out.cpu().numpy(), want)
        assert (guard[0] == 0xA5).all() and (guard[bz + 1] == 0xA5).all()
        dev = r.get_volume_box((x0, y0, z0), (bx, by, bz), stream=s)   # asynchronous on s
        s.synchronize()
        assert dev.is_cuda
        assert_exact(dev.cpu().numpy(), want)
    assert_exact(r.get_volume(), base)


# ---- 7. refusals -----------------------------------------------------------------------------
def test_refusals(r, base):
    setup(r, 0, base)
    good = dict(centre=(17, 11, 23), radius=(3, 2, 4))
    bad = [dict(good, op=3), dict(good, op=-1), dict(good, falloff=2), dict(good, falloff=-1)]
    bad += [dict(good, radius=rr) for rr in ((-1, 2, 4), (3, 256, 4), (3, 2, 2**31 - 1))]
    for kw in bad:
        with pytest.raises(vr.VRError) as e:
            r.paint(**kw)
        assert e.value.status == 1 and "vr_paint" in str(e.value), kw   # VR_ERR_INVALID
        assert np.array_equal(r.get_volume(), base)
    for k in range(2):
        b = vr.make_brush(**good)
        b.reserved[k] = 7
        with pytest.raises(vr.VRError) as e:
            _lib.call("vr_paint", r._ctx, ctypes.byref(b), None)
        assert e.value.status == 1
        assert np.array_equal(r.get_volume(), base)
    with pytest.raises(vr.VRError) as e:
        _lib.call("vr_paint", r._ctx, None, None)
    assert e.value.status == 1
    assert r.paint((-10, -10, -10), (4, 4, 4)) is None            # a miss is VR_OK
    assert np.array_equal(r.get_volume(), base)
    # a box that leaves the volume, or has no extent: vr_update_volume's checks
    host = np.zeros((NZ, NY, NX, 4), np.uint8)
    devt = torch.zeros((NZ, NY, NX, 4), dtype=torch.uint8, device="cuda")
    hp, dp = host.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(devt.data_ptr())
    for origin, ext in [((-1, 0, 0), (1, 1, 1)), ((0, NY, 0), (1, 1, 1)), ((30, 0, 0), (8, 1, 1)), ((0, 0, 38), (1, 1, 8)),
                        ((1, 0, 0), (NX, NY, NZ)), ((0, 0, 0), (0, 1, 1)), ((0, 0, 0), (1, -3, 1)),
                        ((2**31 - 1, 0, 0), (2**31 - 1, 1, 1))]:
        for fn, tail in (("vr_get_volume_box", (hp,)), ("vr_get_volume_box_device", (dp, None))):
            with pytest.raises(vr.VRError) as e:
                _lib.call(fn, r._ctx, *origin, *ext, *tail)
            assert e.value.status == 1, (fn, origin, ext)
    assert not host.any() and not devt.any()
    assert np.array_equal(r.get_volume(), base)
    with pytest.raises(ValueError):   # the wrapper's shape check
        r.get_volume_box((0, 0, 0), (2, 2, 2), out=torch.zeros((2, 2, 3, 4), dtype=torch.uint8, device="cuda"))
    check_needs_a_volume(r, lambda rr: rr.paint(**good))
    with vr.Renderer(0) as empty:     # no volume installed: no box to read back either
        for fn, tail in (("vr_get_volume_box", (hp,)), ("vr_get_volume_box_device", (dp, None))):
            with pytest.raises(vr.VRError) as e:
                _lib.call(fn, empty._ctx, 0, 0, 0, 1, 1, 1, *tail)
            assert e.value.status == 3
    assert np.array_equal(r.get_volume(), base)
