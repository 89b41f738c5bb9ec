"""vr_blur on the GPU: the blurred volume against the numpy restatement of the
box-filter brush (tests/blur_spec.py), byte for byte; volumes that cut the stage
kernel's tiles; the blurred context's frame against a fresh install of the
blurred volume and against the CPU oracle, per layout; two blurs and a
render_rects queued on one side stream; uniform channels; the staging scratch;
undo; refusals.  Everything is exact.

The volume, frame, march and cameras are brush_harness.py's: 37 x 22 x 45, the
reference camera at 64 x 64, 32 steps, `straddle` and `whole` from (0, 0).
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blur_spec as bs  # noqa: E402
import paint_spec as ps  # noqa: E402
from brush_harness import (FULL, H, LAYOUT_IDS, LAYOUTS, UNIFORM_LAYOUTS, VOLUME_BRUSHES, W, assert_exact,  # noqa: E402,F401
                           assert_marches, base, check_frame, check_fresh_install, check_needs_a_volume, frame, fresh,
                           oracle_frame, r, recipe_volume, setup)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import volumetricrenderer_amd as vr
from volumetricrenderer_amd import _lib  # noqa: E402
from volumetricrenderer_amd._lib import FMT_RGBA32F  # noqa: E402

NX, NY, NZ = ps.NX, ps.NY, ps.NZ


def blur(rr, name, h, falloff, strength=bs.STRENGTH, stream=None):
    centre, radius = ps.BRUSHES[name]
    return rr.blur(centre, radius, h, falloff, strength, stream=stream)


# ---- 1. the blurred volume is the specification's ---------------------------------------------
@pytest.mark.parametrize("falloff,fname", ps.FALLOFFS, ids=[n for _, n in ps.FALLOFFS])
@pytest.mark.parametrize("h", bs.HALF_WIDTHS)
@pytest.mark.parametrize("name", VOLUME_BRUSHES)
def test_blurred_volume_equals_the_specification(r, base, name, h, falloff, fname):
    r.set_layout_preference(14)
    r.set_volume(base)
    centre, radius = ps.BRUSHES[name]
    assert blur(r, name, h, falloff) == ps.spec_box(centre, radius)
    want = bs.spec_blur(base, centre, radius, h, falloff)
    assert (want != base).any() == (name != "miss")
    assert_exact(r.get_volume(), want)
    assert_exact(vr.brush_blur_apply(vr.make_brush(centre, radius, 0, falloff, 0, bs.STRENGTH), h, base.copy()), want)


# ---- 2. volumes that cut the stage kernel's tiles ----------------------------------------------
@pytest.mark.parametrize("dims", [(150, 9, 7), (5, 4, 2), (33, 17, 9)], ids=["150x9x7", "5x4x2", "33x17x9"])
def test_tile_edges(r, dims):
    """Rows longer than four 32-texel tiles with y and z smaller than a tile; a volume smaller than the halo on
    every axis; one texel more than a tile on every axis.  The largest brush covers each whole, h = 3."""
    nx, ny, nz = dims
    vol = np.random.default_rng(nx * 1000 + ny).integers(0, 256, size=(nz, ny, nx, 4), dtype=np.uint8)
    centre, radius = (nx // 2, ny // 2, nz // 2), (255, 255, 255)
    inside, _ = ps.spec_weights(vol.shape[:3], centre, radius, 0)
    assert inside.all()
    for falloff in (0, 1):
        r.set_layout_preference(0)
        r.set_volume(vol)
        assert r.blur(centre, radius, 3, falloff, FULL) == ((0, 0, 0), dims)
        want = bs.spec_blur(vol, centre, radius, 3, falloff, FULL)
        assert (want != vol).any()
        assert_exact(r.get_volume(), want)


# ---- 3. the blurred context renders what a fresh install of the blurred volume renders ---------
@pytest.mark.parametrize("pref,lname", LAYOUTS, ids=LAYOUT_IDS)
def test_blurred_render_equals_fresh_install(r, fresh, oracle, base, pref, lname):
    setup(r, pref, base)
    assert_marches(r, lname)
    vol = base
    for name, h in (("straddle", 2), ("whole", 1)):
        centre, radius = ps.BRUSHES[name]
        before, _ = oracle_frame(oracle, vol)
        vol = bs.spec_blur(vol, centre, radius, h, 1)
        ref, ref_steps = oracle_frame(oracle, vol)
        assert (ref != before).any(), "the blur does not change the oracle's frame"
        blur(r, name, h, 1)
        assert_marches(r, lname)
        img, steps = check_frame(r, oracle, vol)
        check_fresh_install(fresh, pref, lname, vol, img, steps)


# ---- 4. one stream, no host wait ---------------------------------------------------------------
@pytest.mark.parametrize("pref,lname", LAYOUTS, ids=LAYOUT_IDS)
def test_two_blurs_then_render_rects_on_a_side_stream(r, oracle, base, pref, lname):
    """`interior` at h = 3 reads texels that `straddle` has just rewritten: the second blur sees the first one's
    bytes, and the footprints' re-render sees both, with one synchronise at the end."""
    setup(r, pref, base)
    assert_marches(r, lname)
    buf = r.render(W, H, FMT_RGBA32F)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    boxes = [blur(r, "straddle", 2, 1, stream=s), blur(r, "interior", 3, 0, FULL, stream=s)]
    rects = r.update_footprints(boxes, W, H)
    r.render_rects(buf, rects, FMT_RGBA32F, stream=s)
    s.synchronize()
    once = bs.spec_blur(base, *ps.BRUSHES["straddle"], 2, 1)
    twice = bs.spec_blur(once, *ps.BRUSHES["interior"], 3, 0, FULL)
    assert (twice != bs.spec_blur(base, *ps.BRUSHES["interior"], 3, 0, FULL))[19:28].any(), "the blurs do not interact"
    assert_exact(r.get_volume(), twice)
    want, want_steps = oracle_frame(oracle, twice)
    assert_exact(buf.cpu().numpy(), want)
    img, steps = frame(r)
    assert_exact(img, want)
    assert steps == want_steps


# ---- 5. uniform channels on the recipe volume --------------------------------------------------


@pytest.mark.parametrize("pref,lname", UNIFORM_LAYOUTS, ids=[n for _, n in UNIFORM_LAYOUTS])
def test_uniform_channel(r, fresh, oracle, recipe_volume, pref, lname):
    vol, g = recipe_volume
    centre, radius = (15, 17, 14), (12, 10, 13)
    setup(r, pref, vol)
    assert r.get_option("uniform_mask") & 2 and r.kernel_variant.endswith("_uG")
    r.blur(centre, radius, 2, 1, FULL)                 # a blur of all four channels cannot break G
    blurred = bs.spec_blur(vol, centre, radius, 2, 1, FULL)
    assert (blurred != vol).any() and (blurred[..., 1] == g).all()
    assert r.get_option("uniform_mask") & 2 and r.kernel_variant.endswith("_uG")
    img, steps = check_frame(r, oracle, blurred)
    check_fresh_install(fresh, pref, lname, blurred, img, steps)
    assert fresh.kernel_variant.endswith("_uG")
    # a paint breaks G; the blur that follows spreads the dab and still renders exactly
    value = (0, (g + 120) % 256, 0, 0)
    r.paint((16, 16, 16), (3, 3, 3), ps.SET, 0, value, (0, 255, 0, 0))
    painted = ps.spec_apply(blurred, (16, 16, 16), (3, 3, 3), ps.SET, 0, value, (0, 255, 0, 0))
    r.blur(centre, radius, 1, 0, FULL)
    final = bs.spec_blur(painted, centre, radius, 1, 0, FULL)
    assert len(np.unique(final[..., 1])) > 2
    assert r.get_option("uniform_mask") & 2 == 0
    assert_marches(r, lname)
    check_frame(r, oracle, final)


# ---- 6. the staging scratch --------------------------------------------------------------------
def test_scratch(base):
    with vr.Renderer(0) as rr:
        assert rr.get_option("blur_scratch_kib") == 0
        rr.set_volume(base)
        assert rr.get_option("blur_scratch_kib") == 0
        assert blur(rr, "miss", 1, 0) is None
        assert rr.get_option("blur_scratch_kib") == 0            # no launch, no scratch
        box = blur(rr, "straddle", 1, 0)                         # 33 x 9 x 5 texels x 3 channels
        need = 3 * box[1][0] * box[1][1] * box[1][2]
        assert rr.get_option("blur_scratch_kib") == 1024 >= (need + 1023) // 1024   # rounded up to 1 MiB
        blur(rr, "texel", 3, 1)
        assert rr.get_option("blur_scratch_kib") == 1024         # a smaller call keeps what is held
        big = np.zeros((80, 128, 128, 4), np.uint8)              # 4 channels x 1 310 720 texels = 5 MiB exactly
        big[40, 64, 64] = 255
        rr.set_volume(big)
        assert rr.get_option("blur_scratch_kib") == 1024         # kept across installs
        centre, radius = (64, 64, 40), (255, 255, 255)
        assert rr.blur(centre, radius, 1, 0, FULL) == ((0, 0, 0), (128, 128, 80))
        assert rr.get_option("blur_scratch_kib") == 5120         # grown to the need
        assert_exact(rr.get_volume(), bs.spec_blur(big, centre, radius, 1, 0, FULL))
        rr.blur((3, 3, 3), (2, 2, 2), 2, 1)
        assert rr.get_option("blur_scratch_kib") == 5120
        rr.set_option("blur_scratch_kib", 0)
        assert rr.get_option("blur_scratch_kib") == 0
        rr.set_option("blur_scratch_kib", 6000)                  # a reserve: at least 6000 KiB, in whole MiB
        assert rr.get_option("blur_scratch_kib") == 6144
        rr.set_volume(base)
        blur(rr, "whole", 3, 1, FULL)                            # within the reserve
        assert rr.get_option("blur_scratch_kib") == 6144
        assert_exact(rr.get_volume(), bs.spec_blur(base, *ps.BRUSHES["whole"], 3, 1, FULL))
        rr.set_option("blur_scratch_kib", 100)                   # a smaller reserve does not shrink it
        assert rr.get_option("blur_scratch_kib") == 6144
        with pytest.raises(vr.VRError):
            rr.set_option("blur_scratch_kib", -1)


# ---- 7. undo and refusals ----------------------------------------------------------------------
def test_undo(r, base):
    r.set_layout_preference(0)
    r.set_volume(base)
    centre, radius = ps.BRUSHES["straddle"]
    origin, extent = vr.brush_box(vr.make_brush(centre, radius), (NX, NY, NZ))
    saved = r.get_volume_box(origin, extent)
    assert blur(r, "straddle", 3, 1) == (origin, extent)
    assert (r.get_volume() != base).any()
    r.update_volume(saved, origin)
    assert_exact(r.get_volume(), base)


def test_refusals(r, base):
    setup(r, 0, base)
    good = dict(centre=(17, 11, 23), radius=(3, 2, 4))
    bad = [dict(good, half_width=0), dict(good, half_width=4), dict(good, half_width=-1), dict(good, falloff=2),
           dict(good, radius=(3, 256, 4)), dict(good, radius=(-1, 2, 4))]
    for kw in bad:
        with pytest.raises(vr.VRError) as e:
            r.blur(**kw)
        assert e.value.status == 1 and "vr_blur" in str(e.value), kw   # VR_ERR_INVALID
        assert np.array_equal(r.get_volume(), base)
    for op in (ps.ADD, ps.SUB, 3, -1):
        b = vr.make_brush(op=op, **good)
        with pytest.raises(vr.VRError) as e:
            _lib.call("vr_blur", r._ctx, ctypes.byref(b), 1, None)
        assert e.value.status == 1 and "vr_blur" in str(e.value), op
        assert np.array_equal(r.get_volume(), base)
    b = vr.make_brush(**good)
    b.reserved[1] = 7
    with pytest.raises(vr.VRError) as e:
        _lib.call("vr_blur", r._ctx, ctypes.byref(b), 1, None)
    assert e.value.status == 1
    with pytest.raises(vr.VRError) as e:
        _lib.call("vr_blur", r._ctx, None, 1, None)
    assert e.value.status == 1
    assert r.blur((-10, -10, -10), (4, 4, 4)) is None             # a miss is VR_OK
    assert r.blur(strength=(0, 0, 0, 0), **good) is not None      # nothing to do is VR_OK too
    assert np.array_equal(r.get_volume(), base)
    check_needs_a_volume(r, lambda rr: rr.blur(**good))
    assert np.array_equal(r.get_volume(), base)
