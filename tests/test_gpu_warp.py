"""vr_warp on the GPU: the edited volume against the numpy restatement
(tests/warp_spec.py), byte for byte, for every brush x map x filter x border x
falloff, through both paths of a tile (option warp_lds 1 and 0); volumes that
cut the tiles; the maps on the boundary of the LDS budget; a hard warp against
the transform paste; the identity; uniform channels; the frame after a warp
against a fresh install and the CPU oracle, per layout; pick -> warp ->
update_footprint -> render_rect on one side stream; the staging scratch;
refusals.  Everything is exact.

The volume is paint_spec.base_volume() (37 x 22 x 45 random bytes); frame, march
and cameras are brush_harness.py's: the reference camera at 64 x 64, 32 steps.
"""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affine_spec as af  # noqa: E402
import paint_spec as ps  # noqa: E402
import warp_spec as ws  # noqa: E402
import brush_harness  # noqa: E402
from brush_harness import (H, LAYOUT_IDS, LAYOUTS, UNIFORM_LAYOUTS, VOLUME_BRUSHES, W, assert_exact, assert_marches,  # noqa: E402,F401
                           base, check_frame, check_fresh_install, check_needs_a_volume, frame, fresh, oracle_frame, r,
                           recipe_volume)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import volumetricrenderer_amd as vr
from volumetricrenderer_amd import _lib  # noqa: E402
from volumetricrenderer_amd._lib import FMT_RGBA32F  # noqa: E402

PATHS = [(1, "lds"), (0, "gather")]


def setup(rr, pref, vol, density=1.0):
    rr.set_option("warp_lds", 1)   # the default path, whatever an earlier test left
    brush_harness.setup(rr, pref, vol, density=density)


def affine(table, filt=ws.LINEAR, border=ws.CLAMP):
    return vr.make_affine(*table, filt, border)


def warp_both_paths(rr, vol, centre, radius, a, falloff, strength, want):
    """The warp of `vol` through the LDS path and through the gather: both are `want`."""
    box = None
    for lds, _ in PATHS:
        rr.set_option("warp_lds", lds)
        rr.set_volume(vol)
        box = rr.warp(centre, radius, a, falloff, strength)
        assert_exact(rr.get_volume(), want)
    rr.set_option("warp_lds", 1)
    return box


# ---- 1. the warped volume is the specification's, by both paths ---------------------------------
@pytest.mark.parametrize("mname", list(ws.MAPS))
@pytest.mark.parametrize("name", VOLUME_BRUSHES)
def test_warped_volume_equals_the_specification(r, base, name, mname):
    r.set_layout_preference(14)
    assert r.get_option("warp_lds") == 1                  # the default
    centre, radius = ps.BRUSHES[name]
    table = ws.placed(mname, centre)
    changed = False
    for (filt, _), (border, _), (falloff, _) in itertools.product(ws.FILTERS, ws.BORDERS, ps.FALLOFFS):
        want = ws.spec_warp(base, table, filt, border, centre, radius, falloff)
        box = warp_both_paths(r, base, centre, radius, affine(table, filt, border), falloff, ws.STRENGTH, want)
        assert box == ps.spec_box(centre, radius)
        changed = changed or (want != base).any()
    if name == "miss" or mname == "identity":
        assert not changed
    if name in ("interior", "straddle", "whole", "max") and mname != "identity":
        assert changed


# ---- 2. volumes that cut the tiles ---------------------------------------------------------------
@pytest.mark.parametrize("dims", [(1, 1, 1), (3, 1, 2), (65, 2, 2), (64, 64, 1), (9, 17, 8)],
                         ids=["1x1x1", "3x1x2", "65x2x2", "64x64x1", "9x17x8"])
def test_volumes_that_cut_the_tiles(r, dims):
    """One texel; a tile smaller than a wave's texels; nine tiles along x, the last one texel wide; 64 tiles in one
    slice; partial tiles on x and y with z exactly one tile.  The brush is `whole`; the maps turn about the middle."""
    nx, ny, nz = dims
    vol = np.random.default_rng(nx * 1000 + ny).integers(0, 256, size=(nz, ny, nx, 4), dtype=np.uint8)
    centre, radius = ps.BRUSHES["whole"]
    mid = (nx // 2, ny // 2, nz // 2)
    r.set_layout_preference(0)
    changed = False
    for mname in ("rot30_axis", "push_frac", "twirl20", "pinch", "quarter", "off_source"):
        table = ws.MAPS[mname](mid, mid)
        for (filt, _), (border, _), (falloff, _) in itertools.product(ws.FILTERS, ws.BORDERS, ps.FALLOFFS):
            want = ws.spec_warp(vol, table, filt, border, centre, radius, falloff, ws.FULL)
            warp_both_paths(r, vol, centre, radius, affine(table, filt, border), falloff, ws.FULL, want)
            changed = changed or (want != vol).any()
    assert changed == (dims != (1, 1, 1))


# ---- 3. the boundary of the LDS budget -----------------------------------------------------------
def test_the_budget_boundary(r, base):
    """tests/test_warp_cpu.py asserts what these maps do: BUDGET_EXACT has a tile whose footprint is exactly the
    budget (the LDS path at its largest), BUDGET_OVER the same tile one row of texels over (the gather) next to
    tiles that fit."""
    r.set_layout_preference(0)
    centre, radius = ps.BRUSHES["whole"]
    for table in (ws.BUDGET_EXACT, ws.BUDGET_OVER):
        for (filt, _), (border, _), (falloff, _) in itertools.product(ws.FILTERS, ws.BORDERS, ps.FALLOFFS):
            want = ws.spec_warp(base, table, filt, border, centre, radius, falloff, ws.FULL)
            assert (want != base).any()
            warp_both_paths(r, base, centre, radius, affine(table, filt, border), falloff, ws.FULL, want)


# ---- 4. a hard warp is the transform paste; the identity changes nothing -------------------------
@pytest.mark.parametrize("name", ["interior", "outside_centre", "straddle", "whole"])
def test_a_hard_warp_is_clone_affine(r, fresh, base, name):
    r.set_layout_preference(0)
    fresh.set_layout_preference(0)
    centre, radius = ps.BRUSHES[name]
    changed = 0
    for mname, (filt, _), (border, _) in itertools.product(("shift_half", "rot30_axis", "far", "off_source", "twirl20", "pinch"),
                                                            ws.FILTERS, ws.BORDERS):
        a = affine(ws.placed(mname, centre), filt, border)
        fresh.set_volume(base)
        fresh.clone_affine(centre, radius, a, ps.SET, 0, ws.STRENGTH)
        want = fresh.get_volume()
        changed += bool((want != base).any())        # a SKIP map may leave every texel of a brush at the edge alone
        warp_both_paths(r, base, centre, radius, a, 0, ws.STRENGTH, want)
    assert changed >= 12


@pytest.mark.parametrize("name", VOLUME_BRUSHES)
def test_the_identity_changes_nothing(r, base, name):
    r.set_layout_preference(0)
    centre, radius = ps.BRUSHES[name]
    for (filt, _), (border, _), (falloff, _) in itertools.product(ws.FILTERS, ws.BORDERS, ps.FALLOFFS):
        for a in (affine(ws.placed("identity", centre), filt, border), vr.warp_push(centre, (0, 0, 0), filt, border)):
            warp_both_paths(r, base, centre, radius, a, falloff, ws.FULL, base)


# ---- 5. uniform channels on the recipe volume ----------------------------------------------------


@pytest.mark.parametrize("pref,lname", UNIFORM_LAYOUTS, ids=[n for _, n in UNIFORM_LAYOUTS])
def test_uniform_channel(r, fresh, oracle, recipe_volume, pref, lname):
    vol, g = recipe_volume
    centre, radius = (15, 17, 14), (6, 5, 7)
    setup(r, pref, vol)
    assert r.get_option("uniform_mask") & 2 and r.kernel_variant.endswith("_uG")
    # warps of all four channels, both filters, both paths, cannot break G
    for mname, filt, lds in (("twirl20", ws.LINEAR, 1), ("push_frac", ws.LINEAR, 0), ("pinch", ws.NEAREST, 1)):
        r.set_option("warp_lds", lds)
        table = ws.placed(mname, centre)
        r.warp(centre, radius, affine(table, filt), 1, ws.FULL)
        new = ws.spec_warp(vol, table, filt, ws.CLAMP, centre, radius, 1, ws.FULL)
        assert (new != vol).any() and (new[..., 1] == g).all()
        vol = new
        assert r.get_option("uniform_mask") & 2
    # a warp of the non-uniform channels alone leaves G's bit alone as well
    table = ws.placed("rot30_axis", centre)
    r.warp(centre, radius, affine(table), 1, (255, 0, 255, 255))
    vol = ws.spec_warp(vol, table, ws.LINEAR, ws.CLAMP, centre, radius, 1, (255, 0, 255, 255))
    assert r.get_option("uniform_mask") == 2 and r.kernel_variant.endswith("_uG")
    img, steps = check_frame(r, oracle, vol)
    check_fresh_install(fresh, pref, lname, vol, img, steps)
    assert_marches(r, lname)


# ---- 6. the frame after a warp; pick -> warp -> update_footprint -> render_rect on one stream ----
@pytest.mark.parametrize("pref,lname", LAYOUTS, ids=LAYOUT_IDS)
def test_render_after_a_warp(r, fresh, oracle, base, pref, lname):
    setup(r, pref, base)
    assert_marches(r, lname)
    centre, radius = ps.BRUSHES["straddle"]
    table = ws.placed("twirl20", centre)
    r.warp(centre, radius, affine(table), 1, ws.FULL)
    warped = ws.spec_warp(base, table, ws.LINEAR, ws.CLAMP, centre, radius, 1, ws.FULL)
    assert_exact(r.get_volume(), warped)
    want, want_steps = oracle_frame(oracle, warped)
    before, _ = oracle_frame(oracle, base)
    assert (want != before).any(), "the warp does not change the frame"
    img, steps = frame(r)
    assert_exact(img, want)
    assert steps == want_steps
    assert_marches(r, lname)
    check_fresh_install(fresh, pref, lname, warped, img, steps)


@pytest.mark.parametrize("pref,lname", LAYOUTS, ids=LAYOUT_IDS)
def test_pick_warp_rerender_on_a_side_stream(r, oracle, base, pref, lname):
    """pick (which returns the texel to the host), then warp, update_footprint and render_rect queued on a side
    stream with one synchronise at the end: the patched frame is the whole frame of the specification's volume.
    A push by (3, -2, 0.5) texels under the picked pixel, within a reserved scratch."""
    density = 32.0   # dense enough for rays to pass the 0.5 transmittance threshold (a hit)
    setup(r, pref, base, density=density)
    r.set_option("blur_scratch_kib", 1024)
    assert_marches(r, lname)
    rec = vr.ray_records(r.query_rect((0, 0, W, H), W, H, 0.5))
    hits = np.argwhere(rec["hit_step"] >= 0)
    assert len(hits) > 0, "no ray has a hit"
    py, px = (int(v) for v in hits[np.argmin(((hits - (H // 2, W // 2)) ** 2).sum(axis=1))])
    one, texel = r.pick(px, py, W, H, 0.5)
    assert one["hit_step"] >= 0 and texel is not None
    centre, radius = tuple(int(v) for v in texel), (9, 6, 5)
    a = vr.warp_push(centre, (3 << 16, -(2 << 16), 0x8000))
    buf = r.render(W, H, FMT_RGBA32F)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    box = r.warp(centre, radius, a, 1, ws.FULL, stream=s)
    assert box == ps.spec_box(centre, radius)
    rect = r.update_footprint(box[0], box[1], W, H)
    r.render_rect(buf, rect, FMT_RGBA32F, stream=s)
    s.synchronize()
    assert r.get_option("blur_scratch_kib") == 1024
    table = (tuple(tuple(row) for row in a.m), tuple(a.pivot), tuple(a.origin))
    warped = ws.spec_warp(base, table, ws.LINEAR, ws.CLAMP, centre, radius, 1, ws.FULL)
    assert_exact(r.get_volume(), warped)
    want, want_steps = oracle_frame(oracle, warped, density=density)
    before, _ = oracle_frame(oracle, base, density=density)
    assert (want != before).any(), "the warp does not change the frame"
    assert_exact(buf.cpu().numpy(), want)
    img, steps = frame(r)
    assert_exact(img, want)
    assert steps == want_steps


# ---- 7. the staging scratch ----------------------------------------------------------------------
def test_scratch(base):
    centre, radius = ps.BRUSHES["interior"]
    table = ws.placed("twirl20", centre)
    with vr.Renderer(0) as rr:
        assert rr.get_option("blur_scratch_kib") == 0
        rr.set_volume(base)
        assert rr.warp(*ps.BRUSHES["miss"], affine(table)) is None
        assert rr.warp(centre, radius, affine(table), strength=(0, 0, 0, 0)) is not None
        assert rr.get_option("blur_scratch_kib") == 0                 # no launch, no scratch
        rr.warp(centre, radius, affine(table), 1, ws.STRENGTH)
        vol = ws.spec_warp(base, table, ws.LINEAR, ws.CLAMP, centre, radius, 1)
        assert_exact(rr.get_volume(), vol)
        assert rr.get_option("blur_scratch_kib") == 1024               # the blur's scratch, rounded up to 1 MiB
        # the whole volume, three painted channels: 3 * 37 * 22 * 45 bytes fit what is held -- it does not grow
        rr.warp(*ps.BRUSHES["whole"], affine(table), 1, ws.STRENGTH)
        vol = ws.spec_warp(vol, table, ws.LINEAR, ws.CLAMP, *ps.BRUSHES["whole"], 1)
        assert_exact(rr.get_volume(), vol)
        assert rr.get_option("blur_scratch_kib") == 1024
        # the blur shares it
        rr.blur(centre, radius, 1)
        assert rr.get_option("blur_scratch_kib") == 1024


# ---- 8. refusals ---------------------------------------------------------------------------------
def test_refusals(r, base):
    setup(r, 0, base)
    centre, radius = ps.BRUSHES["interior"]
    good = affine(ws.placed("twirl20", centre))
    kib = r.get_option("blur_scratch_kib")

    def bad_maps():
        for k, v in (("filter", 2), ("filter", -1), ("border", 2), ("border", -1), ("reserved", 1)):
            a = affine(ws.placed("identity", centre))
            setattr(a, k, v)
            yield a
        for v in (256 * 65536 + 1, -256 * 65536 - 1, -2**31):
            a = affine(ws.placed("identity", centre))
            a.m[2][0] = v
            yield a
        yield affine((af.I3, centre, (centre[0] * 65536 - ws.MAX_DISP16 - 1, centre[1] * 65536, centre[2] * 65536)))

    for a in bad_maps():
        with pytest.raises(vr.VRError) as e:
            r.warp(centre, radius, a)
        assert e.value.status == 1 and "vr_warp" in str(e.value)         # VR_ERR_INVALID
        assert np.array_equal(r.get_volume(), base)
    for kw in (dict(falloff=2), dict(radius=(3, 256, 4)), dict(radius=(-1, 2, 4))):
        with pytest.raises(vr.VRError) as e:
            r.warp(**dict(dict(centre=centre, radius=radius, affine=good), **kw))
        assert e.value.status == 1 and "vr_warp" in str(e.value), kw
    for op in (ps.ADD, ps.SUB, 3, -1):
        b = vr.make_brush(centre, radius, op, 1)
        with pytest.raises(vr.VRError) as e:
            _lib.call("vr_warp", r._ctx, ctypes.byref(b), ctypes.byref(good), None)
        assert e.value.status == 1 and "vr_warp" in str(e.value)
    for k in range(2):
        b = vr.make_brush(centre, radius)
        b.reserved[k] = 7
        with pytest.raises(vr.VRError):
            _lib.call("vr_warp", r._ctx, ctypes.byref(b), ctypes.byref(good), None)
    b = vr.make_brush(centre, radius)
    for args in ((r._ctx, None, ctypes.byref(good), None), (r._ctx, ctypes.byref(b), None, None), (None, ctypes.byref(b), ctypes.byref(good), None)):
        with pytest.raises(vr.VRError) as e:
            _lib.call("vr_warp", *args)
        assert e.value.status == 1 and "null" in str(e.value)
    for v in (2, -1):
        with pytest.raises(vr.VRError):
            r.set_option("warp_lds", v)
    assert np.array_equal(r.get_volume(), base)
    assert r.get_option("blur_scratch_kib") == kib                      # nothing launched, nothing allocated
    # exactly at the limit the map is accepted
    at = (af.I3, centre, (centre[0] * 65536 - ws.MAX_DISP16, centre[1] * 65536, centre[2] * 65536))
    r.warp(centre, radius, affine(at), 1, ws.STRENGTH)
    assert_exact(r.get_volume(), ws.spec_warp(base, at, ws.LINEAR, ws.CLAMP, centre, radius, 1))
    r.set_volume(base)
    assert r.warp(*ps.BRUSHES["miss"], good) is None                    # a miss is VR_OK
    assert r.warp(centre, radius, good, strength=(0, 0, 0, 0)) is not None   # nothing to do is VR_OK too
    assert np.array_equal(r.get_volume(), base)
    check_needs_a_volume(r, lambda rr: rr.warp(centre, radius, good))
    assert np.array_equal(r.get_volume(), base)
