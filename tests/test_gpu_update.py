"""Partial volume updates on the GPU: vr_update_volume / vr_update_volume_device
against the CPU oracle and against a fresh install of the patched volume.

Every fast layout stores a texel more than once -- the footprint words of
corner8 / cornerh hold it under two positions per axis, the apron bricks of
brick4832 / col48 repeat boundary texels in the neighbouring brick, and the
clamp-to-edge copies at padded 0 and N + 1 repeat the edge texels -- so the
boxes below sit on exactly those places.  The volume is 37 x 22 x 45: no axis
is a multiple of a brick edge (3, 4, 7, 31, 32), and brick4832 has two bricks
per axis.  Every comparison is exact (frames bit for bit, step counters equal).

The camera is the reference camera (reference_shader_data, aspect 1) at 64 x 64
and 32 steps.  A march that sparse samples a given corner texel from few
angles only, so each single-corner box renders from the (phi, theta) of a
30-degree grid at which the ORACLE's frame changes in the most pixels when
that texel is inverted (6 to 11 pixels; at phi = theta = 0 six of the eight
corners change nothing, and "the frame differs" could not hold).
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from brush_harness import (H, LAYOUT_IDS, LAYOUTS, W, assert_exact, assert_marches, base, check_frame,  # noqa: E402,F401
                           check_fresh_install, frame, fresh, oracle_frame, r, setup)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import volumetricrenderer_amd as vr
from volumetricrenderer_amd import _lib  # noqa: E402
from volumetricrenderer_amd._lib import FMT_RGBA32F  # noqa: E402

NX, NY, NZ = 37, 22, 45
UNIFORM_VARIANTS = {12, 14, 15}   # the layouts whose march has the _uX (no loads for one channel) kernels

# name -> (origin (x0, y0, z0), extent (bx, by, bz), camera (phi, theta))
BOXES = {
    "interior_texel": ((17, 11, 23), (1, 1, 1), (0.0, 0.0)),
    "corner_000": ((0, 0, 0), (1, 1, 1), (180.0, 60.0)),
    "corner_x00": ((NX - 1, 0, 0), (1, 1, 1), (60.0, -60.0)),
    "corner_0y0": ((0, NY - 1, 0), (1, 1, 1), (240.0, 60.0)),
    "corner_xy0": ((NX - 1, NY - 1, 0), (1, 1, 1), (30.0, -60.0)),
    "corner_00z": ((0, 0, NZ - 1), (1, 1, 1), (180.0, 0.0)),
    "corner_x0z": ((NX - 1, 0, NZ - 1), (1, 1, 1), (90.0, 0.0)),
    "corner_0yz": ((0, NY - 1, NZ - 1), (1, 1, 1), (270.0, 0.0)),
    "corner_xyz": ((NX - 1, NY - 1, NZ - 1), (1, 1, 1), (0.0, 0.0)),
    # numpy shape (5, 9, 34, 4) at origin (2, 6, 30): straddles a brick boundary on every axis of
    # every layout at odd offsets -- x 2..35, y 6..14 (7 | 8, Ba 7 and 4), z 30..34 (30 | 31, 31 | 32)
    "straddle_5x9x34": ((2, 6, 30), (34, 9, 5), (0.0, 0.0)),
    "z_slab": ((0, 0, NZ - 1), (NX, NY, 1), (0.0, 0.0)),
    "x_row": ((0, 0, 0), (NX, 1, 1), (180.0, 60.0)),
    "whole_volume": ((0, 0, 0), (NX, NY, NZ), (0.0, 0.0)),
}


def straddle_box():
    return BOXES["straddle_5x9x34"]


def patch_into(vol, box, origin):
    x0, y0, z0 = origin
    bz, by, bx, _ = box.shape
    out = vol.copy()
    out[z0:z0 + bz, y0:y0 + by, x0:x0 + bx] = box
    return out


def check_against_oracle_and_fresh(rr, fresh, oracle, pref, name, patched, angles=(0.0, 0.0)):
    assert_marches(rr, name)
    img, steps = check_frame(rr, oracle, patched, angles)
    check_fresh_install(fresh, pref, name, patched, img, steps, angles)
    return img


@pytest.mark.parametrize("boxname", list(BOXES))
@pytest.mark.parametrize("pref,name", LAYOUTS, ids=LAYOUT_IDS)
def test_box_placement(r, fresh, oracle, base, pref, name, boxname):
    origin, (bx, by, bz), angles = BOXES[boxname]
    x0, y0, z0 = origin
    # every byte differs from the original (255 - v != v), so a no-op cannot pass
    box = 255 - base[z0:z0 + bz, y0:y0 + by, x0:x0 + bx]
    patched = patch_into(base, box, origin)
    setup(r, pref, base, angles)
    assert_marches(r, name)
    pre, _ = frame(r)
    assert_exact(pre, oracle_frame(oracle, base, angles)[0])
    r.update_volume(box, origin)
    img = check_against_oracle_and_fresh(r, fresh, oracle, pref, name, patched, angles)
    assert (img != pre).any(), "the update did not change the frame"


@pytest.mark.parametrize("pref,name", LAYOUTS, ids=LAYOUT_IDS)
def test_overlapping_updates_in_sequence(r, fresh, oracle, base, pref, name):
    """Three boxes that overlap pairwise, from device memory: the last writer
    wins, as in numpy."""
    rng = np.random.default_rng(7)
    boxes = [((0, 0, 5), (20, 12, 20)), ((2, 6, 11), (5, 9, 34)), ((4, 3, 20), (33, 10, 9))]
    setup(r, pref, base)
    patched = base
    for origin, (bx, by, bz) in boxes:
        box = rng.integers(0, 256, size=(bz, by, bx, 4), dtype=np.uint8)
        r.update_volume(torch.from_numpy(box).cuda(), origin)
        patched = patch_into(patched, box, origin)
    check_against_oracle_and_fresh(r, fresh, oracle, pref, name, patched)


@pytest.mark.parametrize("pref,name", LAYOUTS, ids=LAYOUT_IDS)
def test_uniform_channel(r, oracle, base, pref, name):
    """G is the constant 137: an update that keeps it keeps the uniform bit and
    the _uG kernel; one texel at 138 clears both before the next render.  The
    _uG suffix exists for brick4832, cornerh and col48 only (vr_kernel_variant);
    the mask is checked for every layout."""
    vol = base.copy()
    vol[..., 1] = 137
    origin, (bx, by, bz), _ = straddle_box()
    keep = np.random.default_rng(11).integers(0, 256, size=(bz, by, bx, 4), dtype=np.uint8)
    keep[..., 1] = 137
    one = vol[23:24, 11:12, 17:18].copy()
    one[..., 1] = 138
    try:
        for skip in (1, 0):
            setup(r, pref, vol)
            r.set_option("uniform_skip", skip)
            assert r.get_option("uniform_mask") & 2
            assert r.kernel_variant.endswith("_uG") == (skip == 1 and pref in UNIFORM_VARIANTS)
            r.update_volume(keep, origin)
            patched = patch_into(vol, keep, origin)
            assert r.get_option("uniform_mask") & 2
            assert r.kernel_variant.endswith("_uG") == (skip == 1 and pref in UNIFORM_VARIANTS)
            assert_marches(r, name)
            img, steps = frame(r)
            ref, ref_steps = oracle_frame(oracle, patched)
            assert_exact(img, ref)
            assert steps == ref_steps
            r.update_volume(one, (17, 11, 23))
            patched = patch_into(patched, one, (17, 11, 23))
            assert r.get_option("uniform_mask") & 2 == 0
            assert not r.kernel_variant.endswith("_uG")
            assert_marches(r, name)
            img, steps = frame(r)
            ref, ref_steps = oracle_frame(oracle, patched)
            assert_exact(img, ref)
            assert steps == ref_steps
            assert np.array_equal(r.get_volume(), patched)
    finally:
        r.set_option("uniform_skip", 1)


@pytest.mark.parametrize("pref,name", LAYOUTS, ids=LAYOUT_IDS)
def test_stream_order(r, oracle, base, pref, name):
    """update_volume(..., stream=s) directly followed by a render on s, four
    times with a moving 8^3 box and no host synchronisation in between: every
    frame is the oracle's for that step."""
    rng = np.random.default_rng(13)
    origins = [(0, 0, 0), (9, 5, 13), (20, 10, 25), (29, 14, 37)]
    boxes = [rng.integers(0, 256, size=(8, 8, 8, 4), dtype=np.uint8) for _ in origins]
    dev = [torch.from_numpy(b).cuda() for b in boxes]
    outs = [r.alloc_target(W, H, FMT_RGBA32F) for _ in origins]
    cnts = [torch.zeros(1, dtype=torch.int64, device="cuda") for _ in origins]
    setup(r, pref, base)
    assert_marches(r, name)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    for k, origin in enumerate(origins):
        r.update_volume(dev[k], origin, stream=s)
        r.render(W, H, FMT_RGBA32F, out=outs[k], stream=s, step_counter=cnts[k])
    s.synchronize()
    patched = base
    for k, origin in enumerate(origins):
        patched = patch_into(patched, boxes[k], origin)
        ref, ref_steps = oracle_frame(oracle, patched)
        assert_exact(outs[k].cpu().numpy(), ref)
        assert int(cnts[k].item()) == ref_steps
    assert np.array_equal(r.get_volume(), patched)


def test_layout_switch_after_update(r, oracle, base):
    """Update under planar, then prefer cornerh: the lazily built layout comes
    from the patched planes."""
    origin, (bx, by, bz), _ = straddle_box()
    box = 255 - base[origin[2]:origin[2] + bz, origin[1]:origin[1] + by, origin[0]:origin[0] + bx]
    setup(r, 1, base)
    assert_marches(r, "planar")
    r.update_volume(box, origin)
    r.set_layout_preference(14)
    assert_marches(r, "cornerh")
    img, steps = frame(r)
    ref, ref_steps = oracle_frame(oracle, patch_into(base, box, origin))
    assert_exact(img, ref)
    assert steps == ref_steps


@pytest.mark.parametrize("pref,name", LAYOUTS[1:], ids=LAYOUT_IDS[1:])
def test_mirror_path(r, oracle, base, pref, name):
    """A MediaScroll offset forces grid_planar_mirror while the fast layout is
    held: after the update the mirror frame (the planes) is exact, and with
    the offset removed so is the fast layout's -- both copies were patched."""
    origin, (bx, by, bz), _ = straddle_box()
    box = 255 - base[origin[2]:origin[2] + bz, origin[1]:origin[1] + by, origin[0]:origin[0] + bx]
    patched = patch_into(base, box, origin)
    setup(r, pref, base)
    assert_marches(r, name)
    osd, gsd = vr.reference_shader_data(1.0)
    for col, vals in enumerate([(0.0, 3.7, -2.2, 1.3), (0.0, -0.6, 5.1, -7.9), (0.0, 1.9, 0.4, -1.1)]):
        for row, v in enumerate(vals):
            gsd.media_scroll[col * 4 + row] = v
    r.set_shader_data(osd, gsd)
    assert r.kernel_variant == "grid_planar_mirror"
    r.update_volume(box, origin)
    assert r.kernel_variant == "grid_planar_mirror"
    img, steps = frame(r)
    ref, ref_steps = oracle_frame(oracle, patched, gsd=gsd)
    assert_exact(img, ref)
    assert steps == ref_steps
    r.set_shader_data(*vr.reference_shader_data(1.0))
    assert_marches(r, name)
    img, steps = frame(r)
    ref, ref_steps = oracle_frame(oracle, patched)
    assert_exact(img, ref)
    assert steps == ref_steps


def test_refusals(r, base):
    setup(r, 0, base)
    host = np.zeros_like(base)
    devt = torch.zeros((NZ, NY, NX, 4), dtype=torch.uint8, device="cuda")
    hp, dp = host.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(devt.data_ptr())
    bad = [
        ((-1, 0, 0), (1, 1, 1)), ((0, -1, 0), (1, 1, 1)), ((0, 0, -1), (1, 1, 1)),      # origin out of range
        ((NX, 0, 0), (1, 1, 1)), ((0, NY, 0), (1, 1, 1)), ((0, 0, NZ), (1, 1, 1)),
        ((30, 0, 0), (8, 1, 1)), ((0, 15, 0), (1, 8, 1)), ((0, 0, 38), (1, 1, 8)),      # past the far edge by one
        ((2, 6, 30), (5, 9, 34)),
        ((1, 0, 0), (NX, NY, NZ)),
        ((0, 0, 0), (0, 1, 1)), ((0, 0, 0), (1, 0, 1)), ((0, 0, 0), (1, 1, 0)), ((0, 0, 0), (-3, 1, 1)),   # no extent
        ((2**31 - 1, 0, 0), (2**31 - 1, 1, 1)),                                          # x0 + bx overflows an int
    ]
    for origin, ext in bad:
        for fn, args in (("vr_update_volume", (hp,)), ("vr_update_volume_device", (dp,))):
            tail = (None,) if fn.endswith("_device") else ()
            with pytest.raises(vr.VRError) as e:
                _lib.call(fn, r._ctx, *args, *origin, *ext, *tail)
            assert e.value.status == 1, (fn, origin, ext)   # VR_ERR_INVALID
            assert np.array_equal(r.get_volume(), base)
    for fn, tail in (("vr_update_volume", ()), ("vr_update_volume_device", (None,))):   # null data
        with pytest.raises(vr.VRError) as e:
            _lib.call(fn, r._ctx, None, 0, 0, 0, 1, 1, 1, *tail)
        assert e.value.status == 1
        assert np.array_equal(r.get_volume(), base)
    assert r.volume_dims() == (NX, NY, NZ)
    with vr.Renderer(0) as empty:   # no volume installed
        for fn, args, tail in (("vr_update_volume", (hp,), ()), ("vr_update_volume_device", (dp,), (None,))):
            with pytest.raises(vr.VRError) as e:
                _lib.call(fn, empty._ctx, *args, 0, 0, 0, 1, 1, 1, *tail)
            assert e.value.status == 3   # VR_ERR_NO_VOLUME
    with pytest.raises(ValueError):   # the wrapper's shape and contiguity checks
        r.update_volume(np.zeros((2, 2, 2, 3), np.uint8), (0, 0, 0))
    with pytest.raises(ValueError):
        r.update_volume(devt[:, :, ::2], (0, 0, 0))
    assert np.array_equal(r.get_volume(), base)
