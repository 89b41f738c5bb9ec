"""The paired fetch of the QUAD kernels' step rounds (option "quad_pairs", DESIGN.md sec.
5.1.16): a round of four steps still blends one step per lane, but its loads are issued in
slice pairs -- in each of a tap's two load instructions a lane loads one z-slice of another
lane's step, shifts and packs it, and the owner reads its two slices back through DPP.  Every
check is exact: each of the four targets of vr_render_group equals the plain vr_render of the
same camera byte for byte, with "quad_pairs" 1 and with 0 (every lane loads its own step).
Which kernel ran is read from the counters "quad_launches", "quad_split_launches",
"quad_steps_launches" and "quad_pairs_launches"; a paired launch is a step-round, a split and
a QUAD launch and counts as each.

Set-up and cases of tests/test_gpu_quad_steps.py: the 40^3 recipe volume (one uniform channel:
the _u instance, three loaded taps) or a seeded random 40^3 volume (the general instance, four
taps), 64x48 and 70x37 so that quads fall off the right and the bottom edge, targets pre-filled
with the sentinel 0xA5.  A 40^3 volume spans several bricks of both layouts on every axis.

max_steps 1, 2, 3, 4, 5, 7, 8, 9 and 16 cover every tail length of a round (lanes past the
ray's end load the round's first point, so several lanes of a quad hold one offset), exactly
one round, and the pipeline's first and second refill.  At the default step_scale 4 no ray of
these frames has more than 8 steps, so every case runs at step_scale 1 too.

The early-out must be able to end a ray at each of the four positions of a round: 0.98 does in
the random volume's 70x37 frame and 0.99 in the recipe volume's.
test_early_out_lands_on_every_step_of_a_round asserts that from vr_query_rect's records.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from quad_cases import (BRICK4832, COL48, LAYOUTS, N, SCALES, SIZE_IDS, SIZES, STEPS, cam, check_option, group,  # noqa: E402,F401
                        plain, random_volume_bytes, scrolled, setup)
from quad_cases import OPTIONS  # noqa: E402

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import volumetricrenderer_amd as vr
from volumetricrenderer_amd._lib import VRError  # noqa: E402

EARLY = [0.05, 0.98, 0.99]   # ends no ray; ends rays on every step of a round (random volume; recipe volume)
EARLY_IDS = ["early_0.05", "early_0.98", "early_0.99"]
ROUND_EARLY = {"recipe": 0.99, "random": 0.98}
STEP_COUNTS = pytest.mark.parametrize("steps", [1, 2, 3, 4, 5, 7, 8, 9, 16])


@pytest.fixture(scope="module")
def r():
    with vr.Renderer(0) as rr:
        rr.generate_volume(vr.scaled_recipe(N))
        before = {k: rr.get_option(k) for k in OPTIONS}
        yield rr
        for k, v in before.items():
            rr.set_option(k, v)


@pytest.fixture(scope="module")
def random_volume():
    return random_volume_bytes()


def check_pairs(rr, size, c=None, **band):
    """The paired launch, then the same launch with quad_pairs = 0, against the plain render."""
    return check_option(rr, "quad_pairs", size, c=c, **band)


@SCALES
@STEP_COUNTS
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
@LAYOUTS
def test_u_instance(r, pref, size, steps, scale):
    """Three loaded taps, zero offsets, no early-out: the headline instance."""
    setup(r, pref, max_steps=steps, step_scale=scale)
    r.set_shader_data(*cam(size))
    assert ("col48" if pref == COL48 else "brick4832") in r.kernel_variant and "_u" in r.kernel_variant
    want = check_pairs(r, size)
    assert not (want.view(np.uint32) == 0xA5A5A5A5).any()   # the plain render wrote every pixel


@pytest.mark.parametrize("early", [0.0] + EARLY, ids=["no_early_out"] + EARLY_IDS)
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
@LAYOUTS
def test_early_out(r, pref, size, early):
    """The recipe volume: early-out 0 is the _u instance, early-out on the general one with EARLY."""
    setup(r, pref, early_out=early)
    check_pairs(r, size)


@SCALES
@pytest.mark.parametrize("early", EARLY, ids=EARLY_IDS)
@STEP_COUNTS
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
@LAYOUTS
def test_general_instance_early_out(r, random_volume, pref, size, steps, early, scale):
    """Four loaded taps: a volume without a uniform channel, early-out on (the general kernel has
    no QUAD instance for zero offsets without early-out, vr_internal.h quad_instance)."""
    setup(r, pref, max_steps=steps, early_out=early, step_scale=scale)
    try:
        r.set_volume(random_volume)
        r.set_shader_data(*cam(size))
        assert "_u" not in r.kernel_variant
        check_pairs(r, size)
    finally:
        r.generate_volume(vr.scaled_recipe(N))


@pytest.mark.parametrize("volume", ["recipe", "random"])
def test_early_out_lands_on_every_step_of_a_round(r, random_volume, volume):
    """Rays that the early-out ends do so after 4k + 1, 4k + 2, 4k + 3 and 4k + 4 steps (each lane's
    position in a round), in the 70x37 frames that test_early_out and
    test_general_instance_early_out render at early_out 0.99 (recipe volume) and 0.98 (random)."""
    size = SIZES[1]
    setup(r)
    try:
        if volume == "random":
            r.set_volume(random_volume)
        r.set_shader_data(*cam(size))
        whole = (0, 0, size[0], size[1])
        full = vr.ray_records(r.query_rect(whole, *size))["steps"]
        r.set_march(vr.march_defaults(max_steps=STEPS, early_out=ROUND_EARLY[volume]))
        cut = vr.ray_records(r.query_rect(whole, *size))["steps"]
        ended = cut[(full > 0) & (cut < full)]
        residues = np.bincount(ended % 4, minlength=4).tolist()
        print(f"{volume}, early_out {ROUND_EARLY[volume]}: {ended.size} rays ended early, by steps % 4 {residues}; "
              f"counts {np.bincount(ended, minlength=STEPS + 1).tolist()}")
        assert all(n > 0 for n in residues)
    finally:
        if volume == "random":
            r.generate_volume(vr.scaled_recipe(N))


@pytest.mark.parametrize("early", [0.0] + EARLY, ids=["no_early_out"] + EARLY_IDS)
@SCALES
@STEP_COUNTS
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
@LAYOUTS
def test_equal_tap_offsets(r, pref, size, steps, early, scale):
    """Non-zero tap offsets, the same in the four frames: the ZO = false instances (four taps)."""
    setup(r, pref, max_steps=steps, early_out=early, step_scale=scale)
    c = scrolled(size)
    r.set_shader_data(*c)
    assert "_clamp" in r.kernel_variant and "_u" not in r.kernel_variant
    check_pairs(r, size, c=c)


@SCALES
@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_band_target(r, size, flip, scale):
    setup(r, step_scale=scale)
    check_pairs(r, size, band_rows=16, band_stride=2, band_first=0, band_flip=flip)
    check_pairs(r, size, band_rows=16, band_stride=2, band_first=1, band_flip=-flip)


@SCALES
@pytest.mark.parametrize("size", [(128, 96), (134, 96)], ids=["128x96", "134x96"])
def test_empty_tiles_are_filled(r, size, scale):
    """A small box: most tiles of the lists are empty and filled (empty_fill 1), in all four targets."""
    setup(r, step_scale=scale, box_min=(-0.25, -0.25, -0.25), box_max=(0.25, 0.25, 0.25))
    want = check_pairs(r, size)
    assert r.get_option("region_empty_tiles") > 0
    assert not (want.view(np.uint32) == 0xA5A5A5A5).any()


def test_option_range(r):
    setup(r)
    with pytest.raises(VRError):
        r.set_option("quad_pairs", 2)
    assert r.get_option("quad_pairs") == 1


@pytest.mark.parametrize("off", ["quad_steps", "quad_split"])
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_without_the_step_rounds_the_option_is_idle(r, size, off):
    """quad_steps = 0 or quad_split = 0 with quad_pairs = 1: the launch those options select, exact,
    and quad_pairs_launches unmoved."""
    setup(r)
    c = cam(size)
    want = plain(r, c, size)
    r.set_option(off, 0)
    try:
        assert r.get_option("quad_pairs") == 1
        got, counts = group(r, c, size)
    finally:
        r.set_option(off, 1)
    assert counts == ((1, 1, 0, 0) if off == "quad_steps" else (1, 0, 0, 0)), f"(QUAD, split, step-round, paired) launches {counts}"
    for i in range(4):
        assert np.array_equal(got[i], want), f"frame {i} differs from the plain render"
