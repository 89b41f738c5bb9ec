"""The split fetch of the QUAD kernels (option "quad_split"):
the four lanes of a quad, which hold one ray, load the two z-slices of two
consecutive steps between them and exchange the packed texels through DPP.
Every check is exact: each of the four targets of vr_render_group equals the
plain vr_render of the same camera byte for byte.  Which kernel ran is read from
the counters "quad_launches" and "quad_split_launches"; "quad_split" = 0 must
give the same bytes from the QUAD kernel without the split.

Set-up of tests/test_gpu_quad.py: the 40^3 recipe volume (one uniform channel: the
_u instance, three loaded taps) or a random 40^3 volume (the general instance,
four taps; it has a QUAD kernel with early-out or non-zero tap offsets), 64x48
and 70x37 so that quads fall off the right and the bottom edge, targets
pre-filled with the sentinel 0xA5.

The march runs in pairs of steps, so max_steps 1, 2, 15 and 16 cover the pair
tail and odd lengths.  At the default step_scale 4 no ray of these frames has
more than 8 steps (lengths 1 to 8 all occur), so the same cases run at
step_scale 1 too, where 15 and 16 do cut the long rays.

The early-out must be able to end a ray on the first and on the second step of
a pair.  At early_out 0.05 it ends no ray of a 16-step frame (the CPU oracle's
final transmittance is above 0.85 everywhere), so next to 0.0 and 0.05 the
early-out cases run at 0.98, where the oracle ends 119 rays of the 70x37 recipe
frame (14 after an odd number of steps) and 255 of the random volume's (73).
test_early_out_lands_on_both_steps_of_a_pair reads the executed steps of every
ray from vr_query_rect and checks that both parities occur.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from quad_cases import (BRICK4832, COL48, LAYOUTS, N, SCALES, SIZE_IDS, SIZES, STEPS, cam, check_option, group,  # noqa: E402,F401
                        plain, random_volume_bytes, scrolled, setup)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import volumetricrenderer_amd as vr
from volumetricrenderer_amd._lib import VRError  # noqa: E402

EARLY = [0.05, 0.98]   # ends no ray; ends rays on both steps of a pair
EARLY_IDS = ["early_0.05", "early_0.98"]


@pytest.fixture(scope="module")
def r():
    with vr.Renderer(0) as rr:
        rr.generate_volume(vr.scaled_recipe(N))
        yield rr
        rr.set_option("quad_split", 1)


@pytest.fixture(scope="module")
def random_volume():
    return random_volume_bytes()


def check_split(rr, size, c=None, **band):
    """The split-fetch launch, then the same launch with quad_split = 0, against the plain render."""
    return check_option(rr, "quad_split", size, c=c, **band)


@SCALES
@pytest.mark.parametrize("steps", [1, 2, 15, 16])
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
@LAYOUTS
def test_u_instance(r, pref, size, steps, scale):
    """Three loaded taps, zero offsets, no early-out: the headline instance."""
    setup(r, pref, max_steps=steps, step_scale=scale)
    r.set_shader_data(*cam(size))
    assert ("col48" if pref == COL48 else "brick4832") in r.kernel_variant and "_u" in r.kernel_variant
    want = check_split(r, size)
    assert not (want.view(np.uint32) == 0xA5A5A5A5).any()   # the plain render wrote every pixel


@pytest.mark.parametrize("early", [0.0] + EARLY, ids=["no_early_out"] + EARLY_IDS)
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
@LAYOUTS
def test_early_out(r, pref, size, early):
    """The recipe volume: early-out 0 is the _u instance, early-out on the general one with EARLY."""
    setup(r, pref, early_out=early)
    check_split(r, size)


@SCALES
@pytest.mark.parametrize("early", EARLY, ids=EARLY_IDS)
@pytest.mark.parametrize("steps", [1, 2, 15, 16])
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
        check_split(r, size)
    finally:
        r.generate_volume(vr.scaled_recipe(N))


@pytest.mark.parametrize("volume", ["recipe", "random"])
def test_early_out_lands_on_both_steps_of_a_pair(r, random_volume, volume):
    """Rays that the early-out ends do so after an odd number of steps (the first step of a pair)
    and after an even number (the second), in the 70x37 frames that test_early_out and
    test_general_instance_early_out render at early_out 0.98."""
    size = SIZES[1]
    setup(r)
    try:
        if volume == "random":
            r.set_volume(random_volume)
        r.set_shader_data(*cam(size))
        whole = (0, 0, size[0], size[1])
        full = vr.ray_records(r.query_rect(whole, *size))["steps"]
        r.set_march(vr.march_defaults(max_steps=STEPS, early_out=EARLY[1]))
        cut = vr.ray_records(r.query_rect(whole, *size))["steps"]
        ended = cut[(full > 0) & (cut < full)]
        odd, even = int((ended % 2 == 1).sum()), int((ended % 2 == 0).sum())
        print(f"{volume}: {ended.size} rays ended early, {odd} after an odd and {even} after an even number of steps; "
              f"counts {np.bincount(ended, minlength=STEPS + 1).tolist()}")
        assert odd > 0 and even > 0
    finally:
        if volume == "random":
            r.generate_volume(vr.scaled_recipe(N))


@pytest.mark.parametrize("early", [0.0] + EARLY, ids=["no_early_out"] + EARLY_IDS)
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
@LAYOUTS
def test_equal_tap_offsets(r, pref, size, early):
    """Non-zero tap offsets, the same in the four frames: the ZO = false instances (four taps)."""
    setup(r, pref, early_out=early)
    c = scrolled(size)
    r.set_shader_data(*c)
    assert "_clamp" in r.kernel_variant and "_u" not in r.kernel_variant
    check_split(r, size, c=c)


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_band_target(r, size, flip):
    setup(r)
    check_split(r, size, band_rows=16, band_stride=2, band_first=0, band_flip=flip)
    check_split(r, size, band_rows=16, band_stride=2, band_first=1, band_flip=-flip)


@pytest.mark.parametrize("size", [(128, 96), (134, 96)], ids=["128x96", "134x96"])
def test_empty_tiles_are_filled(r, size):
    """A small box: most tiles of the lists are empty and filled (empty_fill 1), in all four targets."""
    setup(r, box_min=(-0.25, -0.25, -0.25), box_max=(0.25, 0.25, 0.25))
    want = check_split(r, size)
    assert r.get_option("region_empty_tiles") > 0
    assert not (want.view(np.uint32) == 0xA5A5A5A5).any()


def test_option_range(r):
    with pytest.raises(VRError):
        r.set_option("quad_split", 2)
    assert r.get_option("quad_split") == 1
