"""What the brush test modules share: the frame and march every one of them renders, the oracle's
frames, the contexts, and the assertion blocks that recur from brush to brush.

The volume is paint_spec.base_volume(): 37 x 22 x 45 (no axis a multiple of a brick edge).  The frame
is the reference camera's at 64 x 64 and 32 steps.  Everything is exact: volumes byte for byte, frames
bit for bit, step counters equal.

A brush's test module imports the names it uses, fixtures included (an imported module-scoped fixture
still has one instance per importing module), and holds only what is particular to that brush: its
specification's cases, its bad-argument lists and struct refusals, its scratch arithmetic.

This module imports without a GPU -- the CPU modules use `assert_exact` and `base` -- so the library
and torch are imported inside the functions and fixtures that need them.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import paint_spec as ps  # noqa: E402

W = H = 64
STEPS = 32
LAYOUTS = [(1, "planar"), (5, "corner8"), (12, "brick4832"), (14, "cornerh"), (15, "col48")]
LAYOUT_IDS = [n for _, n in LAYOUTS]
UNIFORM_LAYOUTS = [(12, "brick4832"), (14, "cornerh"), (15, "col48")]
VOLUME_BRUSHES = ["interior", "texel", "corner", "outside_centre", "straddle", "whole", "max", "miss"]
FULL = (255, 255, 255, 255)

_oracle_frames = {}


def oracle_frame(oracle, vol, angles=(0.0, 0.0), density=1.0, gsd=None):
    """The oracle's frame and executed steps for `vol`, computed once per session and (volume, camera, density);
    `gsd` replaces the reference camera's global shader data."""
    import volumetricrenderer_amd as vr
    from volumetricrenderer_amd._lib import FMT_RGBA32F
    osd, g = vr.reference_shader_data(1.0, *angles)
    if gsd is not None:
        g = gsd
    obj, glob = vr.shader_data_arrays(osd, g)
    key = (hash(vol.tobytes()), vol.shape, angles, density, None if gsd is None else glob.tobytes())
    if key not in _oracle_frames:
        _oracle_frames[key] = oracle.render(vol, obj, glob, oracle.march(STEPS, density=density), W, H, FMT_RGBA32F)
    return _oracle_frames[key]


@pytest.fixture(scope="module")
def base():
    return ps.base_volume()


@pytest.fixture(scope="module")
def r():
    import volumetricrenderer_amd as vr
    with vr.Renderer(0) as rr:
        yield rr
        rr.set_layout_preference(0)


@pytest.fixture(scope="module")
def fresh():
    import volumetricrenderer_amd as vr
    with vr.Renderer(0) as rr:
        yield rr


@pytest.fixture(scope="module")
def recipe_volume():
    """(the 32^3 recipe volume, the byte its G channel holds everywhere)."""
    import volumetricrenderer_amd as vr
    with vr.Renderer(0) as rr:
        rr.generate_volume(vr.volume_recipe_defaults(size=32))
        vol = rr.get_volume()
    g = int(vol[0, 0, 0, 1])
    assert (vol[..., 1] == g).all(), "the recipe's G is not uniform"
    assert all(len(np.unique(vol[..., c])) > 1 for c in (0, 2, 3))
    return vol, g


def setup(rr, pref, vol, angles=(0.0, 0.0), density=1.0):
    import volumetricrenderer_amd as vr
    rr.set_option("uniform_skip", 1)
    rr.set_layout_preference(pref)
    rr.set_volume(vol)
    rr.set_shader_data(*vr.reference_shader_data(1.0, *angles))
    rr.set_march(vr.march_defaults(max_steps=STEPS, density=density))


def frame(rr, stream=None):
    import torch
    from volumetricrenderer_amd._lib import FMT_RGBA32F
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    img = rr.render(W, H, FMT_RGBA32F, step_counter=cnt, stream=stream)
    torch.cuda.synchronize()
    return img.cpu().numpy(), int(cnt.item())


def assert_marches(rr, name):
    """The intended layout really marches: a silent planar fallback must not pass."""
    assert rr.kernel_variant.startswith(f"grid_{name}_clamp"), rr.kernel_variant


def assert_exact(got, want):
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} mismatches, first {bad[:5].tolist()}"


def check_frame(rr, oracle, vol, angles=(0.0, 0.0), density=1.0):
    """The context's frame is the oracle's for `vol`, with equal step counts, and its volume is `vol`;
    returns (frame, steps)."""
    img, steps = frame(rr)
    ref, ref_steps = oracle_frame(oracle, vol, angles, density)
    assert_exact(img, ref)
    assert steps == ref_steps
    assert_exact(rr.get_volume(), vol)
    return img, steps


def check_fresh_install(fresh, pref, lname, vol, img, steps, angles=(0.0, 0.0), density=1.0):
    """A fresh context with `vol` installed marches the intended layout and renders `img` in `steps` steps."""
    setup(fresh, pref, vol, angles, density)
    assert_marches(fresh, lname)
    img2, steps2 = frame(fresh)
    assert_exact(img, img2)
    assert steps == steps2


def check_needs_a_volume(r, *calls):
    """Each of `calls`, given a context, is refused with VR_ERR_NO_VOLUME (3) on an empty one, which stays
    without a scratch, and on `r` while its medium is procedural (which reads no volume)."""
    import volumetricrenderer_amd as vr
    with vr.Renderer(0) as empty:
        for call in calls:
            with pytest.raises(vr.VRError) as e:
                call(empty)
            assert e.value.status == 3
        assert empty.get_option("blur_scratch_kib") == 0
    r.set_procedural()
    try:
        for call in calls:
            with pytest.raises(vr.VRError) as e:
                call(r)
            assert e.value.status == 3
    finally:
        r.set_procedural(vr.procedural_defaults(enabled=0))
