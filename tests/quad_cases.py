"""What the GPU tests of the four-frame QUAD launches share (test_gpu_quad_split.py, test_gpu_quad_steps.py,
test_gpu_quad_pairs.py, test_gpu_edit_chain.py, test_gpu_extents.py): the layout ids, the options a test starts
from, the cameras, sentinel-filled targets, the plain render and the group launch with its counter deltas, and
predict(), the Python restatement of which mode a launch takes (vr_internal.h quad_kernel_mode and
quad_requested).  A plain helper module: no tests, no fixtures, no pytest settings.
"""
import numpy as np
import pytest
import torch

if torch.cuda.is_available():
    import volumetricrenderer_amd as vr
from volumetricrenderer_amd._lib import FMT_RGBA8_UNORM  # noqa: E402

PLANAR, CORNER8, BRICK4832, CORNERH, COL48 = 1, 5, 12, 14, 15
FRAME_LAYOUTS = (COL48, BRICK4832, CORNERH)     # vr_internal.h FrameLayouts: the layouts with multi-frame kernels
SPLIT_LAYOUTS = (COL48, BRICK4832)              # quad_split_layout; also the is_b4_family members built by default
FMT = FMT_RGBA8_UNORM
SENTINEL = 0xA5

# the three 0/1 options above frame_quad, their read-only counters below, and the mode a group launch ran in,
# read from which counters it moved
OPTIONS = ("quad_split", "quad_steps", "quad_pairs")
COUNTERS = ("quad_launches", "quad_split_launches", "quad_steps_launches", "quad_pairs_launches")
# (quad_split, quad_steps, quad_pairs): quad_pairs 1, then quad_pairs 0, then quad_steps 0, then quad_split 0
LADDER = [(1, 1, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)]
MODES = {(1, 1, 1, 1): "QUAD_PAIRS", (1, 1, 1, 0): "QUAD_STEPS", (1, 1, 0, 0): "QUAD_SPLIT", (1, 0, 0, 0): "QUAD_FRAMES",
         (0, 0, 0, 0): "QUAD_NONE"}
QUAD_MODES = ("QUAD_PAIRS", "QUAD_STEPS", "QUAD_SPLIT", "QUAD_FRAMES")

# the set-up of the three option files: a 40^3 volume (several bricks of both layouts on every axis), 64x48 and
# 70x37 so that quads fall off the right and the bottom edge
N, STEPS = 40, 16
LAYOUTS = pytest.mark.parametrize("pref", [COL48, BRICK4832], ids=["col48", "brick4832"])
SIZES = [(64, 48), (70, 37)]
SIZE_IDS = ["64x48", "70x37"]
SCALES = pytest.mark.parametrize("scale", [4.0, 1.0], ids=["scale4", "scale1"])


def random_volume_bytes():
    return np.random.default_rng(20261021).integers(0, 256, size=(N, N, N, 4), dtype=np.uint8)


def predict(layout, early, mask, split, steps, pairs):
    """(QUAD, split, step-round, paired) launches of one vr_render_group of four frames of one camera with zero tap
    offsets and no step counter, for the layout that marches: vr_internal.h pair_layout, quad_instance,
    quad_requested and quad_kernel_mode as vr_render.cpp render_frames applies them, restated.  A layout without a
    multi-frame kernel renders its group as four plain frames."""
    if layout not in FRAME_LAYOUTS:
        return 0, 0, 0, 0
    b4 = layout in SPLIT_LAYOUTS                                     # is_b4_family, of the layouts used here
    u_kernel = not early and mask in (1, 2, 4, 8)                    # u_kernel_channel(...) >= 0
    quad = u_kernel or not (b4 and not early)                        # quad_instance
    split = quad and bool(split) and layout in SPLIT_LAYOUTS         # quad_split_layout
    steps = split and bool(steps)
    pairs = steps and bool(pairs)
    return int(quad), int(split), int(steps), int(pairs)


def set_options(rr, pref):
    """The options every QUAD test starts from (all three QUAD options on), and the layout."""
    rr.set_procedural(enabled=0)
    for k, v in (("uniform_skip", 1), ("count", 0), ("split", 1), ("slab", 0), ("empty_fill", 1), ("region_gpu", 1),
                 ("region_interval", 32), ("pair_deal", 0), ("frame_quad", 1), ("quad_split", 1), ("quad_steps", 1),
                 ("quad_pairs", 1)):
        rr.set_option(k, v)
    rr.set_layout_preference(pref)


def setup(rr, pref=COL48, **march):
    set_options(rr, pref)
    rr.set_march(vr.march_defaults(**{"max_steps": STEPS, **march}))


def cam(size, phi=20.0, theta=-35.0):
    return vr.reference_shader_data(size[0] / size[1], phi, theta, 0.0)


def scrolled(size):
    c = cam(size)
    c[1].media_scroll[1 * 4 + 1] = 0.01
    c[1].media_scroll[2 * 4 + 2] = -0.02
    return c


def target(rr, size, fmt=FMT, **band):
    out = rr.alloc_target(*size, fmt, **band)
    out.view(torch.uint8).fill_(SENTINEL)
    return out


def refill(outs):
    for o in outs:
        o.view(torch.uint8).fill_(SENTINEL)


def plain(rr, c, size, **band):
    rr.set_shader_data(*c)
    out = rr.render(*size, FMT, out=target(rr, size, **band), **band)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def counters(rr):
    return tuple(rr.get_option(k) for k in COUNTERS)


def group(rr, c, size, **band):
    """(the four targets, (QUAD, split, step-round, paired) launches) of one vr_render_group of camera c."""
    outs = [target(rr, size, **band) for _ in range(4)]
    before = counters(rr)
    rr.render_group(*size, FMT, outs, cameras=[c] * 4, **band)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs], tuple(a - b for a, b in zip(counters(rr), before))


def check_option(rr, option, size, c=None, **band):
    """The launch with every QUAD option on, then the same launch with `option` = 0, each against the plain render:
    the counters say that the mode is the options', and each of the four targets equals the plain frame byte for
    byte.  Returns the plain frame."""
    c = c if c is not None else cam(size)
    want = plain(rr, c, size, **band)
    for on in (1, 0):
        rr.set_option(option, on)
        try:
            assert rr.get_option(option) == on
            got, counts = group(rr, c, size, **band)
        finally:
            rr.set_option(option, 1)
        # a QUAD launch, in the mode below `option` when it is off: each option counts only under the one before it
        split, steps, pairs = (0 if k == option and not on else 1 for k in OPTIONS)
        assert counts == (1, split, split & steps, split & steps & pairs), \
            f"{option} {on}: (QUAD, split, step-round, paired) launches {counts}"
        for i in range(4):
            bad = np.argwhere(got[i] != want)
            assert bad.size == 0, f"{option} {on}, frame {i}: differs at (y, x, c) {bad[:4].tolist()}"
    return want
