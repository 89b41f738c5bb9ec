"""The QUAD instance of the four-frame launch (option "frame_quad", DESIGN.md
sec. 5.1.13): four frames of one camera share a ray per pixel, the frames in the
lanes of a quad.  Every check is exact: each target of vr_render_group equals
the plain vr_render of its frame byte for byte.  Which kernel ran is read from
the counters "quad_launches" (QUAD launches) and "group_launches" (four-frame
launches of either instance).

The volume is the 40^3 recipe volume (vr.scaled_recipe), 16 steps, COL48 and
BRICK4832 once.  Targets are pre-filled with the sentinel 0xA5, so a pixel
nobody wrote shows up.

The step counter: the QUAD instance counts no steps (the per-lane sum costs it a
wave per SIMD), so a group launch with a counter takes the other instance.  The
public call takes one counter for its four targets (vr_render_group: the targets
agree in everything but pixels), so it receives the four frames' counts: four
times the plain render's.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import volumetricrenderer_amd as vr
from volumetricrenderer_amd._lib import FMT_RGBA8_UNORM  # noqa: E402

N, STEPS = 40, 16
COL48, BRICK4832 = 15, 12
FMT = FMT_RGBA8_UNORM
SIZES = [(64, 48), (70, 37)]   # whole tiles; quadrants that fall off the right and bottom edges


@pytest.fixture(scope="module")
def r():
    with vr.Renderer(0) as rr:
        rr.generate_volume(vr.scaled_recipe(N))
        yield rr


def setup(rr, pref=COL48, march=None, uniform_skip=1):
    rr.set_procedural(enabled=0)
    for k, v in (("uniform_skip", uniform_skip), ("count", 0), ("split", 1), ("slab", 0), ("empty_fill", 1),
                 ("region_gpu", 1), ("region_interval", 32), ("pair_deal", 0), ("frame_quad", 1)):
        rr.set_option(k, v)
    rr.set_layout_preference(pref)
    rr.set_march(march if march is not None else vr.march_defaults(max_steps=STEPS))


def cam(size, phi=20.0, theta=-35.0):
    return vr.reference_shader_data(size[0] / size[1], phi, theta, 0.0)


def target(rr, size, **band):
    out = rr.alloc_target(*size, FMT, **band)
    out.view(torch.uint8).fill_(0xA5)
    return out


def plain(rr, c, size, counter=None, **band):
    rr.set_shader_data(*c)
    out = rr.render(*size, FMT, out=target(rr, size, **band), step_counter=counter, **band)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def group(rr, cams, size, counter=None, **band):
    """(the four targets, QUAD launches, four-frame launches) of one vr_render_group."""
    outs = [target(rr, size, **band) for _ in range(4)]
    q0, g0 = rr.get_option("quad_launches"), rr.get_option("group_launches")
    rr.render_group(*size, FMT, outs, cameras=cams, step_counter=counter, **band)
    torch.cuda.synchronize()
    return ([o.cpu().numpy() for o in outs], rr.get_option("quad_launches") - q0,
            rr.get_option("group_launches") - g0)


def check_quad(rr, size, c=None, quads=1, **band):
    """Four frames of camera c (None: the current shader data and four equal cameras, both)."""
    c0 = c if c is not None else cam(size)
    want = plain(rr, c0, size, **band)
    for cams in ([None, [c0] * 4] if c is None else [[c0] * 4]):
        got, dq, dg = group(rr, cams, size, **band)
        for i in range(4):
            assert np.array_equal(got[i], want), f"frame {i}"
        assert (dq, dg) == (quads, 1)
    return want


@pytest.mark.parametrize("size", SIZES, ids=["64x48", "70x37"])
@pytest.mark.parametrize("pref", [COL48, BRICK4832], ids=["col48", "brick4832"])
def test_quad_equals_plain_render(r, pref, size):
    setup(r, pref)
    r.set_shader_data(*cam(size))
    assert ("col48" if pref == COL48 else "brick4832") in r.kernel_variant
    want = check_quad(r, size)
    assert not (want.view(np.uint32) == 0xA5A5A5A5).any()   # the plain render wrote every pixel


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("size", SIZES, ids=["64x48", "70x37"])
def test_quad_band_target(r, size, flip):
    setup(r)
    check_quad(r, size, band_rows=16, band_stride=2, band_first=0, band_flip=flip)
    check_quad(r, size, band_rows=16, band_stride=2, band_first=1, band_flip=-flip)


@pytest.mark.parametrize("early", [0.0, 0.05], ids=["no_early_out", "early_out"])
@pytest.mark.parametrize("size", SIZES, ids=["64x48", "70x37"])
def test_quad_early_out(r, size, early):
    setup(r, march=vr.march_defaults(max_steps=STEPS, early_out=early))
    check_quad(r, size)


@pytest.mark.parametrize("size", [(128, 96), (134, 96)], ids=["128x96", "134x96"])
def test_quad_uncovered_tiles_are_filled(r, size):
    """A small box: most tiles of the lists are empty and filled (empty_fill 1), in all four targets.
    The height is a multiple of 8: a tile whose rows span two bands is never empty (tile_is_empty)."""
    setup(r, march=vr.march_defaults(max_steps=STEPS, box_min=(-0.25, -0.25, -0.25), box_max=(0.25, 0.25, 0.25)))
    want = check_quad(r, size)
    assert r.get_option("region_empty_tiles") > 0
    assert not (want.view(np.uint32) == 0xA5A5A5A5).any()


def test_one_ulp_camera_takes_the_old_kernel(r):
    """The third camera one ulp off in one view-matrix component: not one camera, so no QUAD launch."""
    size = SIZES[1]
    setup(r)
    cams = [cam(size) for _ in range(4)]
    cams[2][0].view[0] = float(np.nextafter(np.float32(cams[2][0].view[0]), np.float32(np.inf)))
    want = [plain(r, c, size) for c in cams]
    got, dq, dg = group(r, cams, size)
    assert (dq, dg) == (0, 1)
    for i in range(4):
        assert np.array_equal(got[i], want[i]), f"frame {i}"


def test_frame_quad_off(r):
    size = SIZES[1]
    setup(r)
    r.set_option("frame_quad", 0)
    try:
        assert r.get_option("frame_quad") == 0
        check_quad(r, size, quads=0)
    finally:
        r.set_option("frame_quad", 1)
    assert r.get_option("frame_quad") == 1


def test_step_counter(r):
    """Each of the four frames adds the plain render's count; the counted launch is not a QUAD one."""
    size = SIZES[1]
    setup(r)
    c = cam(size)
    one = torch.zeros(1, dtype=torch.int64, device="cuda")
    want = plain(r, c, size, counter=one)
    steps = int(one.item())
    assert steps > 0
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    got, dq, dg = group(r, [c] * 4, size, counter=cnt)
    assert (dq, dg) == (0, 1)
    assert int(cnt.item()) == 4 * steps
    for i in range(4):
        assert np.array_equal(got[i], want), f"frame {i}"


def scrolled(size, k=0):
    c = cam(size)
    c[1].media_scroll[1 * 4 + 1] = 0.01 + 0.002 * k
    c[1].media_scroll[2 * 4 + 2] = -0.02 + 0.003 * k
    return c


@pytest.mark.parametrize("size", SIZES, ids=["64x48", "70x37"])
def test_quad_equal_tap_offsets(r, size):
    """Non-zero tap offsets, the same in the four frames: the ZO = false instance."""
    setup(r)
    c = scrolled(size)
    r.set_shader_data(*c)
    assert "_clamp" in r.kernel_variant
    check_quad(r, size, c=c)


def test_tap_offsets_of_one_frame_differ(r):
    size = SIZES[1]
    setup(r)
    cams = [scrolled(size), scrolled(size), scrolled(size, 1), scrolled(size)]
    want = [plain(r, c, size) for c in cams]
    got, dq, dg = group(r, cams, size)
    assert (dq, dg) == (0, 1)
    for i in range(4):
        assert np.array_equal(got[i], want[i]), f"frame {i}"


@pytest.mark.parametrize("uniform", [1, 0], ids=["u_instance", "general_instance"])
def test_quad_uniform_and_general_instances(r, uniform):
    """A random 40^3 volume with one channel uniform (the _u instance skips its loads) and without.
    The general kernel has no QUAD instance for zero offsets without early-out (it would lose a
    wave per SIMD, vr_internal.h quad_instance): those frames take the four-frame kernel.  With
    early-out the general kernel's QUAD instance runs, whatever the volume."""
    size = SIZES[1]
    vol = np.random.default_rng(20261020).integers(0, 256, size=(N, N, N, 4), dtype=np.uint8)
    if uniform:
        vol[..., 1] = 77
    setup(r)
    try:
        r.set_volume(vol)
        r.set_shader_data(*cam(size))
        assert ("_u" in r.kernel_variant) == bool(uniform)
        check_quad(r, size, quads=uniform)
        r.set_march(vr.march_defaults(max_steps=STEPS, early_out=0.05))
        check_quad(r, size)
    finally:
        r.generate_volume(vr.scaled_recipe(N))
