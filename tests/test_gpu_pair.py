"""vr_render_pair (two queued frames in one launch) on the GPU.  Every check is
exact: the bytes of both targets and the step counter equal those of
`set_shader_data(0); render(t0); set_shader_data(1); render(t1)`, and one case
is also compared against the CPU oracle.

The frame is 200 x 120 (edge tiles in both axes: neither side a multiple of
the 8 x 8 wave tile) with 32 steps.  Targets are pre-filled with the sentinel
0xA5, so a tile nobody wrote shows up.  A small volume auto-selects CORNERH;
COL48 and BRICK4832 are forced with set_layout_preference.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import volumetricrenderer_amd as vr
from volumetricrenderer_amd import _lib  # noqa: E402
from volumetricrenderer_amd._lib import FMT_RGBA8_UNORM, FMT_RGBA32F, VRError  # noqa: E402

W, H, STEPS = 200, 120, 32
COL48, BRICK4832, AUTO = 15, 12, 0
LAYOUTS = [(COL48, "col48"), (BRICK4832, "brick4832"), (AUTO, "cornerh")]
LAYOUT_IDS = [n for _, n in LAYOUTS]


@pytest.fixture(scope="module")
def vols():
    rng = np.random.default_rng(20261019)
    v64 = rng.integers(0, 256, size=(64, 64, 64, 4), dtype=np.uint8)
    odd = rng.integers(0, 256, size=(42, 46, 50, 4), dtype=np.uint8)   # 50 x 46 x 42 texels
    uni = v64.copy()
    uni[..., 1] = 77   # G uniform: the _u kernels
    return {"v64": v64, "odd": odd, "uni": uni}


@pytest.fixture(scope="module")
def r():
    with vr.Renderer(0) as rr:
        yield rr


def setup(rr, pref, vol, march=None):
    # split 1: one lane per ray (a frame this small would auto-split its rays, which is not paired)
    rr.set_procedural(enabled=0)
    for k, v in (("uniform_skip", 1), ("count", 0), ("split", 1), ("slab", 0), ("empty_fill", 1), ("region_gpu", 1),
                 ("region_interval", 32), ("pair_deal", 0)):
        rr.set_option(k, v)
    rr.set_layout_preference(pref)
    rr.set_volume(vol)
    rr.set_march(march if march is not None else vr.march_defaults(max_steps=STEPS))


def cam(phi=0.0, theta=0.0, t=0.0, size=(W, H)):
    return vr.reference_shader_data(size[0] / size[1], phi, theta, t)


def target(rr, fmt, size=(W, H), **band):
    out = rr.alloc_target(*size, fmt, **band)
    out.view(torch.uint8).fill_(0xA5)
    return out


def plain(rr, cams, fmt, size=(W, H), **band):
    """The two ordinary renders: (frames, counted steps)."""
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    outs = []
    for c in cams:
        rr.set_shader_data(*c)
        outs.append(rr.render(*size, fmt, out=target(rr, fmt, size, **band), step_counter=cnt, **band))
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs], int(cnt.item())


def paired(rr, cams, fmt, size=(W, H), **band):
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    o0, o1 = target(rr, fmt, size, **band), target(rr, fmt, size, **band)
    rr.render_pair(*size, fmt, o0, o1, cameras=cams, step_counter=cnt, **band)
    torch.cuda.synchronize()
    return [o0.cpu().numpy(), o1.cpu().numpy()], int(cnt.item())


def check(rr, cams, fmt=FMT_RGBA8_UNORM, expect_pair=True, size=(W, H), **band):
    want, steps = plain(rr, cams, fmt, size, **band)
    n0 = rr.get_option("pair_launches")
    got, psteps = paired(rr, cams, fmt, size, **band)
    for i in range(2):
        assert np.array_equal(got[i].view(np.uint8), want[i].view(np.uint8)), f"frame {i}"
    assert psteps == steps
    assert rr.get_option("pair_launches") - n0 == (1 if expect_pair else 0)
    return got


CAMERA_ANGLES = {
    "equal": (20.0, 20.0),
    "spin_1.6": (20.0, 21.6),
    "apart_40": (20.0, 60.0),   # frame 1's empty tiles are not the lists'
}
VR_ERR_INVALID = 1


def cameras(name, size=(W, H)):
    return [cam(phi, -35.0, size=size) for phi in CAMERA_ANGLES[name]]


@pytest.mark.parametrize("cams", list(CAMERA_ANGLES))
@pytest.mark.parametrize("vol", ["v64", "odd", "uni"])
@pytest.mark.parametrize("pref,name", LAYOUTS, ids=LAYOUT_IDS)
def test_pair_equals_two_renders(r, vols, pref, name, vol, cams):
    setup(r, pref, vols[vol])
    r.set_shader_data(*cameras(cams)[0])
    assert name in r.kernel_variant and ("_u" in r.kernel_variant) == (vol == "uni")
    check(r, cameras(cams))


SMALL = (24, 16)   # 3 x 2 wave tiles


@pytest.mark.parametrize("fill", [0, 1])
@pytest.mark.parametrize("pref,name", LAYOUTS, ids=LAYOUT_IDS)
def test_pair_frame_of_six_tiles(r, vols, pref, name, fill):
    """24 x 16 pixels: several XCDs' lists are empty, there is one entry wave per XCD (nwx 1), and
    the second entry wave of a pair's workgroup has no entries (w >= nwx), in either deal."""
    setup(r, pref, vols["v64"])
    r.set_option("empty_fill", fill)
    try:
        for deal in (0, 1):
            r.set_option("pair_deal", deal)
            for cams in ("equal", "apart_40"):
                for frame in check(r, cameras(cams, SMALL), size=SMALL):
                    assert not (frame.view(np.uint32) == 0xA5A5A5A5).any(), (deal, cams)   # a pixel nobody wrote
    finally:
        r.set_option("empty_fill", 1)
        r.set_option("pair_deal", 0)


@pytest.mark.parametrize("fmt", [FMT_RGBA8_UNORM, FMT_RGBA32F])
def test_pair_against_oracle(r, oracle, vols, fmt):
    setup(r, COL48, vols["odd"])
    cams = cameras("spin_1.6")
    got = check(r, cams, fmt)
    m = oracle.from_params(vr.march_defaults(max_steps=STEPS))
    for i in range(2):
        obj, glob = vr.shader_data_arrays(*cams[i])
        ref, _ = oracle.render(vols["odd"], obj, glob, m, W, H, fmt)
        assert np.array_equal(got[i].view(np.uint8), ref.view(np.uint8)), i


def test_pair_current_shader_data(r, vols):
    """osd = gsd = NULL: both frames with the context's shader data."""
    setup(r, COL48, vols["v64"])
    c = cam(-30.0, 40.0)
    want, steps = plain(r, [c, c], FMT_RGBA8_UNORM)
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    o0, o1 = target(r, FMT_RGBA8_UNORM), target(r, FMT_RGBA8_UNORM)
    r.render_pair(W, H, FMT_RGBA8_UNORM, o0, o1, step_counter=cnt)
    torch.cuda.synchronize()
    assert np.array_equal(o0.cpu().numpy(), want[0]) and np.array_equal(o1.cpu().numpy(), want[1])
    assert int(cnt.item()) == steps


@pytest.mark.parametrize("pref,name", LAYOUTS, ids=LAYOUT_IDS)
def test_pair_box_partly_off_screen(r, vols, pref, name):
    """A box shifted so that part of it projects outside the frame."""
    m = vr.march_defaults(max_steps=STEPS, box_min=(0.3, -0.5, -0.5), box_max=(2.3, 1.5, 0.5))
    setup(r, pref, vols["odd"], m)
    check(r, cameras("spin_1.6"))


@pytest.mark.parametrize("pref,name", LAYOUTS, ids=LAYOUT_IDS)
def test_pair_media_scroll_offsets(r, vols, pref, name):
    """Non-zero tap_T inside the clamp-exact range (the non-zero-offset kernels), per frame."""
    setup(r, pref, vols["v64"])
    cams = [cam(20.0, -35.0), cam(21.6, -35.0)]
    for k, (_, gsd) in enumerate(cams):   # small per-tap offsets, other ones per frame (clamp stays exact)
        gsd.media_scroll[1 * 4 + 1] = 0.01 + 0.002 * k
        gsd.media_scroll[2 * 4 + 2] = -0.02 + 0.003 * k
    r.set_shader_data(*cams[0])
    assert "_clamp" in r.kernel_variant
    check(r, cams)
    # one frame with offsets and one without select different kernels: two renders, the same bytes
    check(r, [cam(20.0, -35.0), cams[1]], expect_pair=False)


def test_pair_mirrored_repeat_wrap(r, vols):
    """Offsets far outside [0, 1]: the planar mirrored-repeat kernel has no paired instance."""
    setup(r, COL48, vols["v64"])
    cams = [cam(20.0, -35.0), cam(21.6, -35.0)]
    for _, gsd in cams:
        for col, vals in enumerate([(0.0, 3.7, -2.2, 1.3), (0.0, -0.6, 5.1, -7.9), (0.0, 1.9, 0.4, -1.1)]):
            for row, v in enumerate(vals):
                gsd.media_scroll[col * 4 + row] = v
    r.set_shader_data(*cams[0])
    assert r.kernel_variant == "grid_planar_mirror"
    check(r, cams, expect_pair=False)


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("fmt", [FMT_RGBA8_UNORM, FMT_RGBA32F])
def test_pair_band_target(r, vols, fmt, flip):
    setup(r, COL48, vols["odd"])
    for first in (0, 1):
        check(r, cameras("apart_40"), fmt, band_rows=16, band_stride=2, band_first=first,
              band_flip=flip if first == 0 else -flip)


@pytest.mark.parametrize("gpu,interval", [(0, 1), (0, 32), (1, 1), (1, 32)])
def test_pair_region_rebuilds_over_five_pairs(r, vols, gpu, interval):
    """A moving camera: list reuse, host and GPU rebuilds stay consistent with two renders per pair."""
    setup(r, COL48, vols["v64"])
    r.set_option("region_gpu", gpu)
    r.set_option("region_interval", interval)
    try:
        for k in range(5):
            check(r, [cam(3.2 * k, 10.0), cam(3.2 * k + 1.6, 10.0)])
    finally:
        r.set_option("region_gpu", 1)
        r.set_option("region_interval", 32)


@pytest.mark.parametrize("fill", [0, 1])
@pytest.mark.parametrize("deal", [0, 1])
def test_pair_empty_fill_and_deal(r, vols, fill, deal):
    setup(r, COL48, vols["uni"])
    r.set_option("empty_fill", fill)
    r.set_option("pair_deal", deal)
    try:
        for name in CAMERA_ANGLES:
            check(r, cameras(name))
    finally:
        r.set_option("empty_fill", 1)
        r.set_option("pair_deal", 0)


def test_pair_early_out(r, vols):
    setup(r, BRICK4832, vols["v64"], vr.march_defaults(max_steps=STEPS, early_out=0.05))
    check(r, cameras("spin_1.6"))


@pytest.mark.parametrize("what", ["procedural", "slab", "split"])
def test_pair_fallbacks(r, vols, what):
    """No paired kernel: the two ordinary renders, the same bytes."""
    setup(r, COL48, vols["v64"])
    try:
        if what == "procedural":
            r.set_procedural(shadow_steps=0)
        elif what == "slab":
            r.set_option("slab", 1)
        else:
            r.set_option("split", 2)
        check(r, cameras("spin_1.6"), expect_pair=False)
    finally:
        r.set_procedural(enabled=0)
        r.set_option("slab", 0)
        r.set_option("split", 1)


def test_pair_targets_must_agree(r, vols):
    setup(r, COL48, vols["v64"])
    r.set_shader_data(*cameras("equal")[0])
    o0, o1 = target(r, FMT_RGBA8_UNORM), target(r, FMT_RGBA8_UNORM)

    def tgt(out, **kw):
        f = dict(width=W, height=H, format=FMT_RGBA8_UNORM, band_rows=0, band_stride=1, band_first=0,
                 pixels=out.data_ptr(), row_pitch=W * 4, step_counter=None)
        f.update(kw)
        return _lib.Target(**f)

    for kw in (dict(width=W - 8), dict(height=H - 8), dict(format=FMT_RGBA32F), dict(band_rows=16, band_stride=2),
               dict(row_pitch=W * 4 + 16), dict(pixels=None)):
        with pytest.raises(VRError) as e:
            _lib.call("vr_render_pair", r._ctx, ctypes.byref(tgt(o0)), ctypes.byref(tgt(o1, **kw)), None, None, None)
        assert e.value.status == VR_ERR_INVALID, kw
    torch.cuda.synchronize()
    for o in (o0, o1):
        assert bool((o.view(torch.uint8) == 0xA5).all())


# ---- the paths between a vr_target and the pair's launch: launch cache, a failing second frame, inject_throw ----

def test_pair_frame0_from_launch_cache(r, vols):
    """Frame 0 is the cached launch of a plain render on the same stream, target and counter."""
    setup(r, AUTO, vols["v64"])
    fmt = FMT_RGBA8_UNORM
    r.set_shader_data(*cam(20.0, -35.0))
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    o0, o1 = target(r, fmt), target(r, fmt)

    def plain_o0():
        cnt.zero_()
        o0.view(torch.uint8).fill_(0xA5)
        r.render(W, H, fmt, out=o0, step_counter=cnt)
        torch.cuda.synchronize()
        return o0.cpu().numpy(), int(cnt.item())

    plain_o0()   # (a region-list build of this render has completed before the next one is planned and cached)
    want, steps = plain_o0()
    hits, pairs = r.get_option("launch_cache_hits"), r.get_option("pair_launches")
    cnt.zero_()
    o0.view(torch.uint8).fill_(0xA5)
    r.render_pair(W, H, fmt, o0, o1, cameras=None, step_counter=cnt)
    torch.cuda.synchronize()
    assert r.get_option("launch_cache_hits") - hits == 1
    assert r.get_option("pair_launches") - pairs == 1
    assert np.array_equal(o0.cpu().numpy(), want) and np.array_equal(o1.cpu().numpy(), want)
    assert int(cnt.item()) == 2 * steps
    again, steps_again = plain_o0()
    assert r.get_option("launch_cache_hits") - hits == 2
    assert np.array_equal(again, want) and steps_again == steps


def test_pair_second_frame_fails_first_renders(r, vols):
    """A singular second camera: VR_ERR_INVALID, frame 0 rendered, frame 1's target untouched."""
    setup(r, AUTO, vols["v64"])
    fmt = FMT_RGBA8_UNORM
    a = cam(20.0, -35.0)
    singular = cam(21.6, -35.0)
    for k in range(16):
        singular[0].projection[k] = 0.0
    want, _ = plain(r, [a], fmt)
    pairs = r.get_option("pair_launches")
    o0, o1 = target(r, fmt), target(r, fmt)
    with pytest.raises(VRError) as e:
        r.render_pair(W, H, fmt, o0, o1, cameras=[a, singular])
    assert e.value.status == VR_ERR_INVALID
    torch.cuda.synchronize()
    assert np.array_equal(o0.cpu().numpy(), want[0])
    assert bool((o1.view(torch.uint8) == 0xA5).all())
    assert r.get_option("pair_launches") == pairs
    check(r, cameras("spin_1.6"))


@pytest.mark.parametrize("kind,status", [(1, 2), (2, 5)], ids=["runtime_error", "bad_alloc"])
def test_pair_inject_throw(r, vols, kind, status):
    """The option fires in frame 0's host path: vr_render's status and message, consumed once."""
    setup(r, AUTO, vols["v64"])
    fmt = FMT_RGBA8_UNORM
    cams = cameras("spin_1.6")
    r.set_option("inject_throw", kind)
    o0, o1 = target(r, fmt), target(r, fmt)
    with pytest.raises(VRError) as e:
        r.render_pair(W, H, fmt, o0, o1, cameras=cams)
    assert e.value.status == status
    assert "vr_render: " in str(e.value)
    torch.cuda.synchronize()
    for o in (o0, o1):   # nothing was launched
        assert bool((o.view(torch.uint8) == 0xA5).all())
    check(r, cams)   # the option is write-only: that it was consumed shows in the same call passing now


def test_pair_unpaired_first_frame_cached_once(r, vols):
    """split 2 (no paired kernel): the second call launches both frames from the cache, one entry each."""
    setup(r, AUTO, vols["v64"])
    fmt = FMT_RGBA8_UNORM
    c = cam(20.0, -35.0)
    try:
        r.set_option("split", 2)
        want, steps = plain(r, [c, c], fmt)
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        o0, o1 = target(r, fmt), target(r, fmt)
        deltas = []
        for _ in range(2):
            cnt.zero_()
            o0.view(torch.uint8).fill_(0xA5)
            o1.view(torch.uint8).fill_(0xA5)
            hits, pairs = r.get_option("launch_cache_hits"), r.get_option("pair_launches")
            r.render_pair(W, H, fmt, o0, o1, cameras=None, step_counter=cnt)
            torch.cuda.synchronize()
            deltas.append(r.get_option("launch_cache_hits") - hits)
            assert r.get_option("pair_launches") == pairs
            assert np.array_equal(o0.cpu().numpy(), want[0]) and np.array_equal(o1.cpu().numpy(), want[1])
            assert int(cnt.item()) == steps
        print("launch_cache_hits per call:", deltas)
        assert deltas[1] == 2   # (the first call's depends on which addresses the allocator hands out again)
    finally:
        r.set_option("split", 1)
