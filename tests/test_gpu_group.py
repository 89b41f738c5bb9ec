"""vr_render_group (up to four queued frames, four of them in one launch) on the
GPU.  Every check is exact: the bytes of every target and the step counter
equal those of `set_shader_data(i); render(t_i)` for each frame in order, and
one case is also compared against the CPU oracle.

The frame is 70 x 44 (neither side a multiple of the 8 x 8 wave tile) with 32
steps; the volumes (40 x 24 x 70 and 64^3 texels) span several bricks of every
layout in every axis.  Targets are pre-filled with the sentinel 0xA5, so a tile
nobody wrote shows up.  A small volume auto-selects CORNERH; COL48 and
BRICK4832 are forced with set_layout_preference.  Which launches ran is read
from the counters "group_launches" (four-frame launches) and "pair_launches" (frame
pairs that shared a launch: one per paired launch, two per four-frame launch).
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

W, H, STEPS = 70, 44, 32
COL48, BRICK4832, AUTO = 15, 12, 0
LAYOUTS = [(COL48, "col48"), (BRICK4832, "brick4832"), (AUTO, "cornerh")]
LAYOUT_IDS = [n for _, n in LAYOUTS]
VR_ERR_INVALID = 1


@pytest.fixture(scope="module")
def vols():
    rng = np.random.default_rng(20261020)
    v64 = rng.integers(0, 256, size=(64, 64, 64, 4), dtype=np.uint8)
    odd = rng.integers(0, 256, size=(70, 24, 40, 4), dtype=np.uint8)   # 40 x 24 x 70 texels
    uni = v64.copy()
    uni[..., 1] = 77   # G uniform: the _u kernels
    return {"v64": v64, "odd": odd, "uni": uni}


@pytest.fixture(scope="module")
def r():
    with vr.Renderer(0) as rr:
        yield rr


def setup(rr, pref, vol, march=None):
    # split 1: one lane per ray (a frame this small would auto-split its rays, which is neither paired nor grouped)
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
    """The ordinary renders: (frames, counted steps)."""
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    outs = []
    for c in cams:
        rr.set_shader_data(*c)
        outs.append(rr.render(*size, fmt, out=target(rr, fmt, size, **band), step_counter=cnt, **band))
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs], int(cnt.item())


def grouped(rr, cams, fmt, size=(W, H), **band):
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    outs = [target(rr, fmt, size, **band) for _ in cams]
    rr.render_group(*size, fmt, outs, cameras=cams, step_counter=cnt, **band)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs], int(cnt.item())


def check(rr, cams, fmt=FMT_RGBA8_UNORM, groups=None, pairs=None, size=(W, H), **band):
    """The group of len(cams) frames against the plain renders; `groups` / `pairs`: the four-frame
    and two-frame launches expected (default: what vr_group_split names for len(cams))."""
    n = len(cams)
    if groups is None:
        groups = 1 if n == 4 else 0
    if pairs is None:
        pairs = 1 if n in (2, 3) else 0
    want, steps = plain(rr, cams, fmt, size, **band)
    g0, p0 = rr.get_option("group_launches"), rr.get_option("pair_launches")
    got, gsteps = grouped(rr, cams, fmt, size, **band)
    for i in range(n):
        assert np.array_equal(got[i].view(np.uint8), want[i].view(np.uint8)), f"frame {i}"
    assert gsteps == steps
    assert rr.get_option("group_launches") - g0 == groups
    assert rr.get_option("pair_launches") - p0 == pairs + 2 * groups
    return got


CAMERA_ANGLES = {
    "equal": (20.0, 20.0, 20.0, 20.0),
    "spin_1.6": (20.0, 21.6, 23.2, 24.8),
    "apart_40": (20.0, 60.0, 100.0, 21.6),   # frames whose empty tiles are not the lists'
}


def cameras(name, n=4, size=(W, H)):
    return [cam(phi, -35.0, size=size) for phi in CAMERA_ANGLES[name][:n]]


@pytest.mark.parametrize("cams", list(CAMERA_ANGLES))
@pytest.mark.parametrize("vol", ["v64", "odd", "uni"])
@pytest.mark.parametrize("pref,name", LAYOUTS, ids=LAYOUT_IDS)
def test_group_equals_four_renders(r, vols, pref, name, vol, cams):
    setup(r, pref, vols[vol])
    r.set_shader_data(*cameras(cams)[0])
    assert name in r.kernel_variant and ("_u" in r.kernel_variant) == (vol == "uni")
    check(r, cameras(cams))


SMALL = (24, 16)   # 3 x 2 wave tiles


@pytest.mark.parametrize("fill", [0, 1])
@pytest.mark.parametrize("pref,name", LAYOUTS, ids=LAYOUT_IDS)
def test_group_frame_of_six_tiles(r, vols, pref, name, fill):
    """24 x 16 pixels: several XCDs' lists are empty and there is one workgroup per XCD (nwx 1)."""
    setup(r, pref, vols["v64"])
    r.set_option("empty_fill", fill)
    try:
        for cams in ("equal", "apart_40"):
            for frame in check(r, cameras(cams, size=SMALL), size=SMALL):
                assert not (frame.view(np.uint32) == 0xA5A5A5A5).any(), cams   # a pixel nobody wrote
    finally:
        r.set_option("empty_fill", 1)


@pytest.mark.parametrize("n", [3, 2, 1])
@pytest.mark.parametrize("pref,name", LAYOUTS, ids=LAYOUT_IDS)
def test_fewer_frames_take_the_pair_and_plain_paths(r, vols, pref, name, n):
    """3 = a pair and a plain render, 2 = a pair, 1 = a plain render; never a group launch."""
    setup(r, pref, vols["odd"])
    check(r, cameras("spin_1.6", n))


def test_group_against_oracle(r, oracle, vols):
    setup(r, COL48, vols["odd"])
    cams = cameras("spin_1.6")
    got = check(r, cams, FMT_RGBA8_UNORM)
    m = oracle.from_params(vr.march_defaults(max_steps=STEPS))
    for i in range(4):
        obj, glob = vr.shader_data_arrays(*cams[i])
        ref, _ = oracle.render(vols["odd"], obj, glob, m, W, H, FMT_RGBA8_UNORM)
        assert np.array_equal(got[i].view(np.uint8), ref.view(np.uint8)), i


def test_group_current_shader_data(r, vols):
    """osd = gsd = NULL: every frame with the context's shader data."""
    setup(r, COL48, vols["v64"])
    c = cam(-30.0, 40.0)
    want, steps = plain(r, [c] * 4, FMT_RGBA8_UNORM)
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    outs = [target(r, FMT_RGBA8_UNORM) for _ in range(4)]
    g0 = r.get_option("group_launches")
    r.render_group(W, H, FMT_RGBA8_UNORM, outs, step_counter=cnt)
    torch.cuda.synchronize()
    for o, w in zip(outs, want):
        assert np.array_equal(o.cpu().numpy(), w)
    assert int(cnt.item()) == steps
    assert r.get_option("group_launches") - g0 == 1


@pytest.mark.parametrize("pref,name", LAYOUTS, ids=LAYOUT_IDS)
def test_group_box_partly_off_screen(r, vols, pref, name):
    """A box shifted so that part of it projects outside the frame."""
    m = vr.march_defaults(max_steps=STEPS, box_min=(0.3, -0.5, -0.5), box_max=(2.3, 1.5, 0.5))
    setup(r, pref, vols["odd"], m)
    check(r, cameras("spin_1.6"))


def scrolled(base=0.0):
    """Cameras with small per-tap MediaScroll offsets, other ones per frame (clamp stays exact)."""
    cams = cameras("spin_1.6")
    for k, (_, gsd) in enumerate(cams):
        gsd.media_scroll[1 * 4 + 1] = 0.01 + 0.002 * k
        gsd.media_scroll[2 * 4 + 2] = -0.02 + 0.003 * k
    return cams


@pytest.mark.parametrize("pref,name", LAYOUTS, ids=LAYOUT_IDS)
def test_group_media_scroll_offsets(r, vols, pref, name):
    """Non-zero tap_T inside the clamp-exact range (the non-zero-offset kernels), per frame."""
    setup(r, pref, vols["v64"])
    cams = scrolled()
    r.set_shader_data(*cams[0])
    assert "_clamp" in r.kernel_variant
    check(r, cams)


def test_group_mixed_offsets_fall_back(r, vols):
    """One frame without offsets among three with: the frames select different kernels -- four ordinary renders."""
    setup(r, COL48, vols["v64"])
    cams = scrolled()
    cams[2] = cam(23.2, -35.0)
    check(r, cams, groups=0, pairs=0)


def test_group_mirrored_repeat_wrap(r, vols):
    """Offsets far outside [0, 1]: the planar mirrored-repeat kernel has no grouped instance."""
    setup(r, COL48, vols["v64"])
    cams = cameras("spin_1.6")
    for _, gsd in cams:
        for col, vals in enumerate([(0.0, 3.7, -2.2, 1.3), (0.0, -0.6, 5.1, -7.9), (0.0, 1.9, 0.4, -1.1)]):
            for row, v in enumerate(vals):
                gsd.media_scroll[col * 4 + row] = v
    r.set_shader_data(*cams[0])
    assert r.kernel_variant == "grid_planar_mirror"
    check(r, cams, groups=0, pairs=0)


@pytest.mark.parametrize("flip", [0, 1])
def test_group_band_target(r, vols, flip):
    setup(r, COL48, vols["odd"])
    for first in (0, 1):
        check(r, cameras("apart_40"), FMT_RGBA8_UNORM, band_rows=16, band_stride=2, band_first=first,
              band_flip=flip if first == 0 else -flip)


def test_group_rgba32f(r, vols):
    setup(r, BRICK4832, vols["odd"])
    check(r, cameras("spin_1.6"), FMT_RGBA32F)


@pytest.mark.parametrize("gpu,interval", [(0, 1), (0, 32), (1, 1), (1, 32)])
def test_group_region_rebuilds_over_four_groups(r, vols, gpu, interval):
    """A moving camera: list reuse, host and GPU rebuilds stay consistent with four renders per group."""
    setup(r, COL48, vols["v64"])
    r.set_option("region_gpu", gpu)
    r.set_option("region_interval", interval)
    try:
        for k in range(4):
            check(r, [cam(6.4 * k + 1.6 * j, 10.0) for j in range(4)])
    finally:
        r.set_option("region_gpu", 1)
        r.set_option("region_interval", 32)


@pytest.mark.parametrize("fill", [0, 1])
def test_group_empty_fill(r, vols, fill):
    setup(r, COL48, vols["uni"])
    r.set_option("empty_fill", fill)
    try:
        for name in CAMERA_ANGLES:
            check(r, cameras(name))
    finally:
        r.set_option("empty_fill", 1)


@pytest.mark.parametrize("pref,name", LAYOUTS, ids=LAYOUT_IDS)
def test_group_early_out(r, vols, pref, name):
    setup(r, pref, vols["v64"], vr.march_defaults(max_steps=STEPS, early_out=0.05))
    check(r, cameras("spin_1.6"))


@pytest.mark.parametrize("what", ["procedural", "slab", "split"])
def test_group_fallbacks(r, vols, what):
    """No grouped kernel: the four ordinary renders, the same bytes."""
    setup(r, COL48, vols["v64"])
    try:
        if what == "procedural":
            r.set_procedural(shadow_steps=0)
        elif what == "slab":
            r.set_option("slab", 1)
        else:
            r.set_option("split", 2)
        check(r, cameras("spin_1.6"), groups=0, pairs=0)
    finally:
        r.set_procedural(enabled=0)
        r.set_option("slab", 0)
        r.set_option("split", 1)


@pytest.mark.parametrize("n", [4, 3])
def test_group_targets_must_agree(r, vols, n):
    setup(r, COL48, vols["v64"])
    r.set_shader_data(*cameras("equal")[0])
    outs = [target(r, FMT_RGBA8_UNORM) for _ in range(n)]

    def tgt(out, **kw):
        f = dict(width=W, height=H, format=FMT_RGBA8_UNORM, band_rows=0, band_stride=1, band_first=0,
                 pixels=out.data_ptr(), row_pitch=W * 4, step_counter=None)
        f.update(kw)
        return _lib.Target(**f)

    for kw in (dict(width=W - 8), dict(height=H - 8), dict(format=FMT_RGBA32F), dict(band_rows=16, band_stride=2),
               dict(row_pitch=W * 4 + 16), dict(pixels=None)):
        for bad in range(1, n):
            ts = (_lib.Target * n)(*[tgt(o, **(kw if i == bad else {})) for i, o in enumerate(outs)])
            with pytest.raises(VRError) as e:
                _lib.call("vr_render_group", r._ctx, ts, n, None, None, None)
            assert e.value.status == VR_ERR_INVALID, (kw, bad)
    for bad_n in (0, 5):
        ts = (_lib.Target * 5)(*[tgt(outs[0]) for _ in range(5)])
        with pytest.raises(VRError) as e:
            _lib.call("vr_render_group", r._ctx, ts, bad_n, None, None, None)
        assert e.value.status == VR_ERR_INVALID
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o.view(torch.uint8) == 0xA5).all())


@pytest.mark.parametrize("k", [1, 2, 3])
def test_group_frame_k_fails_earlier_frames_render(r, vols, k):
    """A singular camera k: VR_ERR_INVALID, frames 0..k-1 rendered, the targets from k on untouched."""
    setup(r, AUTO, vols["v64"])
    fmt = FMT_RGBA8_UNORM
    cams = cameras("spin_1.6")
    for j in range(16):
        cams[k][0].projection[j] = 0.0
    want, _ = plain(r, cams[:k], fmt)
    g0 = r.get_option("group_launches")
    outs = [target(r, fmt) for _ in range(4)]
    with pytest.raises(VRError) as e:
        r.render_group(W, H, fmt, outs, cameras=cams)
    assert e.value.status == VR_ERR_INVALID
    torch.cuda.synchronize()
    for i in range(k):
        assert np.array_equal(outs[i].cpu().numpy(), want[i]), i
    for i in range(k, 4):
        assert bool((outs[i].view(torch.uint8) == 0xA5).all()), i
    assert r.get_option("group_launches") == g0
    check(r, cameras("spin_1.6"))   # (and the context is usable afterwards)
