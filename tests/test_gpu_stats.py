"""vr_brush_stats / vr_box_stats on the GPU against the numpy restatement
(tests/stats_spec.py): the spec brushes into a poisoned buffer; boxes with every
channel mask; rows longer and shorter than a wave; more rows than the grid
holds waves; volumes that take and that defeat the kernel's one-atomic path;
stream order against paints; the context left as it was; the eyedropper round
trip; refusals.  Everything is exact.

The volume is brush_harness.py's: 37 x 22 x 45, the reference camera at
64 x 64, 32 steps.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import paint_spec as ps  # noqa: E402
import stats_spec as ss  # noqa: E402
from brush_harness import STEPS, H, W, base, r  # noqa: E402,F401

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import volumetricrenderer_amd as vr
from volumetricrenderer_amd import _lib  # noqa: E402
from volumetricrenderer_amd._lib import FMT_RGBA32F  # noqa: E402

NX, NY, NZ = ps.NX, ps.NY, ps.NZ
BYTES = 8240


def poisoned():
    return torch.full((BYTES,), 0xFF, dtype=torch.uint8, device="cuda")


def brush_stats(rr, centre, radius, falloff, strength, stream=None):
    """Through a buffer pre-filled with 0xFF: the call must overwrite it."""
    buf = poisoned()
    assert rr.brush_stats(centre, radius, falloff, strength, stream=stream, out=buf) is buf
    return vr.unpack_stats(buf)


def box_stats(rr, origin, extent, mask=0xF):
    buf = poisoned()
    assert rr.box_stats(origin, extent, mask, out=buf) is buf
    return vr.unpack_stats(buf)


def whole(vol):
    nz, ny, nx, _ = vol.shape
    return (0, 0, 0), (nx, ny, nz)


# ---- 1. the spec brushes -----------------------------------------------------------------------
@pytest.mark.parametrize("strength", ss.STRENGTHS, ids=["rgb", "a"])
@pytest.mark.parametrize("falloff,fname", ps.FALLOFFS, ids=[n for _, n in ps.FALLOFFS])
@pytest.mark.parametrize("name", list(ps.BRUSHES))
def test_brush_stats_equal_the_specification(r, base, name, falloff, fname, strength):
    r.set_layout_preference(14)
    r.set_volume(base)
    centre, radius = ps.BRUSHES[name]
    want = ss.spec_brush_stats(base, centre, radius, falloff, strength)
    assert (want["count"] == 0) == (name == "miss")
    got = brush_stats(r, centre, radius, falloff, strength)
    ss.assert_stats(got, want, name)
    ss.assert_stats(vr.brush_stats_host(vr.make_brush(centre, radius, 0, falloff, 0, strength), base), want, name)
    ss.assert_stats(r.brush_stats(centre, radius, falloff, strength), want, name)   # the host-returning form


# ---- 2. boxes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", range(16))
def test_box_stats(r, base, mask):
    r.set_layout_preference(0)
    r.set_volume(base)
    for origin, extent in (whole(base), ((5, 3, 7), (1, 19, 38)), ((36, 21, 44), (1, 1, 1))):
        want = ss.spec_box_stats(base, origin, extent, mask)
        ss.assert_stats(box_stats(r, origin, extent, mask), want, (origin, extent))
        ss.assert_stats(vr.box_stats_host(base, origin, extent, mask), want)
    ss.assert_stats(r.box_stats(*whole(base), mask), ss.spec_box_stats(base, *whole(base), mask))


# ---- 3. row lengths ----------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(150, 9, 7), (5, 4, 2), (1, 1, 1)], ids=["150x9x7", "5x4x2", "1x1x1"])
def test_row_lengths(r, dims):
    """Rows of 150 texels make the lanes loop along x three times, the last pass with 22 lanes; 5 and 1 leave most
    of a wave idle."""
    nx, ny, nz = dims
    vol = np.random.default_rng(nx * 1000 + ny).integers(0, 256, size=(nz, ny, nx, 4), dtype=np.uint8)
    r.set_layout_preference(0)
    r.set_volume(vol)
    centre, radius = (nx // 2, ny // 2, nz // 2), (100, 40, 40)
    brushes = [radius] + ([(70, 4, 3)] if nx == 150 else [])   # every row whole; rows cut at both ends, some left out
    for falloff in (0, 1):
        for rad in brushes:
            want = ss.spec_brush_stats(vol, centre, rad, falloff, ss.FULL)
            inside, _ = ps.spec_weights(vol.shape[:3], centre, rad, falloff)
            if rad == radius:
                assert inside.all()
            else:
                per_row = inside.sum(axis=2)
                assert (per_row == 0).any() and (per_row > 128).any() and ((per_row > 0) & (per_row < 64)).any(), per_row
            ss.assert_stats(brush_stats(r, centre, rad, falloff, ss.FULL), want, rad)
    ss.assert_stats(box_stats(r, *whole(vol)), ss.spec_box_stats(vol, *whole(vol), 0xF))


# ---- 4. more rows than the grid holds waves ----------------------------------------------------
def test_grid_stride_loop(r):
    """16 900 rows: more than 1024 workgroups x 4 waves, so the row loop runs more than once under any permitted cap."""
    vol = np.random.default_rng(33130).integers(0, 256, size=(130, 130, 33, 4), dtype=np.uint8)
    assert vol.shape[0] * vol.shape[1] > 1024 * 4
    r.set_layout_preference(0)
    r.set_volume(vol)
    ss.assert_stats(box_stats(r, *whole(vol)), ss.spec_box_stats(vol, *whole(vol), 0xF))
    centre, radius = (16, 65, 65), (20, 70, 70)
    ss.assert_stats(brush_stats(r, centre, radius, 1, (255, 0, 255, 1)), ss.spec_brush_stats(vol, centre, radius, 1, (255, 0, 255, 1)))


# ---- 5. the one-atomic path and the volumes that defeat it -------------------------------------
def test_contention_paths(r):
    with vr.Renderer(0) as rr:
        rr.generate_volume(vr.volume_recipe_defaults(size=32))
        recipe = rr.get_volume()
        g = int(recipe[0, 0, 0, 1])
        assert (recipe[..., 1] == g).all(), "the recipe's G is not uniform"
        for falloff in (0, 1):
            got = brush_stats(rr, (16, 16, 16), (255, 255, 255), falloff, ss.FULL)
            ss.assert_stats(got, ss.spec_brush_stats(recipe, (16, 16, 16), (255, 255, 255), falloff, ss.FULL))
            assert got.count == 32 ** 3 and got.hist[1][g] == 32 ** 3
        ss.assert_stats(box_stats(rr, *whole(recipe)), ss.spec_box_stats(recipe, *whole(recipe), 0xF))
    rng = np.random.default_rng(77)
    ext = rng.integers(0, 256, size=(9, 11, 70, 4), dtype=np.uint8)
    ext[..., 0] = 255   # wsum at its largest
    ext[..., 2] = 0     # and at 0
    alt = np.empty((6, 7, 131, 4), np.uint8)
    zz, yy, xx = np.meshgrid(np.arange(6), np.arange(7), np.arange(131), indexing="ij")
    for c, (a, b) in enumerate(((3, 250), (0, 255), (17, 18), (128, 127))):
        alt[..., c] = np.where((xx + yy + zz) % 2 == 0, a, b)   # both values in every wave's 64 texels
    one_off = np.full((5, 6, 100, 4), 90, np.uint8)
    one_off[2, 3, 64] = (1, 2, 3, 4)                             # one lane differs from its wave's first
    one_off[4, 5, 0] = (5, 6, 7, 8)                              # the first lane differs from all others
    for vol in (ext, alt, one_off):
        r.set_layout_preference(0)
        r.set_volume(vol)
        nz, ny, nx, _ = vol.shape
        centre, radius = (nx // 2, ny // 2, nz // 2), (255, 255, 255)
        for falloff in (0, 1):
            got = brush_stats(r, centre, radius, falloff, ss.FULL)
            ss.assert_stats(got, ss.spec_brush_stats(vol, centre, radius, falloff, ss.FULL))
            assert got.count == nx * ny * nz
        got = box_stats(r, *whole(vol))
        ss.assert_stats(got, ss.spec_box_stats(vol, *whole(vol), 0xF))
        if vol is ext:
            assert got.wsum[0] == 255 * 256 * got.count and got.wsum[2] == 0
        if vol is alt:
            assert all(np.count_nonzero(got.hist[c]) == 2 for c in range(4))


# ---- 6. stream order ---------------------------------------------------------------------------
def test_stats_follow_paints_on_a_side_stream(r, base):
    r.set_layout_preference(15)
    r.set_volume(base)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    centre, radius = ps.BRUSHES["straddle"]
    bufs = [poisoned(), poisoned()]
    torch.cuda.synchronize()
    r.paint(centre, radius, ps.ADD, 1, ps.VALUE, ps.STRENGTH, stream=s)
    r.brush_stats(centre, radius, 1, ss.FULL, stream=s, out=bufs[0])
    r.paint(*ps.BRUSHES["whole"], ps.SUB, 0, ps.VALUE, ps.STRENGTH, stream=s)
    r.brush_stats(centre, radius, 1, ss.FULL, stream=s, out=bufs[1])
    s.synchronize()
    once = ps.spec_apply(base, centre, radius, ps.ADD, 1)
    twice = ps.spec_apply(once, *ps.BRUSHES["whole"], ps.SUB, 0)
    wants = [ss.spec_brush_stats(v, centre, radius, 1, ss.FULL) for v in (once, twice)]
    untouched = ss.spec_brush_stats(base, centre, radius, 1, ss.FULL)
    assert any((w["hist"] != untouched["hist"]).any() for w in wants) and (wants[0]["hist"] != wants[1]["hist"]).any()
    for buf, want in zip(bufs, wants):
        ss.assert_stats(vr.unpack_stats(buf), want)
    assert np.array_equal(r.get_volume(), twice)


# ---- 7. the context is left alone --------------------------------------------------------------
@pytest.mark.parametrize("pref,lname", [(1, "planar"), (15, "col48")], ids=["planar", "col48"])
def test_context_left_alone(pref, lname):
    def frame(rr):
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        img = rr.render(W, H, FMT_RGBA32F, step_counter=cnt)
        torch.cuda.synchronize()
        return img.cpu().numpy(), int(cnt.item())

    with vr.Renderer(0) as rr:
        rr.set_option("uniform_skip", 1)
        rr.set_layout_preference(pref)
        rr.generate_volume(vr.volume_recipe_defaults(size=32))
        rr.set_shader_data(*vr.reference_shader_data(1.0))
        rr.set_march(vr.march_defaults(max_steps=STEPS))
        vol = rr.get_volume()
        # a pending uniform-channel read-back: a paint that leaves G alone re-arms it, and nothing resolves it yet
        rr.paint((16, 16, 16), (5, 5, 5), ps.ADD, 1, (40, 0, 0, 0), (255, 0, 0, 0))
        painted = ps.spec_apply(vol, (16, 16, 16), (5, 5, 5), ps.ADD, 1, (40, 0, 0, 0), (255, 0, 0, 0))
        got = brush_stats(rr, (16, 16, 16), (8, 8, 8), 1, ss.FULL)                     # before the first render
        ss.assert_stats(got, ss.spec_brush_stats(painted, (16, 16, 16), (8, 8, 8), 1, ss.FULL))
        img0, steps0 = frame(rr)
        variant0, mask0 = rr.kernel_variant, rr.get_option("uniform_mask")
        assert variant0.startswith(f"grid_{lname}_clamp"), variant0
        assert mask0 & 2, "the recipe's G is uniform"
        box_stats(rr, *whole(painted))
        brush_stats(rr, (3, 30, 16), (9, 9, 9), 0, (0, 255, 0, 1))
        assert rr.get_option("uniform_mask") == mask0 and rr.kernel_variant == variant0
        img1, steps1 = frame(rr)
        assert np.array_equal(img0.view(np.uint32), img1.view(np.uint32)) and steps0 == steps1
        assert np.array_equal(rr.get_volume(), painted)


# ---- 8. the eyedropper -------------------------------------------------------------------------
def test_eyedropper_round_trip(r, base):
    r.set_layout_preference(0)
    r.set_volume(base)
    centre, radius = ps.BRUSHES["interior"]
    strength = (255, 255, 0, 255)
    picked = vr.stats_summary(r.brush_stats(centre, radius, 1, strength))
    want = ss.spec_summary(ss.spec_brush_stats(base, centre, radius, 1, strength))
    assert np.array_equal(picked.wmean, want["wmean"]) and picked.n[2] == 0 and picked.wmean[2] == 0
    assert (picked.min < picked.max)[[0, 1, 3]].all()
    r.paint(centre, radius, ps.SET, 0, tuple(int(v) for v in picked.wmean), strength)
    after = vr.stats_summary(r.brush_stats(centre, radius, 0, strength))
    for c in (0, 1, 3):
        assert after.min[c] == after.max[c] == picked.wmean[c] == after.wmean[c] == after.median[c]
    assert after.n[2] == 0
    still = vr.stats_summary(r.brush_stats(centre, radius, 0, (0, 0, 255, 0)))        # B was not painted
    assert still.min[2] < still.max[2]


# ---- 9. refusals -------------------------------------------------------------------------------
def test_refusals(r, base):
    r.set_layout_preference(0)
    r.set_volume(base)
    good = dict(centre=(17, 11, 23), radius=(3, 2, 4))
    buf = poisoned()
    keep = buf.cpu().numpy().copy()

    def unchanged():
        torch.cuda.synchronize()
        return np.array_equal(buf.cpu().numpy(), keep) and np.array_equal(r.get_volume(), base)

    for kw in (dict(good, radius=(3, 256, 4)), dict(good, radius=(-1, 2, 4)), dict(good, falloff=2)):
        with pytest.raises(vr.VRError) as e:
            r.brush_stats(out=buf, **kw)
        assert e.value.status == 1 and "vr_brush_stats" in str(e.value), kw   # VR_ERR_INVALID
        assert unchanged()
    big = torch.full((BYTES + 8,), 0xFF, dtype=torch.uint8, device="cuda")
    for off in (1, 4):
        view = big[off:off + BYTES]
        assert view.data_ptr() % 8 == off
        with pytest.raises(vr.VRError) as e:
            r.brush_stats(out=view, **good)
        assert e.value.status == 1 and "aligned" in str(e.value)
        with pytest.raises(vr.VRError) as e:
            r.box_stats((0, 0, 0), (1, 1, 1), out=view)
        assert e.value.status == 1 and "aligned" in str(e.value)
    torch.cuda.synchronize()
    assert (big.cpu().numpy() == 0xFF).all()
    for origin, extent, mask in (((0, 0, 0), (NX + 1, 1, 1), 15), ((-1, 0, 0), (1, 1, 1), 15), ((0, 0, 44), (1, 1, 2), 15),
                                 ((0, 0, 0), (0, 1, 1), 15), ((0, 0, 0), (1, 1, 1), 16), ((0, 0, 0), (1, 1, 1), -1)):
        with pytest.raises(vr.VRError) as e:
            r.box_stats(origin, extent, mask, out=buf)
        assert e.value.status == 1 and "vr_box_stats" in str(e.value), (origin, extent, mask)
        assert unchanged()
    with pytest.raises(vr.VRError) as e:
        _lib.call("vr_brush_stats", r._ctx, None, ctypes.c_void_p(buf.data_ptr()), None)
    assert e.value.status == 1
    with pytest.raises(ValueError):
        r.brush_stats(out=torch.zeros(BYTES, dtype=torch.uint8), **good)          # a host tensor
    with pytest.raises(ValueError):
        r.box_stats((0, 0, 0), (1, 1, 1), out=torch.zeros(BYTES - 8, dtype=torch.uint8, device="cuda"))
    assert unchanged()
    with vr.Renderer(0) as empty:                                                 # no volume installed
        for fn in (lambda: empty.brush_stats(out=buf, **good), lambda: empty.box_stats((0, 0, 0), (1, 1, 1), out=buf)):
            with pytest.raises(vr.VRError) as e:
                fn()
            assert e.value.status == 3                                            # VR_ERR_NO_VOLUME
    assert unchanged()
    r.set_procedural()                                                            # a procedural medium reads no volume
    try:
        for fn in (lambda: r.brush_stats(out=buf, **good), lambda: r.box_stats((0, 0, 0), (1, 1, 1), out=buf)):
            with pytest.raises(vr.VRError) as e:
                fn()
            assert e.value.status == 3
    finally:
        r.set_procedural(vr.procedural_defaults(enabled=0))
    assert unchanged()
    # a miss and an all-zero strength are VR_OK: the first zeroes the buffer, the second still counts
    r.brush_stats((-10, -10, -10), (4, 4, 4), out=buf)
    torch.cuda.synchronize()
    assert not buf.cpu().numpy().any()
    got = brush_stats(r, good["centre"], good["radius"], 0, (0, 0, 0, 0))
    assert got.count > 0 and got.weight == 256 * got.count and not got.hist.any() and not got.wsum.any()
