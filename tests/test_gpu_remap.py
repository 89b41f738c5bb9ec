"""vr_remap, vr_remap_device and vr_stats_lut_device on the GPU: the edited
volume against the numpy restatement (tests/remap_spec.py), byte for byte, for
every brush x table x op x falloff through the host table and the device
table; volumes that cut the row loop; when each kind of table is read; the
device's tables from stats against the host's; stats -> table -> remap ->
footprint -> render_rect on one side stream; the edited context's frame
against a fresh install of the specification's volume and the CPU oracle, per
layout; uniform channels; a remap among a blur and a staged clone; refusals.
Everything is exact.

The volume is paint_spec.base_volume() (37 x 22 x 45 random bytes); frame,
march and cameras are brush_harness.py's: the reference camera at 64 x 64,
32 steps.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blur_spec as bs  # noqa: E402
import clone_spec as cs  # noqa: E402
import paint_spec as ps  # noqa: E402
import remap_spec as rs  # noqa: E402
from brush_harness import (FULL, H, LAYOUT_IDS, LAYOUTS, UNIFORM_LAYOUTS, VOLUME_BRUSHES, W, assert_exact,  # noqa: E402,F401
                           assert_marches, base, check_frame, check_fresh_install, frame, fresh, oracle_frame, r,
                           recipe_volume, setup)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import volumetricrenderer_amd as vr
from volumetricrenderer_amd import _lib  # noqa: E402
from volumetricrenderer_amd._lib import FMT_RGBA32F  # noqa: E402

NX, NY, NZ = ps.NX, ps.NY, ps.NZ
DIMS = (NX, NY, NZ)
T = rs.TABLES


@pytest.fixture(scope="module")
def skewed():
    return rs.skewed_volume()


def dev(lut):
    return torch.from_numpy(np.ascontiguousarray(lut)).cuda()


# ---- 1. the remapped volume is the specification's, through both kinds of table -----------------
@pytest.mark.parametrize("tname", list(T))
@pytest.mark.parametrize("name", VOLUME_BRUSHES)
def test_remapped_volume_equals_the_specification(r, base, name, tname):
    r.set_layout_preference(14)
    centre, radius = ps.BRUSHES[name]
    d_lut = dev(T[tname])
    for op, _ in ps.OPS:
        for falloff, _ in ps.FALLOFFS:
            want = rs.spec_remap(base, T[tname], centre, radius, op, falloff, cs.STRENGTH)
            for lut in (T[tname], d_lut):
                r.set_volume(base)
                assert r.remap(centre, radius, lut, op, falloff, cs.STRENGTH) == ps.spec_box(centre, radius)
                assert_exact(r.get_volume(), want)
            if name == "miss" or (tname == "identity" and op == ps.SET):
                assert (want == base).all()
    if name in ("interior", "whole") and tname != "identity":
        assert (rs.spec_remap(base, T[tname], centre, radius, ps.SET, 0, cs.STRENGTH) != base).any()


def test_a_zero_channel_is_neither_read_nor_written(r, base):
    """Strength 0 on G: its plane stays, and its table is never read -- the device table here is three channels
    long where it matters: G's 256 bytes are poisoned and differ from the host table's."""
    r.set_layout_preference(0)
    centre, radius = ps.BRUSHES["whole"]
    poisoned = T["perm"].copy()
    poisoned[1] = 0xEE
    for lut in (poisoned, dev(poisoned)):
        r.set_volume(base)
        r.remap(centre, radius, lut, ps.SET, 1, rs.ZERO_CHANNEL)
        want = rs.spec_remap(base, T["perm"], centre, radius, ps.SET, 1, rs.ZERO_CHANNEL)
        assert (want[..., 1] == base[..., 1]).all() and (want != base).any()
        assert_exact(r.get_volume(), want)


# ---- 2. volumes that cut the row loop ----------------------------------------------------------
@pytest.mark.parametrize("dims", [(1, 1, 1), (131, 2, 3), (3, 70, 2)], ids=["1x1x1", "131x2x3", "3x70x2"])
def test_small_volumes(r, dims):
    """1 x 1 x 1: one row, three waves of the workgroup have none and still reach both barriers; 131 x 2 x 3: rows
    longer than two passes of the 64 lanes, six rows; 3 x 70 x 2: rows shorter than a wave, more rows than a
    workgroup has waves."""
    nx, ny, nz = dims
    vol = np.random.default_rng(nx * 1000 + ny).integers(0, 256, size=(nz, ny, nx, 4), dtype=np.uint8)
    centre, radius = (nx // 2, ny // 2, nz // 2), (255, 255, 255)
    inside, _ = ps.spec_weights(vol.shape[:3], centre, radius, 0)
    assert inside.all()
    r.set_layout_preference(0)
    for tname in ("perm", "invert", "levels_narrow"):
        d_lut = dev(T[tname])
        for op, falloff in ((ps.SET, 0), (ps.ADD, 1), (ps.SUB, 1)):
            want = rs.spec_remap(vol, T[tname], centre, radius, op, falloff, FULL)
            assert (want != vol).any()
            for lut in (T[tname], d_lut):
                r.set_volume(vol)
                assert r.remap(centre, radius, lut, op, falloff, FULL) == ((0, 0, 0), dims)
                assert_exact(r.get_volume(), want)


# ---- 3. when the table is read ------------------------------------------------------------------
def test_the_host_table_is_copied_at_the_call(r, base):
    r.set_layout_preference(14)
    r.set_volume(base)
    centre, radius = ps.BRUSHES["whole"]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    lut = T["perm"].copy()
    r.remap(centre, radius, lut, ps.SET, 1, FULL, stream=s)
    lut[:] = T["invert"]                                               # before anything has been waited for
    r.remap(centre, radius, lut, ps.ADD, 0, FULL, stream=s)            # a second queued call with its own table
    lut[:] = 0
    s.synchronize()
    first = rs.spec_remap(base, T["perm"], centre, radius, ps.SET, 1, FULL)
    want = rs.spec_remap(first, T["invert"], centre, radius, ps.ADD, 0, FULL)
    assert (want != rs.spec_remap(first, np.zeros_like(lut), centre, radius, ps.ADD, 0, FULL)).any()
    assert_exact(r.get_volume(), want)


def test_the_device_table_is_read_when_the_kernel_runs(r, base):
    r.set_layout_preference(14)
    centre, radius = ps.BRUSHES["whole"]
    a, b = dev(T["perm"]), dev(T["levels_narrow"])
    want_a = rs.spec_remap(base, T["perm"], centre, radius, ps.SET, 0, FULL)
    want_b = rs.spec_remap(base, T["levels_narrow"], centre, radius, ps.SET, 0, FULL)
    assert (want_a != want_b).any()
    s = torch.cuda.Stream()
    for b_first in (False, True):
        r.set_volume(base)
        d_lut = torch.zeros(1024, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            d_lut.copy_(a.reshape(-1), non_blocking=True)
            if b_first:
                d_lut.copy_(b.reshape(-1), non_blocking=True)
            r.remap(centre, radius, d_lut, ps.SET, 0, FULL, stream=s)
            if not b_first:
                d_lut.copy_(b.reshape(-1), non_blocking=True)
        s.synchronize()
        assert_exact(r.get_volume(), want_b if b_first else want_a)


# ---- 4. tables from stats on the device ---------------------------------------------------------
def test_stats_lut_device_equals_the_host(r, skewed):
    r.set_layout_preference(0)
    r.set_volume(skewed)
    centre, radius = ps.BRUSHES[rs.STATS_BRUSH[0]]
    bufs = {
        "brush": r.brush_stats(centre, radius, rs.STATS_BRUSH[1], FULL, out=torch.empty(vr.VOLUME_STATS_BYTES, dtype=torch.uint8, device="cuda")),
        "interior": r.brush_stats(*ps.BRUSHES["interior"], 0, (255, 128, 0, 1),
                                  out=torch.empty(vr.VOLUME_STATS_BYTES, dtype=torch.uint8, device="cuda")),
        "box": r.box_stats((0, 0, 0), DIMS, 0xF, out=torch.empty(vr.VOLUME_STATS_BYTES, dtype=torch.uint8, device="cuda")),
        "zero": torch.zeros(vr.VOLUME_STATS_BYTES, dtype=torch.uint8, device="cuda"),
    }
    torch.cuda.synchronize()
    ident = rs.spec_identity()
    for name, buf in bufs.items():
        st = vr.unpack_stats(buf)
        for kind in (vr.LUT_EQUALIZE, vr.LUT_STRETCH):
            for mask in (0, 5, 15):
                want = rs.spec_stats_lut(st.hist, kind, mask)
                assert_exact(vr.stats_lut(st, kind, mask), want)
                out = torch.full((4, 256), 0xAB, dtype=torch.uint8, device="cuda")
                got = r.stats_lut(buf, kind, mask, out=out)
                torch.cuda.synchronize()
                assert got is out
                assert_exact(got.cpu().numpy(), want)
                if name == "zero" or mask == 0:
                    assert (want == ident).all()
    assert_exact(r.stats_lut(bufs["brush"], vr.LUT_EQUALIZE).cpu().numpy(), T["eq"])
    assert_exact(r.stats_lut(bufs["brush"], vr.LUT_STRETCH).cpu().numpy(), T["stretch"])
    # 64-bit bins: a hand-made buffer with bins of 2^31 - 1 and cumulative sums past 2^32
    hist = np.zeros((4, 256), np.uint64)
    hist[0, 40:200] = 2**31 - 1
    hist[1, [0, 128, 255]] = (2**31 - 1, 1, 2**31 - 1)
    hist[2, [100, 101]] = (2**31 - 1, 1)
    words = np.concatenate([np.zeros(6, np.uint64), hist.reshape(-1)])
    big = torch.from_numpy(words.view(np.uint8).copy()).cuda()
    for kind in (vr.LUT_EQUALIZE, vr.LUT_STRETCH):
        got = r.stats_lut(big, kind)
        torch.cuda.synchronize()
        assert_exact(got.cpu().numpy(), rs.spec_stats_lut(hist.astype(object), kind, 15))
    assert_exact(r.get_volume(), skewed)


# ---- 5. one stream, no host wait ----------------------------------------------------------------
@pytest.mark.parametrize("with_pick", [False, True], ids=["chain", "pick+chain"])
def test_stats_table_remap_footprint_rerender_on_a_side_stream(r, fresh, oracle, base, skewed, with_pick):
    """brush_stats -> stats_lut -> remap (device table) -> update_footprint -> render_rect queued on one side
    stream, one synchronise at the end: the volume and the patched frame are those of the host chain installed
    fresh, and the oracle's.  With the pick in front, the brush sits on the texel under a pixel -- on the base
    volume at a density at which rays pass the 0.5 transmittance threshold (a hit), as in test_gpu_clone.py."""
    density = 32.0 if with_pick else 1.0
    pref, lname = 14, "cornerh"
    skewed = base if with_pick else skewed
    setup(r, pref, skewed, density=density)
    assert_marches(r, lname)
    centre, radius = (18, 11, 22), (9, 8, 10)
    if with_pick:
        rec = vr.ray_records(r.query_rect((0, 0, W, H), W, H, 0.5))
        hits = np.argwhere(rec["hit_step"] >= 0)
        assert len(hits) > 0, "no ray has a hit"
        py, px = (int(v) for v in hits[np.argmin(((hits - (H // 2, W // 2)) ** 2).sum(axis=1))])
        one, texel = r.pick(px, py, W, H, 0.5)
        assert one["hit_step"] >= 0 and texel is not None
        centre = tuple(int(v) for v in texel)
    buf = r.render(W, H, FMT_RGBA32F)
    d_stats = torch.empty(vr.VOLUME_STATS_BYTES, dtype=torch.uint8, device="cuda")
    d_lut = torch.zeros((4, 256), dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    r.brush_stats(centre, radius, 1, FULL, stream=s, out=d_stats)
    r.stats_lut(d_stats, vr.LUT_EQUALIZE, 0xF, stream=s, out=d_lut)
    box = r.remap(centre, radius, d_lut, ps.SET, 1, FULL, stream=s)
    assert box is not None
    rect = r.update_footprint(box[0], box[1], W, H)
    r.render_rect(buf, rect, FMT_RGBA32F, stream=s)
    s.synchronize()
    # the host chain
    st = vr.brush_stats_host(vr.make_brush(centre, radius, ps.SET, 1, 0, FULL), skewed)
    lut = vr.stats_lut(st, vr.LUT_EQUALIZE)
    assert_exact(lut, rs.spec_stats_lut(rs.spec_hist(skewed, centre, radius), rs.EQUALIZE, 15))
    assert_exact(d_lut.cpu().numpy(), lut)
    want_vol = rs.spec_remap(skewed, lut, centre, radius, ps.SET, 1, FULL)
    assert_exact(vr.brush_remap_apply(vr.make_brush(centre, radius, ps.SET, 1, 0, FULL), lut, skewed.copy()), want_vol)
    assert_exact(r.get_volume(), want_vol)
    want, want_steps = oracle_frame(oracle, want_vol, density=density)
    before, _ = oracle_frame(oracle, skewed, density=density)
    assert (want != before).any(), "the remap does not change the frame"
    assert_exact(buf.cpu().numpy(), want)
    img, steps = frame(r)
    assert_exact(img, want)
    assert steps == want_steps
    check_fresh_install(fresh, pref, lname, want_vol, img, steps, density=density)


# ---- 6. the edited context renders what a fresh install of the specification's volume renders --
@pytest.mark.parametrize("pref,lname", LAYOUTS, ids=LAYOUT_IDS)
def test_edited_render_equals_fresh_install(r, fresh, oracle, base, pref, lname):
    """A host-table remap and a device-table remap, one after the other."""
    setup(r, pref, base)
    assert_marches(r, lname)
    d_lut = dev(T["levels_narrow"])
    edits = [
        (lambda: r.remap(*ps.BRUSHES["whole"], T["thresh128"], ps.SET, 1, FULL),
         lambda v: rs.spec_remap(v, T["thresh128"], *ps.BRUSHES["whole"], ps.SET, 1, FULL)),
        (lambda: r.remap(*ps.BRUSHES["straddle"], d_lut, ps.SUB, 0, cs.STRENGTH),
         lambda v: rs.spec_remap(v, T["levels_narrow"], *ps.BRUSHES["straddle"], ps.SUB, 0, cs.STRENGTH)),
    ]
    vol = base
    for apply, restate in edits:
        before, _ = oracle_frame(oracle, vol)
        vol = restate(vol)
        ref, ref_steps = oracle_frame(oracle, vol)
        assert (ref != before).any(), "the edit does not change the oracle's frame"
        assert apply() is not None
        assert_marches(r, lname)
        img, steps = check_frame(r, oracle, vol)
        check_fresh_install(fresh, pref, lname, vol, img, steps)


# ---- 7. uniform channels on the recipe volume --------------------------------------------------


def check_uniform(rr, fresh, oracle, pref, lname, vol, uniform):
    assert bool(rr.get_option("uniform_mask") & 2) == uniform
    assert rr.kernel_variant.endswith("_uG") == uniform
    img, steps = check_frame(rr, oracle, vol)
    check_fresh_install(fresh, pref, lname, vol, img, steps)


@pytest.mark.parametrize("pref,lname", UNIFORM_LAYOUTS, ids=[n for _, n in UNIFORM_LAYOUTS])
def test_uniform_channel(r, fresh, oracle, recipe_volume, pref, lname):
    vol, g = recipe_volume
    assert 0 < g < 255 and 255 - g != g
    centre, radius = (15, 17, 14), (6, 5, 7)
    # an identity SET remap of all four channels keeps the bit, through both kinds of table
    setup(r, pref, vol)
    assert r.get_option("uniform_mask") & 2 and r.kernel_variant.endswith("_uG")
    r.remap(centre, radius, T["identity"], ps.SET, 1, FULL)
    r.remap(centre, radius, dev(T["identity"]), ps.SET, 0, FULL)
    check_uniform(r, fresh, oracle, pref, lname, vol, True)
    # invert on the others with strength 0 on G keeps it
    setup(r, pref, vol)
    r.remap(centre, radius, T["invert"], ps.SET, 1, (255, 0, 255, 255))
    kept = rs.spec_remap(vol, T["invert"], centre, radius, ps.SET, 1, (255, 0, 255, 255))
    assert (kept != vol).any() and (kept[..., 1] == g).all()
    check_uniform(r, fresh, oracle, pref, lname, kept, True)
    # invert on all four changes G where it is painted: the bit goes before the next render
    setup(r, pref, vol)
    assert r.get_option("uniform_mask") & 2
    r.remap(centre, radius, dev(T["invert"]), ps.SET, 1, FULL)
    inverted = rs.spec_remap(vol, T["invert"], centre, radius, ps.SET, 1, FULL)
    assert len(np.unique(inverted[..., 1])) > 1
    check_uniform(r, fresh, oracle, pref, lname, inverted, False)
    assert_marches(r, lname)


# ---- 8. a remap among the staged brushes --------------------------------------------------------
def test_remap_blur_and_staged_clone_in_sequence(base):
    centre, radius = ps.BRUSHES["whole"]
    with vr.Renderer(0) as rr:
        rr.set_volume(base)
        assert rr.get_option("blur_scratch_kib") == 0
        rr.set_option("blur_scratch_kib", 1024)
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        rr.remap(centre, radius, T["levels_narrow"], ps.SET, 1, FULL, stream=s)
        assert rr.get_option("blur_scratch_kib") == 1024                  # the remap needs none and takes none
        rr.blur(centre, radius, 1, 1, FULL, stream=s)
        offset, mirror = cs.MAPS["push+x"](centre)
        assert not cs.spec_direct(centre, radius, offset, mirror)
        rr.clone(centre, radius, offset, mirror, ps.SET, 0, FULL, stream=s)
        rr.remap(*ps.BRUSHES["straddle"], dev(T["perm"]), ps.ADD, 0, cs.STRENGTH, stream=s)
        s.synchronize()
        vol = rs.spec_remap(base, T["levels_narrow"], centre, radius, ps.SET, 1, FULL)
        vol = bs.spec_blur(vol, centre, radius, 1, 1, FULL)
        vol = cs.spec_clone(vol, centre, radius, offset, mirror, ps.SET, 0, FULL)
        vol = rs.spec_remap(vol, T["perm"], *ps.BRUSHES["straddle"], ps.ADD, 0, cs.STRENGTH)
        assert_exact(rr.get_volume(), vol)
        assert rr.get_option("blur_scratch_kib") == 1024
    with vr.Renderer(0) as rr:                                            # alone, a remap never makes a scratch
        rr.set_volume(base)
        rr.remap(centre, radius, T["perm"], ps.SET, 1, FULL)
        assert rr.get_option("blur_scratch_kib") == 0


# ---- 9. refusals ---------------------------------------------------------------------------------
def test_refusals(r, base):
    setup(r, 0, base)
    lut = T["perm"]
    flat = torch.zeros(1024 + 8, dtype=torch.uint8, device="cuda")
    flat[:1024] = dev(lut).reshape(-1)
    flat[1024:] = 0x5A
    d_lut = flat[:1024]
    assert d_lut.data_ptr() % 8 == 0
    keep = flat.cpu().numpy().copy()
    d_stats = torch.zeros(vr.VOLUME_STATS_BYTES + 8, dtype=torch.uint8, device="cuda")
    good = dict(centre=(17, 11, 23), radius=(3, 2, 4))

    def untouched():
        torch.cuda.synchronize()
        assert np.array_equal(r.get_volume(), base)
        assert np.array_equal(flat.cpu().numpy(), keep)

    for table, fn in ((lut, "vr_remap"), (d_lut, "vr_remap_device")):
        for kw in (dict(good, falloff=2), dict(good, op=3), dict(good, op=-1), dict(good, radius=(3, 256, 4)),
                   dict(good, radius=(-1, 2, 4))):
            with pytest.raises(vr.VRError) as e:
                r.remap(lut=table, **kw)
            assert e.value.status == 1 and fn in str(e.value), kw   # VR_ERR_INVALID
            untouched()
    for shift in (1, 2, 3):                                             # a misaligned device table
        view = flat[shift:shift + 1024]
        assert view.is_contiguous() and view.data_ptr() % 4 == shift
        with pytest.raises(vr.VRError) as e:
            r.remap(lut=view, **good)
        assert e.value.status == 1 and "vr_remap_device" in str(e.value) and "aligned" in str(e.value)
        with pytest.raises(vr.VRError) as e:
            r.stats_lut(d_stats[:vr.VOLUME_STATS_BYTES], vr.LUT_STRETCH, out=view)
        assert e.value.status == 1 and "vr_stats_lut_device" in str(e.value) and "aligned" in str(e.value)
        untouched()
    for shift in (1, 4, 7):                                             # misaligned stats
        with pytest.raises(vr.VRError) as e:
            r.stats_lut(d_stats[shift:shift + vr.VOLUME_STATS_BYTES], vr.LUT_STRETCH, out=d_lut)
        assert e.value.status == 1 and "d_stats" in str(e.value)
        untouched()
    for kind, mask in ((2, 15), (-1, 15), (0, 16), (1, -1)):
        with pytest.raises(vr.VRError) as e:
            r.stats_lut(d_stats[:vr.VOLUME_STATS_BYTES], kind, mask, out=d_lut)
        assert e.value.status == 1 and "vr_stats_lut_device" in str(e.value)
        untouched()
    for bad_tensor in (d_lut.cpu(), d_lut.to(torch.int8), flat[:1023], flat[:2048:2]):
        with pytest.raises(ValueError):
            r.remap(lut=bad_tensor, **good)
    with pytest.raises(ValueError):
        r.remap(lut=lut[:3], **good)
    b = vr.make_brush((17, 11, 23), (3, 2, 4))
    s = _lib.Lut()
    ctypes.memmove(ctypes.byref(s), lut.ctypes.data, 1024)
    lp, sp = ctypes.c_void_p(d_lut.data_ptr()), ctypes.c_void_p(d_stats.data_ptr())
    for k in range(2):
        bb = vr.make_brush((17, 11, 23), (3, 2, 4))
        bb.reserved[k] = 7
        for args in (("vr_remap", r._ctx, ctypes.byref(bb), ctypes.byref(s), None), ("vr_remap_device", r._ctx, ctypes.byref(bb), lp, None)):
            with pytest.raises(vr.VRError) as e:
                _lib.call(*args)
            assert e.value.status == 1
    for args in (("vr_remap", None, ctypes.byref(b), ctypes.byref(s), None), ("vr_remap", r._ctx, None, ctypes.byref(s), None),
                 ("vr_remap", r._ctx, ctypes.byref(b), None, None), ("vr_remap_device", None, ctypes.byref(b), lp, None),
                 ("vr_remap_device", r._ctx, None, lp, None), ("vr_remap_device", r._ctx, ctypes.byref(b), None, None),
                 ("vr_stats_lut_device", None, sp, 0, 15, lp, None), ("vr_stats_lut_device", r._ctx, None, 0, 15, lp, None),
                 ("vr_stats_lut_device", r._ctx, sp, 0, 15, None, None)):
        with pytest.raises(vr.VRError) as e:
            _lib.call(*args)
        assert e.value.status == 1 and "null" in str(e.value)
    untouched()
    assert r.remap((-10, -10, -10), (4, 4, 4), lut) is None               # a miss is VR_OK
    assert r.remap((-10, -10, -10), (4, 4, 4), d_lut) is None
    assert r.remap(lut=lut, strength=(0, 0, 0, 0), **good) is not None    # nothing to do is VR_OK too
    assert r.remap(lut=d_lut, strength=(0, 0, 0, 0), **good) is not None
    untouched()
    with vr.Renderer(0) as empty:                                         # no volume installed
        for table in (lut, d_lut):
            with pytest.raises(vr.VRError) as e:
                empty.remap(lut=table, **good)
            assert e.value.status == 3                                    # VR_ERR_NO_VOLUME
        out = empty.stats_lut(d_stats[:vr.VOLUME_STATS_BYTES], vr.LUT_EQUALIZE)   # needs no volume
        torch.cuda.synchronize()
        assert_exact(out.cpu().numpy(), rs.spec_identity())
    r.set_procedural()                                                    # a procedural medium reads no volume
    try:
        for table in (lut, d_lut):
            with pytest.raises(vr.VRError) as e:
                r.remap(lut=table, **good)
            assert e.value.status == 3
        out = r.stats_lut(d_stats[:vr.VOLUME_STATS_BYTES], vr.LUT_STRETCH)        # accepted all the same
        torch.cuda.synchronize()
        assert_exact(out.cpu().numpy(), rs.spec_identity())
    finally:
        r.set_procedural(vr.procedural_defaults(enabled=0))
    untouched()
