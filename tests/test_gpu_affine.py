"""vr_stamp_affine and vr_clone_affine on the GPU: the edited volume against the
numpy restatement (tests/affine_spec.py), byte for byte, for every brush x map
x filter x op x falloff; volumes that cut the row loop; the path the host
picks, seen through the staging scratch; a source taken with get_volume_box on
the device and pasted rotated on one side stream, the patched frame against a
fresh install and the CPU oracle, per layout; uniform channels; refusals.
Everything is exact.

The volume is paint_spec.base_volume() (37 x 22 x 45 random bytes); frame,
march and cameras are brush_harness.py's: the reference camera at 64 x 64,
32 steps.
"""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affine_spec as af  # noqa: E402
import paint_spec as ps  # noqa: E402
from brush_harness import (FULL, H, LAYOUT_IDS, LAYOUTS, UNIFORM_LAYOUTS, VOLUME_BRUSHES, W, assert_exact,  # noqa: E402,F401
                           assert_marches, base, check_frame, check_fresh_install, check_needs_a_volume, frame, fresh,
                           oracle_frame, r, recipe_volume, setup)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import volumetricrenderer_amd as vr
from volumetricrenderer_amd import _lib  # noqa: E402
from volumetricrenderer_amd._lib import FMT_RGBA32F  # noqa: E402

NX, NY, NZ = ps.NX, ps.NY, ps.NZ
DIMS = (NX, NY, NZ)


@pytest.fixture(scope="module")
def stamp():
    return af.stamp_bytes()


@pytest.fixture(scope="module")
def d_stamp(stamp):
    return torch.from_numpy(stamp).cuda()


def affine(table, filt=af.NEAREST, border=af.CLAMP):
    return vr.make_affine(*table, filt, border)


# ---- 1. the pasted volume is the specification's ----------------------------------------------
@pytest.mark.parametrize("mname", list(af.MAPS))
@pytest.mark.parametrize("name", VOLUME_BRUSHES)
def test_pasted_volume_equals_the_specification(r, base, stamp, d_stamp, name, mname):
    r.set_layout_preference(14)
    centre, radius = ps.BRUSHES[name]
    changed = False
    for src, table in ((None, af.MAPS[mname](centre, centre)), (stamp, af.MAPS[mname](centre, af.STAMP_CENTRE))):
        for filt, _ in af.FILTERS:
            sampled = af.sample(base if src is None else src, table, filt, base.shape[:3])
            for border in af.BORDERS[mname]:
                a = affine(table, filt, border)
                for (op, _), (falloff, _) in itertools.product(ps.OPS, ps.FALLOFFS):
                    r.set_volume(base)
                    if src is None:
                        box = r.clone_affine(centre, radius, a, op, falloff, af.STRENGTH)
                    else:
                        box = r.stamp_affine(d_stamp, a, centre, radius, op, falloff, af.STRENGTH)
                    assert box == ps.spec_box(centre, radius)
                    want = af.spec_affine(base, src, table, filt, border, centre, radius, op, falloff, sampled=sampled)
                    assert_exact(r.get_volume(), want)
                    changed = changed or (want != base).any()
    assert changed == (name != "miss")


# ---- 2. volumes that cut the row loop ----------------------------------------------------------
@pytest.mark.parametrize("dims", [(1, 1, 1), (3, 1, 2), (65, 2, 2), (64, 64, 1)], ids=["1x1x1", "3x1x2", "65x2x2", "64x64x1"])
def test_volumes_that_cut_the_row_loop(r, stamp, d_stamp, dims):
    """One texel; rows shorter than a wave; a row one texel longer than the 64 lanes; 64 rows of exactly 64 lanes in
    one slice -- more rows than a workgroup has waves.  The brush is `whole`; the maps turn about the volume's middle."""
    nx, ny, nz = dims
    vol = np.random.default_rng(nx * 1000 + ny).integers(0, 256, size=(nz, ny, nx, 4), dtype=np.uint8)
    centre, radius = ps.BRUSHES["whole"]
    mid = (nx // 2, ny // 2, nz // 2)
    r.set_layout_preference(0)
    changed = False
    for mname in ("rot30_axis", "shift_half", "flip", "off_source"):
        for src, table in ((None, af.MAPS[mname](mid, mid)), (stamp, af.MAPS[mname](mid, af.STAMP_CENTRE))):
            for (filt, _), border in itertools.product(af.FILTERS, (af.CLAMP, af.SKIP)):
                a = affine(table, filt, border)
                for op, falloff in ((ps.SET, 0), (ps.ADD, 1)):
                    r.set_volume(vol)
                    if src is None:
                        r.clone_affine(centre, radius, a, op, falloff, FULL)
                    else:
                        r.stamp_affine(d_stamp, a, centre, radius, op, falloff, FULL)
                    want = af.spec_affine(vol, src, table, filt, border, centre, radius, op, falloff, FULL)
                    assert_exact(r.get_volume(), want)
                    changed = changed or (want != vol).any()
    assert changed


# ---- 3. the path choice is observable; both paths give the specification's bytes ---------------
def test_path_choice(base):
    centre, radius = ps.BRUSHES["interior"]
    far, rot = af.MAPS["far"](centre, centre), af.MAPS["rot30_axis"](centre, centre)
    for filt, _ in af.FILTERS:
        assert af.spec_direct(far, filt, centre, radius) and not af.spec_direct(rot, filt, centre, radius)
    with vr.Renderer(0) as rr:
        assert rr.get_option("blur_scratch_kib") == 0
        rr.set_volume(base)
        vol = base
        for filt, _ in af.FILTERS:
            rr.clone_affine(centre, radius, affine(far, filt), ps.SET, 1, af.STRENGTH)
            vol = af.spec_affine(vol, None, far, filt, af.CLAMP, centre, radius, ps.SET, 1)
            assert_exact(rr.get_volume(), vol)
            assert rr.get_option("blur_scratch_kib") == 0             # direct: one launch, no scratch
        assert rr.clone_affine(*ps.BRUSHES["miss"], affine(rot)) is None
        assert rr.clone_affine(centre, radius, affine(rot), strength=(0, 0, 0, 0)) is not None
        assert rr.get_option("blur_scratch_kib") == 0                 # no launch, no scratch
        for filt, _ in af.FILTERS:
            rr.clone_affine(centre, radius, affine(rot, filt), ps.SET, 1, af.STRENGTH)
            vol = af.spec_affine(vol, None, rot, filt, af.CLAMP, centre, radius, ps.SET, 1)
            assert_exact(rr.get_volume(), vol)
            assert rr.get_option("blur_scratch_kib") == 1024           # staged: the blur's scratch, rounded up to 1 MiB
        # the same map by both paths: a stamp of the whole volume is the direct statement of the staged clone
        d_vol = torch.from_numpy(vol).cuda()
        want = af.spec_affine(vol, None, rot, af.LINEAR, af.SKIP, *ps.BRUSHES["whole"], ps.ADD, 1, FULL)
        rr.clone_affine(*ps.BRUSHES["whole"], affine(rot, af.LINEAR, af.SKIP), ps.ADD, 1, FULL)
        assert_exact(rr.get_volume(), want)
        rr.set_volume(vol)
        rr.stamp_affine(d_vol, affine(rot, af.LINEAR, af.SKIP), *ps.BRUSHES["whole"], ps.ADD, 1, FULL)
        assert_exact(rr.get_volume(), want)


# ---- 4. a source taken on the device, pasted rotated, one stream, no host wait -----------------
@pytest.mark.parametrize("pref,lname", LAYOUTS, ids=LAYOUT_IDS)
def test_copy_rotate_paste_rerender_on_a_side_stream(r, fresh, oracle, base, pref, lname):
    setup(r, pref, base)
    assert_marches(r, lname)
    src_origin, extent = (2, 12, 28), (11, 8, 13)
    centre, radius = ps.BRUSHES["straddle"]
    x, y, z = src_origin
    cut = np.ascontiguousarray(base[z:z + extent[2], y:y + extent[1], x:x + extent[0]])
    table = af.MAPS["rot30_axis"](centre, (5, 4, 6))
    a = affine(table, af.LINEAR, af.CLAMP)
    buf = r.render(W, H, FMT_RGBA32F)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    saved = r.get_volume_box(src_origin, extent, stream=s)
    box = r.stamp_affine(saved, a, centre, radius, ps.SET, 1, FULL, stream=s)
    assert box == ps.spec_box(centre, radius)
    rect = r.update_footprint(box[0], box[1], W, H)
    r.render_rect(buf, rect, FMT_RGBA32F, stream=s)
    s.synchronize()
    assert np.array_equal(saved.cpu().numpy(), cut)
    pasted = af.spec_affine(base, cut, table, af.LINEAR, af.CLAMP, centre, radius, ps.SET, 1, FULL)
    assert_exact(r.get_volume(), pasted)
    want, want_steps = oracle_frame(oracle, pasted)
    before, _ = oracle_frame(oracle, base)
    assert (want != before).any(), "the paste does not change the frame"
    assert_exact(buf.cpu().numpy(), want)
    assert_marches(r, lname)
    img, steps = frame(r)
    assert_exact(img, want)
    assert steps == want_steps
    check_fresh_install(fresh, pref, lname, pasted, img, steps)


# ---- 5. uniform channels on the recipe volume --------------------------------------------------


def check_uniform(rr, fresh, oracle, pref, lname, vol, uniform):
    assert bool(rr.get_option("uniform_mask") & 2) == uniform
    assert rr.kernel_variant.endswith("_uG") == uniform
    img, steps = check_frame(rr, oracle, vol)
    check_fresh_install(fresh, pref, lname, vol, img, steps)


@pytest.mark.parametrize("pref,lname", UNIFORM_LAYOUTS, ids=[n for _, n in UNIFORM_LAYOUTS])
def test_uniform_channel(r, fresh, oracle, recipe_volume, pref, lname):
    vol, g = recipe_volume
    assert 0 < g < 255
    centre, radius = (15, 17, 14), (6, 5, 7)
    setup(r, pref, vol)
    assert r.get_option("uniform_mask") & 2 and r.kernel_variant.endswith("_uG")
    # SET pastes of all four channels, trilinear, staged, cannot break G
    for mname in ("identity", "rot30_axis"):
        table = af.MAPS[mname](centre, (10, 20, 12))
        r.clone_affine(centre, radius, affine(table, af.LINEAR), ps.SET, 1, FULL)
        new = af.spec_affine(vol, None, table, af.LINEAR, af.CLAMP, centre, radius, ps.SET, 1, FULL)
        assert (new != vol).any() and (new[..., 1] == g).all()
        vol = new
    d_src = r.get_volume_box((3, 4, 5), (12, 10, 9), stream=torch.cuda.current_stream())
    src = d_src.cpu().numpy()
    table = af.MAPS["rot30_axis"](centre, (6, 5, 4))
    r.stamp_affine(d_src, affine(table, af.LINEAR), centre, radius, ps.SET, 1, FULL)
    new = af.spec_affine(vol, src, table, af.LINEAR, af.CLAMP, centre, radius, ps.SET, 1, FULL)
    assert (new != vol).any() and (new[..., 1] == g).all()
    vol = new
    check_uniform(r, fresh, oracle, pref, lname, vol, True)
    # an ADD paste changes G where it is painted: the bit goes before the next render
    setup(r, pref, vol)
    assert r.get_option("uniform_mask") & 2
    r.clone_affine(centre, radius, affine(table, af.LINEAR), ps.ADD, 1, FULL)
    added = af.spec_affine(vol, None, table, af.LINEAR, af.CLAMP, centre, radius, ps.ADD, 1, FULL)
    assert len(np.unique(added[..., 1])) > 1
    check_uniform(r, fresh, oracle, pref, lname, added, False)
    assert_marches(r, lname)


# ---- 6, 7. refusals ----------------------------------------------------------------------------
def test_refusals(r, base, d_stamp):
    setup(r, 0, base)
    centre, radius = ps.BRUSHES["interior"]
    good = affine(af.MAPS["rot30_axis"](centre, centre), af.LINEAR)

    def bad_maps():
        for k, v in (("filter", 2), ("filter", -1), ("border", 2), ("border", -1), ("reserved", 1)):
            a = affine(af.MAPS["identity"](centre, centre))
            setattr(a, k, v)
            yield a
        for v in (256 * 65536 + 1, -256 * 65536 - 1, -2**31):
            a = affine(af.MAPS["identity"](centre, centre))
            a.m[2][0] = v
            yield a

    for a in bad_maps():
        for name, call in (("vr_clone_affine", lambda: r.clone_affine(centre, radius, a)),
                           ("vr_stamp_affine", lambda: r.stamp_affine(d_stamp, a, centre, radius))):
            with pytest.raises(vr.VRError) as e:
                call()
            assert e.value.status == 1 and name in str(e.value)       # VR_ERR_INVALID
            assert np.array_equal(r.get_volume(), base)
    for kw in (dict(falloff=2), dict(op=3), dict(op=-1), dict(radius=(3, 256, 4)), dict(radius=(-1, 2, 4))):
        args = dict(dict(centre=centre, radius=radius, affine=good), **kw)
        for name, call in (("vr_clone_affine", lambda: r.clone_affine(**args)),
                           ("vr_stamp_affine", lambda: r.stamp_affine(stamp_tensor=d_stamp, **args))):
            with pytest.raises(vr.VRError) as e:
                call()
            assert e.value.status == 1 and name in str(e.value), kw
            assert np.array_equal(r.get_volume(), base)
    with pytest.raises(vr.VRError) as e:
        r.stamp_affine(d_stamp[:0], good, centre, radius)              # an empty source
    assert e.value.status == 1 and "vr_stamp_affine" in str(e.value) and "extent" in str(e.value)
    for bad_tensor in (d_stamp.cpu(), d_stamp.to(torch.int8), d_stamp[:, :, :, :3], d_stamp[:, ::2]):
        with pytest.raises(ValueError):
            r.stamp_affine(bad_tensor, good, centre, radius)
    b, ptr = vr.make_brush(centre, radius), ctypes.c_void_p(d_stamp.data_ptr())
    ext = af.STAMP_EXTENT
    for bad_ext in ((0, 9, 11), (13, -1, 11), (13, 9, 32769)):
        with pytest.raises(vr.VRError) as e:
            _lib.call("vr_stamp_affine", r._ctx, ctypes.byref(b), ptr, *bad_ext, ctypes.byref(good), None)
        assert e.value.status == 1 and "extent" in str(e.value)
    for k in range(2):
        bb = vr.make_brush(centre, radius)
        bb.reserved[k] = 7
        for args in (("vr_clone_affine", r._ctx, ctypes.byref(bb), ctypes.byref(good), None),
                     ("vr_stamp_affine", r._ctx, ctypes.byref(bb), ptr, *ext, ctypes.byref(good), None)):
            with pytest.raises(vr.VRError) as e:
                _lib.call(*args)
            assert e.value.status == 1 and args[0] in str(e.value)
    for args in (("vr_clone_affine", r._ctx, None, ctypes.byref(good), None), ("vr_clone_affine", r._ctx, ctypes.byref(b), None, None),
                 ("vr_stamp_affine", r._ctx, None, ptr, *ext, ctypes.byref(good), None),
                 ("vr_stamp_affine", r._ctx, ctypes.byref(b), None, *ext, ctypes.byref(good), None),
                 ("vr_stamp_affine", r._ctx, ctypes.byref(b), ptr, *ext, None, None)):
        with pytest.raises(vr.VRError) as e:
            _lib.call(*args)
        assert e.value.status == 1 and "null" in str(e.value) and args[0] in str(e.value)
    assert np.array_equal(r.get_volume(), base)
    assert r.clone_affine(*ps.BRUSHES["miss"], good) is None            # a miss is VR_OK
    assert r.stamp_affine(d_stamp, good, *ps.BRUSHES["miss"]) is None
    assert r.clone_affine(centre, radius, good, strength=(0, 0, 0, 0)) is not None   # nothing to do is VR_OK too
    assert r.stamp_affine(d_stamp, good, centre, radius, strength=(0, 0, 0, 0)) is not None
    assert np.array_equal(r.get_volume(), base)
    check_needs_a_volume(r, lambda rr: rr.clone_affine(centre, radius, good),
                         lambda rr: rr.stamp_affine(d_stamp, good, centre, radius))
    assert np.array_equal(r.get_volume(), base)


def test_a_misaligned_source_is_refused(r, base):
    r.set_layout_preference(0)
    r.set_volume(base)
    centre, radius = ps.BRUSHES["interior"]
    a = affine((af.I3, (16, 10, 22), (0, 0, 0)), af.LINEAR, af.SKIP)
    flat = torch.zeros(3 * 3 * 3 * 4 + 4, dtype=torch.uint8, device="cuda")
    assert flat.data_ptr() % 4 == 0
    for shift in (1, 2, 3):
        view = flat[shift:shift + 108].view(3, 3, 3, 4)
        assert view.is_contiguous() and view.data_ptr() % 4 == shift
        with pytest.raises(vr.VRError) as e:
            r.stamp_affine(view, a, centre, radius)
        assert e.value.status == 1 and "vr_stamp_affine" in str(e.value) and "aligned" in str(e.value)
        assert np.array_equal(r.get_volume(), base)
    assert r.stamp_affine(flat[4:].view(3, 3, 3, 4), a, centre, radius) == ps.spec_box(centre, radius)
    got = r.get_volume()
    assert (got[22:25, 10:13, 16:19, :] == 0).any()
    got[22:25, 10:13, 16:19, :] = base[22:25, 10:13, 16:19, :]
    assert np.array_equal(got, base)                                    # SKIP: nothing outside the 3 x 3 x 3 source
