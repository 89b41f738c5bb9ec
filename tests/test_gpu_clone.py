"""vr_clone and vr_stamp on the GPU: the edited volume against the numpy
restatement (tests/clone_spec.py), byte for byte, for every brush x map x op x
falloff; volumes that cut the row loop; the path the host picks, seen through
the staging scratch; stamps read with get_volume_box on the device; the edited
context's frame against a fresh install of the specification's volume and the
CPU oracle, per layout; pick -> clone -> footprint -> render_rect on one side
stream; uniform channels; refusals.  Everything is exact.

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
import morph_spec as ms  # noqa: E402
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


def clone(rr, name, mname, op=ps.SET, falloff=0, strength=cs.STRENGTH, stream=None):
    centre, radius = ps.BRUSHES[name]
    offset, mirror = cs.MAPS[mname](centre)
    return rr.clone(centre, radius, offset, mirror, op, falloff, strength, stream=stream)


def spec(vol, name, mname, op=ps.SET, falloff=0, strength=cs.STRENGTH):
    centre, radius = ps.BRUSHES[name]
    offset, mirror = cs.MAPS[mname](centre)
    return cs.spec_clone(vol, centre, radius, offset, mirror, op, falloff, strength)


# ---- 1. the cloned volume is the specification's ----------------------------------------------
@pytest.mark.parametrize("mname", list(cs.MAPS))
@pytest.mark.parametrize("name", VOLUME_BRUSHES)
def test_cloned_volume_equals_the_specification(r, base, name, mname):
    r.set_layout_preference(14)
    centre, radius = ps.BRUSHES[name]
    for op, _ in ps.OPS:
        for falloff, _ in ps.FALLOFFS:
            r.set_volume(base)
            assert clone(r, name, mname, op, falloff) == ps.spec_box(centre, radius)
            want = spec(base, name, mname, op, falloff)
            assert_exact(r.get_volume(), want)
            if name == "miss" or (mname == "identity" and op == ps.SET):
                assert (want == base).all()
    if name == "interior" and mname != "identity":
        assert (spec(base, name, mname) != base).any()


# ---- 2. volumes that cut the row loop ----------------------------------------------------------
def test_a_one_texel_volume(r):
    one = np.array([[[[9, 200, 0, 255]]]], np.uint8)
    r.set_layout_preference(0)
    for mname in cs.MAPS:
        for op, _ in ps.OPS:
            offset, mirror = cs.MAPS[mname]((0, 0, 0))
            r.set_volume(one)
            assert r.clone((0, 0, 0), (255, 255, 255), offset, mirror, op, 1, FULL) == ((0, 0, 0), (1, 1, 1))
            want = cs.spec_clone(one, (0, 0, 0), (255, 255, 255), offset, mirror, op, 1, FULL)   # its own source
            assert_exact(r.get_volume(), want)
            assert (want == one).all() == (op == ps.SET)


@pytest.mark.parametrize("dims", [(131, 2, 3), (3, 70, 2)], ids=["131x2x3", "3x70x2"])
def test_thin_volumes(r, dims):
    """131 x 2 x 3: a row longer than two passes of the 64 lanes, under a brush wider than 64 lanes, with the
    pushes along x and a mirror about the middle column; 3 x 70 x 2: rows shorter than a wave, more rows than a
    workgroup has waves."""
    nx, ny, nz = dims
    vol = np.random.default_rng(nx * 1000 + ny).integers(0, 256, size=(nz, ny, nx, 4), dtype=np.uint8)
    centre, radius = (nx // 2, ny // 2, nz // 2), (255, 255, 255)
    inside, _ = ps.spec_weights(vol.shape[:3], centre, radius, 0)
    assert inside.all()
    maps = [((1, 0, 0), (0, 0, 0)), ((-1, 0, 0), (0, 0, 0)), ((2 * centre[0], 0, 0), (1, 0, 0)), ((0, 1, 0), (0, 0, 0)),
            ((0, -1, 0), (0, 0, 0)), ((0, 2 * centre[1], 0), (0, 1, 0)), ((nx, 0, 0), (0, 0, 0)), ((-70, 3, 1), (1, 0, 1))]
    r.set_layout_preference(0)
    for offset, mirror in maps:
        for op, falloff in ((ps.SET, 0), (ps.ADD, 1), (ps.SUB, 1)):
            r.set_volume(vol)
            assert r.clone(centre, radius, offset, mirror, op, falloff, FULL) == ((0, 0, 0), dims)
            want = cs.spec_clone(vol, centre, radius, offset, mirror, op, falloff, FULL)
            assert (want != vol).mean() > 0.2
            assert_exact(r.get_volume(), want)


# ---- 3. the path choice is observable; the scratch is the blur's ------------------------------
def test_path_choice_and_shared_scratch(base):
    centre, radius = ps.BRUSHES["interior"]
    for mname in ("far", "touch", "overlap1"):
        assert cs.spec_direct(centre, radius, *cs.MAPS[mname](centre)) == (mname != "overlap1")
    with vr.Renderer(0) as rr:
        assert rr.get_option("blur_scratch_kib") == 0
        rr.set_volume(base)
        vol = base
        for mname in ("far", "touch"):
            clone(rr, "interior", mname, ps.SET, 1)
            vol = spec(vol, "interior", mname, ps.SET, 1)
            assert_exact(rr.get_volume(), vol)
            assert rr.get_option("blur_scratch_kib") == 0, mname      # direct: one launch, no scratch
        assert clone(rr, "miss", "push+x") is None
        assert clone(rr, "interior", "push+x", strength=(0, 0, 0, 0)) is not None
        assert rr.get_option("blur_scratch_kib") == 0                 # no launch, no scratch
        clone(rr, "interior", "overlap1", ps.SET, 1)
        vol = spec(vol, "interior", "overlap1", ps.SET, 1)
        assert_exact(rr.get_volume(), vol)
        assert rr.get_option("blur_scratch_kib") == 1024               # staged: the blur's scratch, rounded up to 1 MiB
        rr.set_option("blur_scratch_kib", 0)
        assert rr.get_option("blur_scratch_kib") == 0
        rr.set_option("blur_scratch_kib", 2000)                        # a reserve serves all three
        assert rr.get_option("blur_scratch_kib") == 2048
        vol = ms.morph_volume()                                        # a blur and a morph want a smoother input
        rr.set_volume(vol)
        clone(rr, "whole", "mirror_xyz", ps.ADD, 1, FULL)
        vol = spec(vol, "whole", "mirror_xyz", ps.ADD, 1, FULL)
        assert_exact(rr.get_volume(), vol)
        rr.blur(*ps.BRUSHES["whole"], 2, 1, FULL)
        vol = bs.spec_blur(vol, *ps.BRUSHES["whole"], 2, 1, FULL)
        assert_exact(rr.get_volume(), vol)
        rr.morph(*ps.BRUSHES["straddle"], ms.DILATE, 1, 0, FULL)
        vol = ms.spec_morph(vol, *ps.BRUSHES["straddle"], ms.DILATE, 1, 0, FULL)
        assert_exact(rr.get_volume(), vol)
        clone(rr, "max", "push-z", ps.SET, 0, FULL)
        assert_exact(rr.get_volume(), spec(vol, "max", "push-z", ps.SET, 0, FULL))
        assert rr.get_option("blur_scratch_kib") == 2048


# ---- 4. stamps ---------------------------------------------------------------------------------
def test_copy_and_paste_with_a_soft_edge(r, base):
    """A box read with get_volume_box on the device and stamped elsewhere, for every op and falloff."""
    r.set_layout_preference(14)
    centre, radius = ps.BRUSHES["interior"]
    src_origin, extent = (2, 13, 30), (9, 7, 11)
    origin = (13, 8, 18)                                               # the placement holds the brush's box
    x, y, z = src_origin
    cut = np.ascontiguousarray(base[z:z + extent[2], y:y + extent[1], x:x + extent[0]])
    for op, _ in ps.OPS:
        for falloff, _ in ps.FALLOFFS:
            r.set_volume(base)
            saved = r.get_volume_box(src_origin, extent, stream=torch.cuda.current_stream())
            assert saved.is_cuda and np.array_equal(saved.cpu().numpy(), cut)
            assert r.stamp(saved, origin, centre, radius, op, falloff, cs.STRENGTH) == ps.spec_box(centre, radius)
            want = cs.spec_stamp(base, cut, origin, centre, radius, op, falloff)
            assert (want != base).any()
            assert_exact(r.get_volume(), want)
            assert_exact(vr.brush_stamp_apply(vr.make_brush(centre, radius, op, falloff, 0, cs.STRENGTH), cut, origin, base.copy()), want)


@pytest.mark.parametrize("sname", list(cs.STAMPS))
def test_stamp_placements(r, base, sname):
    """Placements that hang over two faces, are smaller than the brush, miss it, lie at the ends of int32; a
    1 x 1 x 1 stamp; the whole volume."""
    bname, extent, origin = cs.STAMPS[sname]
    centre, radius = ps.BRUSHES[bname]
    stamp = cs.stamp_bytes(extent)
    d_stamp = torch.from_numpy(stamp).cuda()
    want_box = cs.spec_stamp_box(centre, radius, origin, extent)
    assert (want_box is None) == (sname in ("miss", "outside"))
    r.set_layout_preference(14)
    for op, _ in ps.OPS:
        for falloff, _ in ps.FALLOFFS:
            r.set_volume(base)
            assert r.stamp(d_stamp, origin, centre, radius, op, falloff, cs.STRENGTH) == want_box
            assert vr.stamp_box(vr.make_brush(centre, radius), (origin, extent), DIMS) == want_box
            want = cs.spec_stamp(base, stamp, origin, centre, radius, op, falloff)
            assert (want != base).any() == (want_box is not None)
            assert_exact(r.get_volume(), want)


def test_a_misaligned_stamp_is_refused(r, base):
    r.set_layout_preference(0)
    r.set_volume(base)
    centre, radius = ps.BRUSHES["interior"]
    flat = torch.zeros(3 * 3 * 3 * 4 + 4, dtype=torch.uint8, device="cuda")
    assert flat.data_ptr() % 4 == 0
    for shift in (1, 2, 3):
        view = flat[shift:shift + 108].view(3, 3, 3, 4)
        assert view.is_contiguous() and view.data_ptr() % 4 == shift
        with pytest.raises(vr.VRError) as e:
            r.stamp(view, (16, 10, 22), centre, radius)
        assert e.value.status == 1 and "vr_stamp" in str(e.value) and "aligned" in str(e.value)
        assert np.array_equal(r.get_volume(), base)
    assert r.stamp(flat[4:].view(3, 3, 3, 4), (16, 10, 22), centre, radius) == ((16, 10, 22), (3, 3, 3))
    assert (r.get_volume()[22:25, 10:13, 16:19, :] == 0).any()


def test_feathered_undo(r, base):
    """Paint, then stamp the saved box back through a hard full-strength brush that covers it: the box is
    restored; through a smooth one, the centre is restored and the rim keeps some paint."""
    r.set_layout_preference(14)
    r.set_volume(base)
    centre, radius = ps.BRUSHES["interior"]
    origin, extent = ps.spec_box(centre, radius)
    saved = r.get_volume_box(origin, extent, stream=torch.cuda.current_stream())
    r.paint(centre, radius, ps.ADD, 1, (90, 90, 90, 90), FULL)
    painted = ps.spec_apply(base, centre, radius, ps.ADD, 1, (90,) * 4, FULL)
    assert_exact(r.get_volume(), painted)
    cover = tuple(2 * v for v in radius)                               # an ellipsoid that holds the whole box
    inside, _ = ps.spec_weights(base.shape[:3], centre, cover, 0)
    (x, y, z), (ex, ey, ez) = origin, extent
    assert inside[z:z + ez, y:y + ey, x:x + ex].all()
    assert r.stamp(saved, origin, centre, radius, ps.SET, 1, FULL) == (origin, extent)
    soft = cs.spec_stamp(painted, saved.cpu().numpy(), origin, centre, radius, ps.SET, 1, FULL)
    assert_exact(r.get_volume(), soft)
    assert (soft[centre[2], centre[1], centre[0]] == base[centre[2], centre[1], centre[0]]).all()
    assert (soft != base).any() and (soft != painted).any()
    assert r.stamp(saved, origin, centre, cover, ps.SET, 0, FULL) == (origin, extent)
    assert_exact(r.get_volume(), base)


# ---- 5. the edited context renders what a fresh install of the specification's volume renders --
@pytest.mark.parametrize("pref,lname", LAYOUTS, ids=LAYOUT_IDS)
def test_edited_render_equals_fresh_install(r, fresh, oracle, base, pref, lname):
    """A staged clone, a direct clone and a stamp, one after the other."""
    setup(r, pref, base)
    assert_marches(r, lname)
    stamp = cs.stamp_bytes((20, 12, 9), seed=5)
    d_stamp = torch.from_numpy(stamp).cuda()
    s_centre, s_radius = ps.BRUSHES["straddle"]
    edits = [
        (lambda: clone(r, "whole", "mirror_x", ps.SET, 1, FULL), lambda v: spec(v, "whole", "mirror_x", ps.SET, 1, FULL), False),
        (lambda: clone(r, "corner", "far", ps.ADD, 0, FULL), lambda v: spec(v, "corner", "far", ps.ADD, 0, FULL), True),
        (lambda: r.stamp(d_stamp, (10, 5, 28), s_centre, s_radius, ps.SET, 1, FULL),
         lambda v: cs.spec_stamp(v, stamp, (10, 5, 28), s_centre, s_radius, ps.SET, 1, FULL), None),
    ]
    assert not cs.spec_direct(*ps.BRUSHES["whole"], *cs.MAPS["mirror_x"](ps.BRUSHES["whole"][0]))
    assert cs.spec_direct(*ps.BRUSHES["corner"], *cs.MAPS["far"](ps.BRUSHES["corner"][0]))
    vol = base
    for apply, restate, _ in edits:
        before, _ = oracle_frame(oracle, vol)
        vol = restate(vol)
        ref, ref_steps = oracle_frame(oracle, vol)
        assert (ref != before).any(), "the edit does not change the oracle's frame"
        assert apply() is not None
        assert_marches(r, lname)
        img, steps = check_frame(r, oracle, vol)
        check_fresh_install(fresh, pref, lname, vol, img, steps)


# ---- 6. one stream, no host wait ---------------------------------------------------------------
@pytest.mark.parametrize("pref,lname", LAYOUTS, ids=LAYOUT_IDS)
def test_pick_clone_footprint_rerender_on_a_side_stream(r, oracle, base, pref, lname):
    """pick (which returns the texel to the host), then clone, update_footprint and render_rect queued on a side
    stream with one synchronise at the end: the patched frame is the whole frame of the specification's volume.
    A push by two texels under the picked pixel -- a staged clone, within a reserved scratch."""
    density = 32.0   # dense enough for rays to pass the 0.5 transmittance threshold (a hit)
    setup(r, pref, base, density=density)
    r.set_option("blur_scratch_kib", 1024)
    assert_marches(r, lname)
    rec = vr.ray_records(r.query_rect((0, 0, W, H), W, H, 0.5))
    hits = np.argwhere(rec["hit_step"] >= 0)
    assert len(hits) > 0, "no ray has a hit"
    py, px = (int(v) for v in hits[np.argmin(((hits - (H // 2, W // 2)) ** 2).sum(axis=1))])
    one, texel = r.pick(px, py, W, H, 0.5)
    assert one["hit_step"] >= 0 and texel is not None
    buf = r.render(W, H, FMT_RGBA32F)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    box = r.clone(texel, (4, 4, 4), (2, 0, -1), (0, 0, 0), ps.SET, 0, FULL, stream=s)
    assert box is not None
    rect = r.update_footprint(box[0], box[1], W, H)
    r.render_rect(buf, rect, FMT_RGBA32F, stream=s)
    s.synchronize()
    assert r.get_option("blur_scratch_kib") == 1024
    pushed = cs.spec_clone(base, texel, (4, 4, 4), (2, 0, -1), (0, 0, 0), ps.SET, 0, FULL)
    assert_exact(r.get_volume(), pushed)
    want, want_steps = oracle_frame(oracle, pushed, density=density)
    before, _ = oracle_frame(oracle, base, density=density)
    assert (want != before).any(), "the clone does not change the frame"
    assert_exact(buf.cpu().numpy(), want)
    img, steps = frame(r)
    assert_exact(img, want)
    assert steps == want_steps


# ---- 7. uniform channels on the recipe volume --------------------------------------------------


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
    # SET clones of all four channels, direct and staged, cannot break G
    for offset, mirror in (((14, 0, 0), (0, 0, 0)), ((1, -1, 2), (0, 0, 0)), ((30, 0, 0), (1, 0, 0))):
        r.clone(centre, radius, offset, mirror, ps.SET, 1, FULL)
        new = cs.spec_clone(vol, centre, radius, offset, mirror, ps.SET, 1, FULL)
        assert (new != vol).any() and (new[..., 1] == g).all()
        vol = new
    check_uniform(r, fresh, oracle, pref, lname, vol, True)
    # an ADD clone changes G where it is painted: the bit goes before the next render
    setup(r, pref, vol)
    assert r.get_option("uniform_mask") & 2
    r.clone(centre, radius, (14, 0, 0), (0, 0, 0), ps.ADD, 1, FULL)
    added = cs.spec_clone(vol, centre, radius, (14, 0, 0), (0, 0, 0), ps.ADD, 1, FULL)
    assert len(np.unique(added[..., 1])) > 1
    check_uniform(r, fresh, oracle, pref, lname, added, False)
    assert_marches(r, lname)
    # a stamp that changes G loses the bit too; one that leaves G alone (strength 0) keeps it
    setup(r, pref, vol)
    stamp = cs.stamp_bytes((13, 11, 15), seed=9)
    d_stamp = torch.from_numpy(stamp).cuda()
    origin = (9, 12, 7)
    r.stamp(d_stamp, origin, centre, radius, ps.SET, 1, (255, 0, 255, 255))
    kept = cs.spec_stamp(vol, stamp, origin, centre, radius, ps.SET, 1, (255, 0, 255, 255))
    assert (kept != vol).any() and (kept[..., 1] == g).all()
    check_uniform(r, fresh, oracle, pref, lname, kept, True)
    setup(r, pref, vol)
    r.stamp(d_stamp, origin, centre, radius, ps.SET, 1, FULL)
    stamped = cs.spec_stamp(vol, stamp, origin, centre, radius, ps.SET, 1, FULL)
    assert len(np.unique(stamped[..., 1])) > 1
    check_uniform(r, fresh, oracle, pref, lname, stamped, False)
    assert_marches(r, lname)


# ---- 8. refusals -------------------------------------------------------------------------------
def test_refusals(r, base):
    setup(r, 0, base)
    good = dict(centre=(17, 11, 23), radius=(3, 2, 4), offset=(1, 0, 0))
    d_stamp = torch.zeros((3, 3, 3, 4), dtype=torch.uint8, device="cuda")
    sgood = dict(stamp_tensor=d_stamp, placement_origin=(16, 10, 22), centre=(17, 11, 23), radius=(3, 2, 4))
    bad = [dict(good, mirror=(2, 0, 0)), dict(good, mirror=(0, -1, 0)), dict(good, mirror=(0, 0, 2**31 - 1)),
           dict(good, falloff=2), dict(good, op=3), dict(good, op=-1), dict(good, radius=(3, 256, 4)),
           dict(good, radius=(-1, 2, 4))]
    for kw in bad:
        with pytest.raises(vr.VRError) as e:
            r.clone(**kw)
        assert e.value.status == 1 and "vr_clone" in str(e.value), kw   # VR_ERR_INVALID
        assert np.array_equal(r.get_volume(), base)
    for kw in (dict(sgood, falloff=2), dict(sgood, op=3), dict(sgood, radius=(3, 256, 4)), dict(sgood, radius=(3, 2, -4)),
               dict(sgood, stamp_tensor=d_stamp[:0])):
        with pytest.raises(vr.VRError) as e:
            r.stamp(**kw)
        assert e.value.status == 1 and "vr_stamp" in str(e.value), kw
        assert np.array_equal(r.get_volume(), base)
    for bad_tensor in (d_stamp.cpu(), d_stamp.to(torch.int8), d_stamp[:, :, :, :3], d_stamp[:, ::2]):
        with pytest.raises(ValueError):
            r.stamp(**dict(sgood, stamp_tensor=bad_tensor))
    b, m, box = vr.make_brush((17, 11, 23), (3, 2, 4)), vr.make_clone_map((1, 0, 0)), _lib.Box(16, 10, 22, 3, 3, 3)
    ptr = ctypes.c_void_p(d_stamp.data_ptr())
    for k in range(2):
        bb, mm = vr.make_brush((17, 11, 23), (3, 2, 4)), vr.make_clone_map((1, 0, 0))
        bb.reserved[k] = 7
        mm.reserved[k] = 7
        for args in (("vr_clone", r._ctx, ctypes.byref(bb), ctypes.byref(m), None), ("vr_clone", r._ctx, ctypes.byref(b), ctypes.byref(mm), None),
                     ("vr_stamp", r._ctx, ctypes.byref(bb), ptr, ctypes.byref(box), None)):
            with pytest.raises(vr.VRError) as e:
                _lib.call(*args)
            assert e.value.status == 1
    for args in (("vr_clone", r._ctx, None, ctypes.byref(m), None), ("vr_clone", r._ctx, ctypes.byref(b), None, None),
                 ("vr_stamp", r._ctx, None, ptr, ctypes.byref(box), None), ("vr_stamp", r._ctx, ctypes.byref(b), None, ctypes.byref(box), None),
                 ("vr_stamp", r._ctx, ctypes.byref(b), ptr, None, None)):
        with pytest.raises(vr.VRError) as e:
            _lib.call(*args)
        assert e.value.status == 1 and "null" in str(e.value)
    assert np.array_equal(r.get_volume(), base)
    assert r.clone((-10, -10, -10), (4, 4, 4), (1, 0, 0)) is None       # a miss is VR_OK
    assert r.clone(strength=(0, 0, 0, 0), **good) is not None           # nothing to do is VR_OK too
    assert r.stamp(strength=(0, 0, 0, 0), **sgood) is not None
    assert r.stamp(**dict(sgood, placement_origin=(30, 10, 22))) is None
    assert np.array_equal(r.get_volume(), base)
    check_needs_a_volume(r, lambda rr: rr.clone(**good), lambda rr: rr.stamp(**sgood))
    assert np.array_equal(r.get_volume(), base)
