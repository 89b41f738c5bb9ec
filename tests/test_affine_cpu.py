"""The transform paste's host side, the checks that need no GPU:
vr_brush_stamp_affine_apply and vr_brush_clone_affine_apply against the numpy
restatement (tests/affine_spec.py) for every brush x map x filter x op x
falloff; the maps that vr_clone and vr_stamp can express, against those; a
quarter turn against np.rot90; uniform channels under the trilinear filter;
refusals; the map builders; the direct / staged rule against brute force.
Everything is exact."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affine_spec as af  # noqa: E402
import clone_spec as cs  # noqa: E402
import paint_spec as ps  # noqa: E402
from brush_harness import assert_exact, base  # noqa: E402,F401

DIMS = (ps.NX, ps.NY, ps.NZ)
VOLUME_BRUSHES = ["interior", "texel", "corner", "outside_centre", "straddle", "whole", "max", "miss"]


def brush(centre, radius, op=ps.SET, falloff=0, strength=af.STRENGTH):
    import volumetricrenderer_amd as vr
    return vr.make_brush(centre, radius, op, falloff, (1, 2, 3, 4), strength)


def affine(table, filt=af.NEAREST, border=af.CLAMP):
    import volumetricrenderer_amd as vr
    return vr.make_affine(*table, filt, border)


@pytest.fixture(scope="module")
def stamp():
    return af.stamp_bytes()


# ---- 1. the host statements are the numpy restatement's ---------------------------------------
@pytest.mark.parametrize("mname", list(af.MAPS))
@pytest.mark.parametrize("name", VOLUME_BRUSHES)
def test_apply_matches_the_numpy_restatement(base, stamp, name, mname):
    import volumetricrenderer_amd as vr
    centre, radius = ps.BRUSHES[name]
    changed = False
    for src, table in ((None, af.MAPS[mname](centre, centre)), (stamp, af.MAPS[mname](centre, af.STAMP_CENTRE))):
        for filt, _ in af.FILTERS:
            sampled = af.sample(base if src is None else src, table, filt, base.shape[:3])
            for border in af.BORDERS[mname]:
                for (op, _), (falloff, _) in itertools.product(ps.OPS, ps.FALLOFFS):
                    want = af.spec_affine(base, src, table, filt, border, centre, radius, op, falloff, sampled=sampled)
                    b, a = brush(centre, radius, op, falloff), affine(table, filt, border)
                    got = (vr.brush_clone_affine_apply(b, a, base.copy()) if src is None
                           else vr.brush_stamp_affine_apply(b, src, a, base.copy()))
                    assert_exact(got, want)
                    assert (got[..., 3] == base[..., 3]).all()        # strength 0: never written
                    changed = changed or (want != base).any()
    assert changed == (name != "miss")


def test_the_maps_tell_wrong_implementations_apart(base):
    """Asserted of the restatement alone: the half-texel shift differs between the filters and from both whole
    shifts next to it; off_source leaves about half of the box outside; SKIP and CLAMP differ there."""
    centre, radius = ps.BRUSHES["whole"]
    t = af.MAPS["shift_half"](centre, centre)
    near = af.spec_affine(base, None, t, af.NEAREST, af.CLAMP, centre, radius, ps.SET, 0, af.FULL)
    lin = af.spec_affine(base, None, t, af.LINEAR, af.CLAMP, centre, radius, ps.SET, 0, af.FULL)
    assert (near != lin).mean() > 0.5
    for shift in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0)):
        whole = cs.spec_clone(base, centre, radius, shift, (0, 0, 0), ps.SET, 0, af.FULL)
        assert (whole != lin).mean() > 0.5
    assert_exact(near, cs.spec_clone(base, centre, radius, (1, 0, 0), (0, 0, 0), ps.SET, 0, af.FULL))   # 0x8000 rounds up, 0x4000 down
    t = af.MAPS["off_source"](centre, centre)
    _, outside = af.sample(base, t, af.LINEAR, base.shape[:3])
    assert 0.4 < outside.mean() < 0.6
    clamp = af.spec_affine(base, None, t, af.LINEAR, af.CLAMP, centre, radius, ps.SET, 0, af.FULL)
    skip = af.spec_affine(base, None, t, af.LINEAR, af.SKIP, centre, radius, ps.SET, 0, af.FULL)
    assert (clamp != skip).any() and (skip[outside] == base[outside]).all()


# ---- 2, 3. what vr_clone can express ------------------------------------------------------------
@pytest.mark.parametrize("name", VOLUME_BRUSHES)
def test_translations_and_the_mirror_equal_vr_clone(base, name):
    import volumetricrenderer_amd as vr
    centre, radius = ps.BRUSHES[name]
    cases = [("identity", (0, 0, 0), (0, 0, 0)), ("shift_int", (5, -3, 7), (0, 0, 0)), ("flip", (2 * centre[0], 0, 0), (1, 0, 0))]
    for mname, offset, mirror in cases:
        table = af.MAPS[mname](centre, centre)
        for (filt, _), (op, _), (falloff, _) in itertools.product(af.FILTERS, ps.OPS, ps.FALLOFFS):
            b = brush(centre, radius, op, falloff)
            want = vr.brush_clone_apply(b, vr.make_clone_map(offset, mirror), base.copy())
            assert_exact(vr.brush_clone_affine_apply(b, affine(table, filt), base.copy()), want)


# ---- 4. what vr_stamp can express ---------------------------------------------------------------
@pytest.mark.parametrize("sname", ["covers", "two_faces", "far_faces", "smaller", "one", "max"])
def test_the_identity_stamp_equals_vr_stamp_inside_the_placement(base, sname):
    """pivot = the placement origin, origin = 0: stamp texel (i, j, k) lies on texel placement + (i, j, k).  With
    VR_BORDER_SKIP the texels outside the placement are left alone, as vr_stamp leaves them."""
    import volumetricrenderer_amd as vr
    bname, extent, origin = cs.STAMPS[sname]
    centre, radius = ps.BRUSHES[bname]
    src = cs.stamp_bytes(extent)
    for (filt, _), (op, _), (falloff, _) in itertools.product(af.FILTERS, ps.OPS, ps.FALLOFFS):
        b = brush(centre, radius, op, falloff)
        want = vr.brush_stamp_apply(b, src, origin, base.copy())
        assert (want != base).any()
        got = vr.brush_stamp_affine_apply(b, src, affine((af.I3, origin, (0, 0, 0)), filt, af.SKIP), base.copy())
        assert_exact(got, want)
        # CLAMP agrees inside the placement (outside it reads the stamp's edge instead)
        got = vr.brush_stamp_affine_apply(b, src, affine((af.I3, origin, (0, 0, 0)), filt, af.CLAMP), base.copy())
        (x, y, z), (bx, by, bz) = origin, extent
        sl = (slice(max(z, 0), z + bz), slice(max(y, 0), y + by), slice(max(x, 0), x + bx))
        assert_exact(got[sl], want[sl])


# ---- 5. a quarter turn ---------------------------------------------------------------------------
def test_a_quarter_turn_is_np_rot90(base):
    """m = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]: destination offset (dx, dy) reads source offset (-dy, dx).  A hard,
    full-strength SET brush that fills a 9 x 9 x 5 box, source block elsewhere in the volume."""
    import volumetricrenderer_amd as vr
    centre, src = (8, 10, 20), (25, 11, 30)
    fill = (40, 40, 40)                                              # an ellipsoid that holds the whole 9 x 9 x 5 box
    table = (((0, -65536, 0), (65536, 0, 0), (0, 0, 65536)), centre, tuple(v * 65536 for v in src))
    b = vr.make_brush(centre, fill, ps.SET, 0, 0, af.FULL)
    got = vr.brush_clone_affine_apply(b, affine(table), base.copy())
    block = base[src[2] - 2:src[2] + 3, src[1] - 4:src[1] + 5, src[0] - 4:src[0] + 5]
    # out[dy, dx] = block[dx, -dy]: a quarter turn in the (y, x) plane
    turned = np.rot90(block, k=1, axes=(1, 2))
    want = np.empty_like(block)
    for dy in range(-4, 5):
        for dx in range(-4, 5):
            want[:, dy + 4, dx + 4] = block[:, dx + 4, -dy + 4]
    assert (turned == want).all()
    assert_exact(got[centre[2] - 2:centre[2] + 3, centre[1] - 4:centre[1] + 5, centre[0] - 4:centre[0] + 5], turned)


# ---- 6. a uniform channel survives the trilinear filter -------------------------------------------
def test_linear_returns_the_byte_of_a_uniform_channel():
    import volumetricrenderer_amd as vr
    rng = np.random.default_rng(7)
    centre, radius = (4, 3, 2), (9, 9, 9)
    tables = [af.MAPS[n](centre, centre) for n in ("shift_half", "rot30_axis", "scale2", "shear", "collapse")]
    tables.append((af.I3, centre, (4 * 65536 + 0xFF00, 3 * 65536 + 0x0100, 2 * 65536 + 0x7F80)))
    for value in range(256):
        vol = rng.integers(0, 256, size=(5, 7, 9, 4), dtype=np.uint8)
        vol[..., 1] = value
        for table in tables:
            got = vr.brush_clone_affine_apply(vr.make_brush(centre, radius, ps.SET, 1, 0, af.FULL), affine(table, af.LINEAR), vol.copy())
            assert (got[..., 1] == value).all(), (value, table)
            assert (got != vol).any()


# ---- 7. refusals leave the array alone -----------------------------------------------------------
def test_refusals_leave_the_array_unchanged(base, stamp):
    import volumetricrenderer_amd as vr
    from volumetricrenderer_amd import _lib
    centre, radius = ps.BRUSHES["interior"]
    good_b, good_a = brush(centre, radius), affine(af.MAPS["rot30_axis"](centre, centre), af.LINEAR)
    vol = base.copy()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731

    def bad_maps():
        for k, v in (("filter", 2), ("filter", -1), ("border", 2), ("border", -1), ("reserved", 1)):
            a = affine(af.MAPS["identity"](centre, centre))
            setattr(a, k, v)
            yield a
        for v in (256 * 65536 + 1, -256 * 65536 - 1, 2**31 - 1, -2**31):
            a = affine(af.MAPS["identity"](centre, centre))
            a.m[1][2] = v
            yield a

    def bad_brushes():
        for kw in (dict(op=3), dict(op=-1), dict(falloff=2)):
            yield brush(centre, radius, **kw)
        for r in ((3, 256, 4), (-1, 2, 4)):
            yield brush(centre, r)
        for k in range(2):
            b = brush(centre, radius)
            b.reserved[k] = 7
            yield b

    calls = []
    for a in bad_maps():
        calls.append((good_b, a, DIMS, af.STAMP_EXTENT))
    for b in bad_brushes():
        calls.append((b, good_a, DIMS, af.STAMP_EXTENT))
    for dims in ((0, ps.NY, ps.NZ), (ps.NX, -1, ps.NZ), (ps.NX, ps.NY, 0)):
        calls.append((good_b, good_a, dims, af.STAMP_EXTENT))
    for b, a, dims, ext in calls:
        for args in (("vr_brush_clone_affine_apply", ctypes.byref(b), ctypes.byref(a), vp(vol), *dims),
                     ("vr_brush_stamp_affine_apply", ctypes.byref(b), vp(stamp), *ext, ctypes.byref(a), vp(vol), *dims)):
            with pytest.raises(vr.VRError) as e:
                _lib.call(*args)
            assert e.value.status == 1 and args[0] in str(e.value)
            assert np.array_equal(vol, base)
    for ext in ((0, 9, 11), (13, -1, 11), (13, 9, 32769)):
        with pytest.raises(vr.VRError) as e:
            _lib.call("vr_brush_stamp_affine_apply", ctypes.byref(good_b), vp(stamp), *ext, ctypes.byref(good_a), vp(vol), *DIMS)
        assert e.value.status == 1 and "extent" in str(e.value)
    for args in (("vr_brush_clone_affine_apply", None, ctypes.byref(good_a), vp(vol), *DIMS),
                 ("vr_brush_clone_affine_apply", ctypes.byref(good_b), None, vp(vol), *DIMS),
                 ("vr_brush_clone_affine_apply", ctypes.byref(good_b), ctypes.byref(good_a), None, *DIMS),
                 ("vr_brush_stamp_affine_apply", ctypes.byref(good_b), None, *af.STAMP_EXTENT, ctypes.byref(good_a), vp(vol), *DIMS),
                 ("vr_brush_stamp_affine_apply", ctypes.byref(good_b), vp(stamp), *af.STAMP_EXTENT, None, vp(vol), *DIMS),
                 ("vr_brush_stamp_affine_apply", ctypes.byref(good_b), vp(stamp), *af.STAMP_EXTENT, ctypes.byref(good_a), None, *DIMS)):
        with pytest.raises(vr.VRError) as e:
            _lib.call(*args)
        assert e.value.status == 1 and "null" in str(e.value)
    assert np.array_equal(vol, base)
    # the largest legal coefficient and pivots at the ends of int32 are accepted
    a = affine((((256 * 65536, 0, 0), (0, -256 * 65536, 0), (0, 0, 65536)), (2**31 - 1, -2**31, 0), (-2**31, 2**31 - 1, 0)), af.LINEAR)
    want = af.spec_affine(base, None, (tuple(tuple(r) for r in a.m), tuple(a.pivot), tuple(a.origin)), af.LINEAR, af.CLAMP,
                          centre, radius, ps.SET, 0)
    assert_exact(vr.brush_clone_affine_apply(good_b, a, base.copy()), want)


def test_texels_outside_the_source_are_untouched_under_skip(base, stamp):
    import volumetricrenderer_amd as vr
    centre, radius = ps.BRUSHES["whole"]
    for mname in ("off_source", "shift_int", "rot30_axis"):
        table = af.MAPS[mname](centre, af.STAMP_CENTRE)
        for filt, _ in af.FILTERS:
            _, outside = af.sample(stamp, table, filt, base.shape[:3])
            assert outside.any() and not outside.all()
            got = vr.brush_stamp_affine_apply(vr.make_brush(centre, radius, ps.ADD, 1, 0, af.FULL), stamp,
                                              affine(table, filt, af.SKIP), base.copy())
            assert (got[outside] == base[outside]).all()
            assert (got[~outside] != base[~outside]).any()


# ---- 8. the builders -----------------------------------------------------------------------------
def table_of(a):
    return [[list(r) for r in a.m], list(a.pivot), list(a.origin), a.filter, a.border, a.reserved]


def test_affine_identity_and_place():
    import volumetricrenderer_amd as vr
    eye = [[65536, 0, 0], [0, 65536, 0], [0, 0, 65536]]
    assert table_of(vr.affine_identity()) == [eye, [0, 0, 0], [0, 0, 0], af.NEAREST, af.CLAMP, 0]
    a = vr.affine_place(np.eye(3), (1.5, -2.25, 3), (7, -8, 2**31 - 1), af.LINEAR, af.SKIP)
    assert table_of(a) == [eye, [7, -8, 2**31 - 1], [98304, -147456, 196608], af.LINEAR, af.SKIP, 0]
    # the 24 rotations of the cube: signed permutation matrices of determinant +1; the inverse is the transpose
    count = 0
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1, -1), repeat=3):
            f = np.zeros((3, 3))
            for r in range(3):
                f[r, perm[r]] = signs[r]
            if round(np.linalg.det(f)) != 1:
                continue
            count += 1
            assert table_of(vr.affine_place(f, (0, 0, 0), (0, 0, 0)))[0] == (f.T * 65536).astype(int).tolist()
    assert count == 24
    assert table_of(vr.affine_place(np.eye(3) * 2, (0, 0, 0), (0, 0, 0)))[0] == [[32768, 0, 0], [0, 32768, 0], [0, 0, 32768]]
    assert table_of(vr.affine_place(np.eye(3) * 0.5, (0, 0, 0), (0, 0, 0)))[0] == [[131072, 0, 0], [0, 131072, 0], [0, 0, 131072]]
    assert table_of(vr.affine_place(np.eye(3) / 256, (0, 0, 0), (0, 0, 0)))[0][0][0] == 256 * 65536   # the largest coefficient
    # a rotation by 30 degrees: within one unit of numpy's inverse, and of the table the suite spells out
    R = af.rot30()
    got = np.array(table_of(vr.affine_place(R, (0, 0, 0), (0, 0, 0)))[0])
    assert np.abs(got - np.rint(np.linalg.inv(R) * 65536)).max() <= 1
    assert np.abs(got - np.array(af.MAPS["rot30_axis"]((0, 0, 0), (0, 0, 0))[0])).max() <= 1


def test_affine_place_refusals():
    import volumetricrenderer_amd as vr
    sentinel = vr.make_affine(((1, 2, 3), (4, 5, 6), (7, 8, 9)), (10, 11, 12), (13, 14, 15), 1, 1)
    singular = [np.zeros((3, 3)), np.ones((3, 3)), np.diag([1.0, 1.0, 0.0]), np.array([[1, 2, 3], [2, 4, 6], [0, 1, 0.0]]),
                np.diag([1e6, 1e6, 1e-7])]
    nonfinite = [np.diag([np.nan, 1, 1]), np.diag([1, np.inf, 1]), np.array([[1, 0, 0], [0, 1, -np.inf], [0, 0, 1.0]])]
    too_large = [np.eye(3) / 257, np.diag([1, 1, 1 / 256.01])]
    from volumetricrenderer_amd import _lib
    for f in singular + nonfinite + too_large:
        for src in ((0, 0, 0),):
            with pytest.raises(vr.VRError) as e:
                vr.affine_place(f, src, (0, 0, 0))
            assert e.value.status == 1 and "vr_affine_place" in str(e.value)
    for src in ((32768.0, 0, 0), (0, -40000.0, 0), (0, 0, np.nan), (np.inf, 0, 0)):
        with pytest.raises(vr.VRError):
            vr.affine_place(np.eye(3), src, (0, 0, 0))
    for filt, border in ((2, 0), (-1, 0), (0, 2), (0, -1)):
        with pytest.raises(vr.VRError):
            vr.affine_place(np.eye(3), (0, 0, 0), (0, 0, 0), filt, border)
    # *out is written only on success
    f = (ctypes.c_double * 9)(*np.zeros(9))
    z, d = (ctypes.c_double * 3)(), (ctypes.c_int32 * 3)()
    before = bytes(sentinel)
    with pytest.raises(vr.VRError):
        _lib.call("vr_affine_place", f, z, d, 0, 0, ctypes.byref(sentinel))
    assert bytes(sentinel) == before
    for args in ((None, z, d, 0, 0, ctypes.byref(sentinel)), (f, None, d, 0, 0, ctypes.byref(sentinel)),
                 (f, z, None, 0, 0, ctypes.byref(sentinel)), (f, z, d, 0, 0, None)):
        with pytest.raises(vr.VRError) as e:
            _lib.call("vr_affine_place", *args)
        assert "null" in str(e.value)
    with pytest.raises(vr.VRError):
        _lib.call("vr_affine_identity", None)
    assert vr.affine_place(np.eye(3), (32767.99, 0, 0), (0, 0, 0)).origin[0] == int(np.rint(32767.99 * 65536))


# ---- 9. the direct / staged rule -----------------------------------------------------------------
@pytest.mark.parametrize("mname", list(af.MAPS))
def test_path_rule_against_brute_force(mname):
    import volumetricrenderer_amd as vr
    some_direct = False
    for name, (centre, radius) in ps.BRUSHES.items():
        if name == "miss":
            assert not vr.affine_direct(brush(centre, radius), affine(af.MAPS[mname](centre, centre)), DIMS)
            continue
        table = af.MAPS[mname](centre, centre)
        for (filt, _), border in itertools.product(af.FILTERS, (af.CLAMP, af.SKIP)):
            direct = vr.affine_direct(brush(centre, radius), affine(table, filt, border), DIMS)
            assert direct == af.spec_direct(table, filt, centre, radius), (name, filt, border)
            if direct:
                assert not af.reads_a_written_texel(table, filt, border, centre, radius), (name, filt, border)
            some_direct = some_direct or direct
    centre, radius = ps.BRUSHES["interior"]
    for filt, _ in af.FILTERS:
        assert vr.affine_direct(brush(centre, radius), affine(af.MAPS["far"](centre, centre), filt), DIMS)
        assert not vr.affine_direct(brush(centre, radius), affine(af.MAPS["rot30_axis"](centre, centre), filt), DIMS)
    assert some_direct or mname not in ("far", "collapse")


def test_exports_and_struct_layout():
    from volumetricrenderer_amd import _lib
    assert ctypes.sizeof(_lib.Affine) == 72
    assert _lib.Affine.pivot.offset == 36 and _lib.Affine.origin.offset == 48 and _lib.Affine.filter.offset == 60
    lib = _lib.load()
    for name in ("vr_stamp_affine", "vr_clone_affine", "vr_brush_stamp_affine_apply", "vr_brush_clone_affine_apply",
                 "vr_affine_direct", "vr_affine_identity", "vr_affine_place"):
        assert hasattr(lib, name), name
    assert lib.vr_abi_version() == 2
