"""The liquify brush's host side, the checks that need no GPU:
vr_brush_warp_apply against the numpy restatement (tests/warp_spec.py) for
every brush x map x filter x border x falloff; the identity; falloff 0 against
vr_brush_clone_affine_apply; uniform channels; vr_warp_reach against brute
force; the push builder; refusals; and that the cases the GPU tests run reach
both device paths of a tile and the boundary between them.  Everything is
exact."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affine_spec as af  # noqa: E402
import paint_spec as ps  # noqa: E402
from brush_harness import assert_exact, base  # noqa: E402,F401
import warp_spec as ws  # noqa: E402

DIMS = (ps.NX, ps.NY, ps.NZ)


def brush(centre, radius, op=ps.SET, falloff=0, strength=ws.STRENGTH):
    import volumetricrenderer_amd as vr
    return vr.make_brush(centre, radius, op, falloff, (1, 2, 3, 4), strength)


def affine(table, filt=ws.NEAREST, border=ws.CLAMP):
    import volumetricrenderer_amd as vr
    return vr.make_affine(*table, filt, border)


# ---- 1. the host statement is the numpy restatement's -----------------------------------------
@pytest.mark.parametrize("mname", list(ws.MAPS))
@pytest.mark.parametrize("name", list(ps.BRUSHES))
def test_apply_matches_the_numpy_restatement(base, name, mname):
    import volumetricrenderer_amd as vr
    centre, radius = ps.BRUSHES[name]
    table = ws.placed(mname, centre)
    changed = False
    for (filt, _), (border, _), (falloff, _) in itertools.product(ws.FILTERS, ws.BORDERS, ps.FALLOFFS):
        want = ws.spec_warp(base, table, filt, border, centre, radius, falloff)
        got = vr.brush_warp_apply(brush(centre, radius, ps.SET, falloff), affine(table, filt, border), base.copy())
        assert_exact(got, want)
        assert (got[..., 3] == base[..., 3]).all()        # strength 0: never written
        changed = changed or (want != base).any()
    if name == "miss" or mname == "identity":
        assert not changed
    if name in ("interior", "straddle", "whole", "max") and mname != "identity":
        assert changed


def test_the_weight_shapes_the_displacement_not_the_mix(base):
    """Asserted of the restatement alone: a soft push differs from the hard one and from the soft transform paste (a
    cross-fade of the moved copy), and next to the rim it moves a texel by less than next to the centre."""
    centre, radius = ps.BRUSHES["straddle"]
    table = ws.placed("shift_int", centre)
    hard = ws.spec_warp(base, table, ws.LINEAR, ws.CLAMP, centre, radius, 0, ws.FULL)
    soft = ws.spec_warp(base, table, ws.LINEAR, ws.CLAMP, centre, radius, 1, ws.FULL)
    ghost = af.spec_affine(base, None, table, ws.LINEAR, ws.CLAMP, centre, radius, ps.SET, 1, ws.FULL)
    assert (hard != soft).any() and (soft != ghost).any()
    inside, w = ps.spec_weights(base.shape[:3], centre, radius, 1)
    P = ws.positions(table, base.shape[:3], w)
    x = np.arange(ps.NX, dtype=np.int64)[None, None, :] << 16
    moved = np.abs(P[0] - x)
    assert (inside & (w <= 32)).any()
    assert moved[inside & (w >= 250)].min() > moved[inside & (w <= 32)].max()
    assert (moved[~inside] == 0).all()


# ---- 2. the three identities ---------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ps.BRUSHES))
def test_the_identity_map_changes_nothing(base, name):
    import volumetricrenderer_amd as vr
    centre, radius = ps.BRUSHES[name]
    for (filt, _), (border, _), (falloff, _) in itertools.product(ws.FILTERS, ws.BORDERS, ps.FALLOFFS):
        for a in (affine(ws.placed("identity", centre), filt, border), vr.warp_push(centre, (0, 0, 0), filt, border)):
            assert_exact(vr.brush_warp_apply(brush(centre, radius, ps.SET, falloff, ws.FULL), a, base.copy()), base)


@pytest.mark.parametrize("mname", list(ws.MAPS))
def test_a_hard_warp_is_the_transform_paste(base, mname):
    import volumetricrenderer_amd as vr
    for name in ("interior", "corner", "outside_centre", "straddle", "whole"):
        centre, radius = ps.BRUSHES[name]
        for (filt, _), (border, _) in itertools.product(ws.FILTERS, ws.BORDERS):
            b, a = brush(centre, radius, ps.SET, 0), affine(ws.placed(mname, centre), filt, border)
            assert_exact(vr.brush_warp_apply(b, a, base.copy()), vr.brush_clone_affine_apply(b, a, base.copy()))


def test_a_constant_channel_stays_constant():
    import volumetricrenderer_amd as vr
    rng = np.random.default_rng(11)
    centre, radius = (4, 3, 2), (9, 9, 9)
    tables = [ws.placed(n, centre) for n in ("shift_half", "rot30_axis", "scale2", "shear", "collapse", "push_frac", "twirl20", "pinch")]
    for value in (0, 1, 127, 128, 254, 255):
        vol = rng.integers(0, 256, size=(5, 7, 9, 4), dtype=np.uint8)
        vol[..., 1] = value
        for table, (filt, _), (falloff, _) in itertools.product(tables, ws.FILTERS, ps.FALLOFFS):
            got = vr.brush_warp_apply(vr.make_brush(centre, radius, ps.SET, falloff, 0, ws.FULL), affine(table, filt), vol.copy())
            assert (got[..., 1] == value).all(), (value, table)
            assert (got != vol).any()


# ---- 3. the reach and the push -------------------------------------------------------------------
@pytest.mark.parametrize("mname", list(ws.MAPS))
def test_reach_against_brute_force(mname):
    """The corners bound |D| over every texel of the unclipped box, and some corner attains the bound."""
    import volumetricrenderer_amd as vr
    for name in ("interior", "texel", "corner", "outside_centre", "straddle"):
        centre, radius = ps.BRUSHES[name]
        table = ws.placed(mname, centre)
        m, pivot, origin = table
        got = vr.warp_reach(brush(centre, radius), affine(table))
        assert got == ws.spec_reach(table, centre, radius)
        t = [np.arange(c - r, c + r + 1, dtype=np.int64) for c, r in zip(centre, radius)]
        tx, ty, tz = t[0][None, None, :], t[1][None, :, None], t[2][:, None, None]
        for a in range(3):
            A = origin[a] + m[a][0] * (tx - pivot[0]) + m[a][1] * (ty - pivot[1]) + m[a][2] * (tz - pivot[2])
            assert int(np.abs(A - ((tx, ty, tz)[a] << 16)).max()) == got[a]


def test_reach_saturates_and_checks_its_arguments():
    import volumetricrenderer_amd as vr
    from volumetricrenderer_amd import _lib
    centre, radius = ps.BRUSHES["interior"]
    far = affine((af.I3, centre, (2**31 - 1, -2**31, 17 * 65536 + 5)))
    assert vr.warp_reach(brush(centre, radius), far) == (2**31 - 1 - (17 << 16), 2**31 - 1, abs(17 * 65536 + 5 - (23 << 16)))
    r = (ctypes.c_int32 * 3)()
    for args in ((None, ctypes.byref(far), r), (ctypes.byref(brush(centre, radius)), None, r),
                 (ctypes.byref(brush(centre, radius)), ctypes.byref(far), None)):
        with pytest.raises(vr.VRError) as e:
            _lib.call("vr_warp_reach", *args)
        assert e.value.status == 1 and "null" in str(e.value)
    bad = affine(ws.placed("identity", centre))
    bad.filter = 2
    with pytest.raises(vr.VRError):
        vr.warp_reach(brush(centre, radius), bad)
    assert vr.warp_reach(brush(centre, radius, ps.ADD), far)[1] == 2**31 - 1     # the op is vr_warp's business


def table_of(a):
    return [[list(r) for r in a.m], list(a.pivot), list(a.origin), a.filter, a.border, a.reserved]


def test_push_tables(base):
    import volumetricrenderer_amd as vr
    from volumetricrenderer_amd import _lib
    eye = [list(r) for r in af.I3]
    a = vr.warp_push((17, 11, 23), (0x18000, -0x8000, 0x4000), ws.LINEAR, ws.SKIP)
    assert table_of(a) == [eye, [17, 11, 23], [17 * 65536 - 0x18000, 11 * 65536 + 0x8000, 23 * 65536 - 0x4000], ws.LINEAR, ws.SKIP, 0]
    m, pivot, origin = ws.placed("push_frac", (17, 11, 23))
    assert table_of(a)[:3] == [[list(r) for r in m], list(pivot), list(origin)]
    assert table_of(vr.warp_push((-5, 0, 32767), (-65536, 0, 2**31 - 1)))[2] == [-4 * 65536, 0, 32767 * 65536 - (2**31 - 1)]
    # the content moves by +d: a hard whole push by (2, 0, -1) texels puts texel t - d on t
    centre, radius = ps.BRUSHES["whole"]
    got = vr.brush_warp_apply(vr.make_brush(centre, radius, ps.SET, 0, 0, ws.FULL), vr.warp_push(centre, (2 << 16, 0, -(1 << 16))), base.copy())
    assert_exact(got[:-1, :, 2:], base[1:, :, :-2])
    sentinel = affine(ws.placed("twirl20", (1, 2, 3)), 1, 1)
    before = bytes(sentinel)
    c3, d3 = (ctypes.c_int32 * 3)(32767, 0, 0), (ctypes.c_int32 * 3)(-65536, 0, 0)    # origin 2^31: outside int32
    for args in ((c3, d3, 1, 0), ((ctypes.c_int32 * 3)(-32768, 0, 0), (ctypes.c_int32 * 3)(1, 0, 0), 1, 0),
                 (c3, (ctypes.c_int32 * 3)(), 2, 0), (c3, (ctypes.c_int32 * 3)(), 0, -1)):
        with pytest.raises(vr.VRError) as e:
            _lib.call("vr_warp_push", *args, ctypes.byref(sentinel))
        assert e.value.status == 1 and "vr_warp_push" in str(e.value)
        assert bytes(sentinel) == before
    for args in ((None, d3, 0, 0, ctypes.byref(sentinel)), (c3, None, 0, 0, ctypes.byref(sentinel)), (c3, d3, 0, 0, None)):
        with pytest.raises(vr.VRError) as e:
            _lib.call("vr_warp_push", *args)
        assert "null" in str(e.value)
    assert vr.warp_push((32767, 0, 0), (1, 0, 0)).origin[0] == 2**31 - 65536 - 1


# ---- 4. refusals leave the array alone -----------------------------------------------------------
def limit_map(centre, over=0):
    """The identity pushed by exactly VR_WARP_MAX_DISP texels along x (plus `over` units of 1 / 65536)."""
    return (af.I3, centre, (centre[0] * 65536 - ws.MAX_DISP16 - over, centre[1] * 65536, centre[2] * 65536))


def test_refusals_leave_the_array_unchanged(base):
    import volumetricrenderer_amd as vr
    from volumetricrenderer_amd import _lib
    centre, radius = ps.BRUSHES["interior"]
    good_b, good_a = brush(centre, radius), affine(ws.placed("twirl20", centre), ws.LINEAR)
    vol = base.copy()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731

    def bad_maps():
        for k, v in (("filter", 2), ("filter", -1), ("border", 2), ("border", -1), ("reserved", 1)):
            a = affine(ws.placed("identity", centre))
            setattr(a, k, v)
            yield a
        for v in (256 * 65536 + 1, -256 * 65536 - 1, 2**31 - 1, -2**31):
            a = affine(ws.placed("identity", centre))
            a.m[1][2] = v
            yield a
        yield affine(limit_map(centre, 1))                                      # one unit above the limit
        # the other sign, on y: D_y = origin - pivot * 65536 = 1 + 2^31
        yield affine((af.I3, (centre[0], -32768, centre[2]), (centre[0] * 65536, 1, centre[2] * 65536)))

    def bad_brushes():
        for kw in (dict(op=ps.ADD), dict(op=ps.SUB), dict(op=3), dict(op=-1), dict(falloff=2)):
            yield brush(centre, radius, **kw)
        for r in ((3, 256, 4), (-1, 2, 4)):
            yield brush(centre, r)
        for k in range(2):
            b = brush(centre, radius)
            b.reserved[k] = 7
            yield b

    calls = [(good_b, a, DIMS) for a in bad_maps()] + [(b, good_a, DIMS) for b in bad_brushes()]
    calls += [(good_b, good_a, dims) for dims in ((0, ps.NY, ps.NZ), (ps.NX, -1, ps.NZ), (ps.NX, ps.NY, 0))]
    for b, a, dims in calls:
        with pytest.raises(vr.VRError) as e:
            _lib.call("vr_brush_warp_apply", ctypes.byref(b), ctypes.byref(a), vp(vol), *dims)
        assert e.value.status == 1 and "vr_brush_warp_apply" in str(e.value)
        assert np.array_equal(vol, base)
    for args in ((None, ctypes.byref(good_a), vp(vol)), (ctypes.byref(good_b), None, vp(vol)), (ctypes.byref(good_b), ctypes.byref(good_a), None)):
        with pytest.raises(vr.VRError) as e:
            _lib.call("vr_brush_warp_apply", *args, *DIMS)
        assert e.value.status == 1 and "null" in str(e.value)
    assert np.array_equal(vol, base)
    # exactly at the limit the map is accepted: every position is far outside the volume
    at = limit_map(centre)
    assert ws.spec_reach(at, centre, radius)[0] == ws.MAX_DISP16 and vr.warp_reach(good_b, affine(at))[0] == 2**31 - 1
    for border, _ in ws.BORDERS:
        want = ws.spec_warp(base, at, ws.LINEAR, border, centre, radius, 1)
        assert_exact(vr.brush_warp_apply(brush(centre, radius, ps.SET, 1), affine(at, ws.LINEAR, border), base.copy()), want)
        assert (want != base).any() == (border == ws.CLAMP)
    # the reach is taken over the UNCLIPPED box: a scale that is fine under a small brush is refused under a huge one
    grow = (((256 * 65536, 0, 0), (0, 65536, 0), (0, 0, 65536)), centre, af._at(centre))
    assert vr.brush_warp_apply(brush(centre, (128, 1, 1)), affine(grow), base.copy()) is not None    # 255 * 128 < 32768
    with pytest.raises(vr.VRError) as e:
        vr.brush_warp_apply(brush(centre, (129, 1, 1)), affine(grow), base.copy())                  # 255 * 129 > 32768
    assert "VR_WARP_MAX_DISP" in str(e.value)


# ---- 5. the GPU cases reach both paths of a tile and the boundary between them -------------------
def test_the_gpu_cases_cover_both_paths_and_the_boundary():
    small = large = 0
    for name, mname in itertools.product(("interior", "straddle", "whole"), ws.MAPS):
        centre, radius = ps.BRUSHES[name]
        for (filt, _), (falloff, _) in itertools.product(ws.FILTERS, ps.FALLOFFS):
            v = ws.volumes(ws.tile_footprint(ws.placed(mname, centre), filt, centre, radius, falloff))
            small += sum(1 for n in v if n <= ws.BUDGET)
            large += sum(1 for n in v if n > ws.BUDGET)
    assert small > 0 and large > 0
    centre, radius = ps.BRUSHES["whole"]
    exact = ws.volumes(ws.tile_footprint(ws.BUDGET_EXACT, ws.LINEAR, centre, radius, 0))
    assert max(exact) == ws.BUDGET and exact.count(ws.BUDGET) >= 1
    over = ws.tile_footprint(ws.BUDGET_OVER, ws.LINEAR, centre, radius, 0)
    assert (16, 17, 16) in over and min(n for n in ws.volumes(over) if n > ws.BUDGET) == ws.BUDGET + 256
    assert any(n <= ws.BUDGET for n in ws.volumes(over))
    # a tile SKIP leaves alone reads nothing; a brush that misses has no tile
    assert None in ws.tile_footprint(ws.placed("off_source", centre), ws.LINEAR, centre, radius, 0, border=ws.SKIP)
    assert ws.tile_footprint(ws.placed("pinch", (0, 0, 0)), ws.LINEAR, *ps.BRUSHES["miss"], 1) == []


def test_exports_and_struct_layout():
    from volumetricrenderer_amd import _lib
    assert ctypes.sizeof(_lib.Affine) == 72 and ctypes.sizeof(_lib.Brush) == 48
    assert _lib.Affine.pivot.offset == 36 and _lib.Affine.origin.offset == 48 and _lib.Affine.filter.offset == 60
    lib = _lib.load()
    for name in ("vr_warp", "vr_brush_warp_apply", "vr_warp_reach", "vr_warp_push"):
        assert hasattr(lib, name), name
    assert _lib.WARP_MAX_DISP == 32768 and lib.vr_abi_version() == 2
