"""vr_fill's host side, the checks that need no GPU: the conditions the shared
volumes must meet (a test must not pass vacuously); vr_brush_fill_apply against
the numpy restatement of the flood-fill brush (tests/fill_spec.py), bytes and
report, on every volume x brush of paint_spec.BRUSHES x op x falloff x relative
/ absolute, with selected channels that differ from the painted ones; the
snakes' corridors against the generator's lists; a seed that is not passable;
refusals; struct sizes, prototypes and exports.  Everything is exact."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fill_spec as fs  # noqa: E402
import paint_spec as ps  # noqa: E402
from brush_harness import assert_exact  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["blobs", "snakes", "detour", "edges"]


@pytest.fixture(scope="module")
def cases():
    return fs.cases()


def lib_rule(rule):
    import volumetricrenderer_amd as vr
    return vr.make_fill_rule(rule.seed, rule.lo, rule.hi, rule.select, rule.relative)


def brush(centre, radius, op=0, falloff=0, strength=fs.STRENGTH, value=fs.VALUE):
    import volumetricrenderer_amd as vr
    return vr.make_brush(centre, radius, op, falloff, value, strength)


def apply(vol, centre, radius, op, falloff, rule, strength=fs.STRENGTH):
    import volumetricrenderer_amd as vr
    got, rep = vr.brush_fill_apply(brush(centre, radius, op, falloff, strength), lib_rule(rule), vol.copy())
    return got, tuple(rep)


def rule_of(cases, cname, centre, relative, channel=None):
    case = cases[cname]
    if cname == "edges":
        return fs.edge_rule(case.vol, case.seed(centre))
    return case.rule(centre, relative, channel)


def test_the_volumes_tell_wrong_implementations_apart(cases):
    """Asserted before anything is compared with the library."""
    whole = ps.BRUSHES["whole"]
    # blobs: several components; the seed's holds 5..60 % of what passes, so "passable everywhere" is another answer
    case = cases["blobs"]
    passable, region, rep = fs.spec_region(case.vol, *whole, case.rule(whole[0], 0))
    print("blobs: region", rep[0], "of", rep[1])
    assert 0.05 * rep[1] < rep[0] < 0.60 * rep[1] and (passable & ~region).any()
    # snakes: each corridor is one region of more than 40 % of the passable texels, the two disjoint
    vol, a, b = fs.snakes()
    assert not set(a) & set(b) and len(set(a)) == len(a) and len(set(b)) == len(b)
    for path in (a, b):
        rule = fs.absolute_rule(path[len(path) // 3], fs.SNAKE_LO, fs.SNAKE_HI)
        passable, region, rep = fs.spec_region(vol, *whole, rule)
        print("snakes: region", rep[0], "of", rep[1])
        assert rep[0] == len(path) > 0.40 * rep[1] and rep[1] == len(a) + len(b)
        assert sorted(map(tuple, fs.texels_where(region).tolist())) == sorted(path)   # the dilation equals the list
        assert (passable & ~region).any()
    f = vol[..., 0]
    assert f.min() == fs.SNAKE_LO and (f == fs.SNAKE_HI).any() and (f[f > fs.SNAKE_HI] == fs.SNAKE_HI + 1).all()
    assert (vol[..., 3] == 255 - f.astype(np.int64)).all()
    # one `<` for `<=`, at either end, or one missed wall floods or starves the corridor
    for lo, hi in ((fs.SNAKE_LO, fs.SNAKE_HI + 1), (fs.SNAKE_LO + 1, fs.SNAKE_HI), (fs.SNAKE_LO, fs.SNAKE_HI - 1)):
        wrong = fs.spec_region(vol, *whole, fs.absolute_rule(a[len(a) // 3], lo, hi))[2]
        assert wrong[0] != len(a), (lo, hi)
    # the corridors cross the tiles' x and y faces many times and every z face, and a tile holds separate pieces of both
    pa = np.array(a)
    crossings = [int((np.diff(pa[:, k] // 8) != 0).sum()) for k in range(3)]
    assert crossings[0] > 20 and crossings[1] > 20 and crossings[2] == (ps.NZ - 1) // 8, crossings
    in_tile = [tuple(t) for t in pa.tolist() if t[0] < 8 and t[1] < 8 and t[2] < 8]
    assert len({t[2] for t in in_tile}) >= 4 and any(t[0] < 8 and t[1] < 8 and t[2] < 8 for t in b)
    # detour: the far part passes, is not reached under `interior`, and is reached once the brush holds the path
    case = cases["detour"]
    interior = ps.BRUSHES["interior"]
    passable, region, rep = fs.spec_region(case.vol, *interior, case.rule(interior[0], 1))
    far = [t for t in fs.DETOUR_PARTS[1] if passable[t[2], t[1], t[0]]]
    assert far and not any(region[t[2], t[1], t[0]] for t in far) and rep[0] > 0 and rep[1] > rep[0]
    assert all(region[t[2], t[1], t[0]] for t in fs.DETOUR_PARTS[0] if passable[t[2], t[1], t[0]])
    _, region_whole, _ = fs.spec_region(case.vol, *whole, case.rule(whole[0], 1))
    assert all(region_whole[t[2], t[1], t[0]] for t in fs.DETOUR_PARTS[0] + fs.DETOUR_PARTS[1])
    # edges: all three seed bytes occur as seeds of the brush list, and their ranges clamp
    case = cases["edges"]
    seeds = {int(case.vol[s[2], s[1], s[0], 0]) for s in (case.seed(c) for c, _ in ps.BRUSHES.values())}
    assert seeds == set(fs.EDGE_SEED_BYTES), seeds


@pytest.mark.parametrize("relative", [0, 1], ids=["absolute", "relative"])
@pytest.mark.parametrize("name", list(ps.BRUSHES))
@pytest.mark.parametrize("cname", CASES)
def test_fill_apply_matches_the_numpy_restatement(cases, cname, name, relative):
    vol = cases[cname].vol
    centre, radius = ps.BRUSHES[name]
    rule = rule_of(cases, cname, centre, relative)
    _, region, want_rep = fs.spec_region(vol, centre, radius, rule)
    for op, _ in ps.OPS:
        for falloff, _ in ps.FALLOFFS:
            want, _ = fs.spec_fill(vol, centre, radius, op, falloff, rule)
            got, rep = apply(vol, centre, radius, op, falloff, rule)
            assert rep == want_rep
            assert_exact(got, want)
            assert (want[~region] == vol[~region]).all() and (want[..., 3] == vol[..., 3]).all()
    if name in ("whole", "max") or (name, cname) in (("interior", "blobs"), ("interior", "snakes"), ("interior", "detour"),
                                                     ("corner", "blobs"), ("corner", "snakes"), ("corner", "edges")):
        assert want_rep[0] > 0, "nothing was filled where the brush holds the seed"
        assert (fs.spec_fill(vol, centre, radius, ps.SET, 0, rule)[0] != vol).any()
    if name == "miss":
        assert want_rep == fs.empty_report((ps.NX, ps.NY, ps.NZ))


@pytest.mark.parametrize("relative", [0, 1], ids=["absolute", "relative"])
@pytest.mark.parametrize("cname", ["blobs", "snakes", "detour"])
def test_the_selected_channel_need_not_be_painted(cases, cname, relative):
    """The rule on A, which STRENGTH never paints (and whose range is the mirrored one: the walls of the snakes lie
    one below it); and a rule on R and A together with only G painted."""
    vol = cases[cname].vol
    for name in ("whole", "interior"):
        centre, radius = ps.BRUSHES[name]
        on_a = rule_of(cases, cname, centre, relative, 3)
        on_r = rule_of(cases, cname, centre, relative, 0)
        assert on_a.select == (0, 0, 0, 1)
        assert fs.spec_region(vol, centre, radius, on_a)[2] == fs.spec_region(vol, centre, radius, on_r)[2]
        both = fs.Rule(on_r.seed, (on_r.lo[0], 0, 0, on_a.lo[3]), (on_r.hi[0], 0, 0, on_a.hi[3]), (1, 0, 0, 1), relative)
        for rule, strength in ((on_a, fs.STRENGTH), (both, (0, 255, 0, 0))):
            want, want_rep = fs.spec_fill(vol, centre, radius, ps.ADD, 1, rule, strength=strength)
            got, rep = apply(vol, centre, radius, ps.ADD, 1, rule, strength)
            assert rep == want_rep and rep[0] > 0
            assert_exact(got, want)
            assert (got != vol).any() and (got[..., 0] == vol[..., 0]).all() == (strength[0] == 0)


def test_each_corridor_fills_alone():
    vol, a, b = fs.snakes()
    centre, radius = ps.BRUSHES["whole"]
    for path, other in ((a, b), (b, a)):
        for seed in (path[0], path[-1], path[len(path) // 2]):
            rule = fs.relative_rule(vol, seed, fs.SNAKE_LO, fs.SNAKE_HI)
            got, rep = apply(vol, centre, radius, ps.SET, 0, rule, fs.FULL)
            assert rep[0] == len(path) and rep[1] == len(a) + len(b)
            changed = (got != vol).any(axis=-1)
            assert not any(changed[z, y, x] for x, y, z in other)
            assert all((got[z, y, x] == fs.VALUE).all() for x, y, z in path)
            assert_exact(got, fs.spec_fill(vol, centre, radius, ps.SET, 0, rule, strength=fs.FULL)[0])


def test_a_seed_that_is_not_passable_fills_nothing(cases):
    vol = cases["snakes"].vol
    _, a, _ = fs.snakes()
    dims = (ps.NX, ps.NY, ps.NZ)
    # out of range with an absolute rule: a wall texel next to the corridor
    wall = next((x, y + 1, z) for x, y, z in a if vol[z, y + 1, x, 0] == fs.SNAKE_WALL)
    rule = fs.absolute_rule(wall, fs.SNAKE_LO, fs.SNAKE_HI)
    got, rep = apply(vol, *ps.BRUSHES["whole"], ps.SET, 0, rule)
    assert rep == fs.spec_region(vol, *ps.BRUSHES["whole"], rule)[2] and rep[:1] + rep[2:] == (0, dims, (-1, -1, -1))
    assert rep[1] > 0, "the passable texels are still counted"
    assert_exact(got, vol)
    # inside the clipped box and outside the ellipsoid: the box's corner
    centre, radius = (18, 11, 22), (10, 8, 12)
    corner = (8, 3, 10)
    inside, _ = ps.spec_weights(vol.shape[:3], centre, radius, 0)
    assert not inside[corner[2], corner[1], corner[0]]
    rule = fs.Rule(corner, (255, 0, 0, 0), (255, 0, 0, 0), (1, 0, 0, 0), 1)   # every byte passes
    got, rep = apply(vol, centre, radius, ps.SET, 0, rule)
    assert rep == (0, int(inside.sum()), dims, (-1, -1, -1)) == fs.spec_region(vol, centre, radius, rule)[2]
    assert_exact(got, vol)
    # outside the clipped box: the empty report, `passable` 0
    got, rep = apply(vol, centre, radius, ps.SET, 0, rule._replace(seed=(0, 0, 0)))
    assert rep == fs.empty_report(dims)
    assert_exact(got, vol)


def test_refusals_leave_the_array_untouched():
    import volumetricrenderer_amd as vr
    from volumetricrenderer_amd import _lib
    lib = _lib.load()
    vol = np.random.default_rng(5).integers(0, 256, size=(4, 4, 4, 4), dtype=np.uint8)
    keep = vol.copy()
    vp = vol.ctypes.data_as(ctypes.c_void_p)
    good_b = brush((1, 1, 1), (2, 2, 2))
    good_r = vr.make_fill_rule((1, 1, 1), 255, 255, (1, 1, 1, 1), 1)
    rep = _lib.FillReport(filled=77)
    assert lib.vr_brush_fill_apply(ctypes.byref(good_b), ctypes.byref(good_r), vp, 4, 4, 4, ctypes.byref(rep)) == 0
    assert rep.filled > 0 and (vol != keep).any()
    vol[...] = keep

    def rule(**kw):
        r = vr.make_fill_rule((1, 1, 1), 10, 20, (1, 0, 0, 0), 1)
        for k, v in kw.items():
            if k in ("relative", "reserved"):
                setattr(r, k, v)
            else:
                getattr(r, k)[:] = v
        return r

    bad = [(good_b, rule(seed=(4, 1, 1))), (good_b, rule(seed=(1, -1, 1))), (good_b, rule(seed=(1, 1, 4))),
           (good_b, rule(relative=2)), (good_b, rule(relative=-1)), (good_b, rule(select=(0, 0, 0, 0))),
           (good_b, rule(relative=0, lo=(21, 0, 0, 0))), (good_b, rule(relative=0, select=(0, 0, 1, 0), lo=(0, 0, 9, 0), hi=(0, 0, 8, 0))),
           (good_b, rule(reserved=1)),
           (brush((1, 1, 1), (2, 2, 2), op=3), good_r), (brush((1, 1, 1), (2, 256, 2)), good_r),
           (brush((1, 1, 1), (2, 2, -1)), good_r), (brush((1, 1, 1), (2, 2, 2), falloff=2), good_r)]
    for k in range(2):
        b = brush((1, 1, 1), (2, 2, 2))
        b.reserved[k] = 1
        bad.append((b, good_r))
    for b, r in bad:
        rep = _lib.FillReport(filled=77)
        assert lib.vr_brush_fill_apply(ctypes.byref(b), ctypes.byref(r), vp, 4, 4, 4, ctypes.byref(rep)) == 1   # VR_ERR_INVALID
        assert "vr_brush_fill_apply:" in lib.vr_last_error().decode()
        assert rep.filled == 77 and (vol == keep).all()
        assert lib.vr_fill(None, ctypes.byref(b), ctypes.byref(r), None, None) == 1
    # lo > hi is a refusal only where it is a range: relative distances and unselected channels are free
    assert lib.vr_brush_fill_apply(ctypes.byref(good_b), ctypes.byref(rule(lo=(21, 9, 9, 9), hi=(20, 0, 0, 0))), vp, 4, 4, 4, None) == 0
    assert lib.vr_brush_fill_apply(ctypes.byref(good_b), ctypes.byref(rule(relative=0, lo=(0, 9, 9, 9), hi=(255, 0, 0, 0))), vp, 4, 4, 4, None) == 0
    vol[...] = keep
    for dims in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
        assert lib.vr_brush_fill_apply(ctypes.byref(good_b), ctypes.byref(good_r), vp, *dims, None) == 1
    for name, args in (("vr_brush_fill_apply", (None, ctypes.byref(good_r), vp, 4, 4, 4, None)),
                       ("vr_brush_fill_apply", (ctypes.byref(good_b), None, vp, 4, 4, 4, None)),
                       ("vr_brush_fill_apply", (ctypes.byref(good_b), ctypes.byref(good_r), None, 4, 4, 4, None)),
                       ("vr_fill", (None, ctypes.byref(good_b), ctypes.byref(good_r), None, None)),
                       ("vr_fill", (ctypes.c_void_p(8), None, ctypes.byref(good_r), None, None)),
                       ("vr_fill", (ctypes.c_void_p(8), ctypes.byref(good_b), None, None, None))):
        assert getattr(lib, name)(*args) == 1, name
        msg = lib.vr_last_error().decode()
        assert name + ":" in msg and "null" in msg, msg
    assert (vol == keep).all()
    with pytest.raises(ValueError):
        vr.brush_fill_apply(good_b, good_r, np.zeros((2, 2, 2, 3), np.uint8))


def test_struct_sizes_prototypes_and_exports():
    import volumetricrenderer_amd as vr
    from volumetricrenderer_amd import _lib
    lib = _lib.load()
    assert ctypes.sizeof(_lib.FillRule) == 32 and ctypes.sizeof(_lib.FillReport) == 40 == vr.FILL_REPORT_BYTES
    assert (_lib.FillRule.relative.offset, _lib.FillRule.lo.offset, _lib.FillRule.hi.offset, _lib.FillRule.select.offset,
            _lib.FillRule.reserved.offset) == (12, 16, 20, 24, 28)
    assert (_lib.FillReport.passable.offset, _lib.FillReport.min.offset, _lib.FillReport.max.offset) == (8, 16, 28)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vr.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(vr_[a-z_0-9]+)\s*\(", src))
    for name, nargs in (("vr_fill", 5), ("vr_brush_fill_apply", 7)):
        assert name in declared and name in _lib.exported_symbols() and hasattr(lib, name), name
        m = re.search(r"vr_status\s+" + name + r"\s*\(([^)]*)\)", src)
        assert m and len(m.group(1).split(",")) == nargs == len(_lib._SIGS[name][1]), name
        assert _lib._SIGS[name][0] is ctypes.c_int
    assert re.search(r"\}\s*vr_fill_rule\s*;", src) and re.search(r"\}\s*vr_fill_report\s*;", src)
    assert lib.vr_abi_version() == 2
    assert callable(vr.Renderer.fill) and callable(vr.brush_fill_apply) and callable(vr.make_fill_rule)
    for name in ("brush_fill_apply", "make_fill_rule", "FillRule", "FillReport", "unpack_fill_report"):
        assert name in vr.__all__
    r = vr.make_fill_rule((1, 2, 3), 4, (5, 6, 7, 8))
    assert (tuple(r.seed), r.relative, tuple(r.lo), tuple(r.hi), tuple(r.select), r.reserved) == \
        ((1, 2, 3), 1, (4, 4, 4, 4), (5, 6, 7, 8), (1, 0, 0, 0), 0)
    hpp = open(os.path.join(ROOT, "include", "vr_renderer.hpp")).read()
    assert "vr_fill(" in hpp and "vr_brush_fill_apply(" in hpp
