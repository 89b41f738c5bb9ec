"""vr_rank's host side, the checks that need no GPU: the conditions the shared
inputs must meet (neighbouring ranks, the half widths, a zero-padded halo, a
separable median of medians and a `<=`-for-`<` count all give other bytes);
vr_brush_rank_apply against the numpy restatement of the rank brush
(tests/rank_spec.py) on every brush of paint_spec.BRUSHES x half width x
falloff x rank x input; the plain rank-th element; ranks 0 and N - 1 against
vr_brush_morph_apply; edge volumes; refusals; prototypes and exports."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import morph_spec as ms  # noqa: E402
import paint_spec as ps  # noqa: E402
from brush_harness import assert_exact  # noqa: E402,F401
import rank_spec as rs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUT_IDS = [n for n, _ in rs.INPUTS]


def brush(centre, radius, falloff=0, strength=rs.STRENGTH, op=0):
    import volumetricrenderer_amd as vr
    return vr.make_brush(centre, radius, op, falloff, (1, 2, 3, 4), strength)


@pytest.fixture(scope="module")
def inputs():
    return {name: make() for name, make in rs.INPUTS}


def ranks(h):
    return (rs.MEDIAN, 0, rs.window(h) - 1, 5)


def test_the_input_tells_wrong_implementations_apart(inputs):
    """Asserted before anything is compared with the library.  On the ramp (channels 0 and 3) the median differs
    from the old byte, from the ranks next to it, from a zero-padded halo, from a separable median of medians and
    from the half width before; indices 0 and N - 1 of the sorted stack are the morph's extrema."""
    base = inputs["ramp"]
    assert base.shape == (ps.NZ, ps.NY, ps.NX, 4)
    assert (rs.window(1), rs.window(2), rs.window(3)) == (27, 125, 343)
    assert [rs.resolve(rs.MEDIAN, h) for h in rs.HALF_WIDTHS] == [13, 62, 171]
    for c in (0, 3):
        ch = np.ascontiguousarray(base[..., c])
        med = {h: rs.cube_rank(ch, h, rs.MEDIAN) for h in rs.HALF_WIDTHS}
        for h, changed, beside, zero, separable in ((1, 0.9, 0.6, 0.15, 0.6), (2, 0.9, 0.2, 0.3, 0.7), (3, 0.9, 0.1, 0.4, 0.75)):
            k = rs.resolve(rs.MEDIAN, h)
            figures = ((med[h] != ch).mean(), (rs.cube_rank(ch, h, k - 1) != med[h]).mean(),
                       (rs.cube_rank(ch, h, k + 1) != med[h]).mean(),
                       (rs.cube_rank(ch, h, rs.MEDIAN, pad_mode="constant") != med[h]).mean(),
                       (rs.separable_median(ch, h) != med[h]).mean())
            print(f"channel {c} h {h}: changed {figures[0]:.3f}, rank - 1 {figures[1]:.3f}, rank + 1 {figures[2]:.3f}, "
                  f"zero halo {figures[3]:.3f}, separable {figures[4]:.3f}")
            assert figures[0] > changed, "the median is too close to the input"
            assert figures[1] > beside and figures[2] > beside, "the ranks next to the median are too close to it"
            assert figures[3] > zero, "a zero-padded halo is too close to clamping"
            assert figures[4] > separable, "a separable median is too close to the specification"
            assert (rs.cube_rank(ch, h, 0) == ms.cube_extrema(ch, h, ms.ERODE)).all()
            assert (rs.cube_rank(ch, h, rs.window(h) - 1) == ms.cube_extrema(ch, h, ms.DILATE)).all()
        assert (med[1] != med[2]).mean() > 0.67 and (med[2] != med[3]).mean() > 0.67, "the half widths are too close"


def test_the_tie_volume_tells_a_wrong_count_apart(inputs):
    """Four distinct bytes, both extremes among them; nearly every window is full of ties; results 255 and the
    candidate 1 occur; a bisection counting `<=` instead of `<` differs from the specification."""
    ties = inputs["ties"]
    assert sorted(np.unique(ties).tolist()) == [0, 1, 128, 255]
    ch = np.ascontiguousarray(ties[..., 0])
    for h in rs.HALF_WIDTHS:
        srt = rs.cube_sorted(ch, h)
        assert ((srt[..., 1:] == srt[..., :-1]).sum(axis=-1) >= rs.window(h) - 4).all(), "a window without ties"
        got = {r: rs.cube_rank(ch, h, r) for r in ranks(h)}
        assert (got[rs.window(h) - 1] == 255).any() and (got[0] == 0).any()
        assert any((g == 1).any() for g in got.values()), "no result is 1: the candidate 1 is never kept"
        wrong = rs.wrong_rule_rank(ch, h, rs.MEDIAN)
        assert (wrong != got[rs.MEDIAN]).mean() > 0.5, "the wrong rule is too close to the specification"


@pytest.mark.parametrize("iname", INPUT_IDS)
@pytest.mark.parametrize("falloff,fname", ps.FALLOFFS, ids=[n for _, n in ps.FALLOFFS])
@pytest.mark.parametrize("h", rs.HALF_WIDTHS)
@pytest.mark.parametrize("name", list(ps.BRUSHES))
def test_rank_apply_matches_the_numpy_restatement(inputs, name, h, falloff, fname, iname):
    import volumetricrenderer_amd as vr
    base = inputs[iname]
    centre, radius = ps.BRUSHES[name]
    inside, _ = ps.spec_weights(base.shape[:3], centre, radius, falloff)
    for rank in ranks(h):
        want = rs.spec_rank(base, centre, radius, rank, h, falloff)
        got = vr.brush_rank_apply(brush(centre, radius, falloff), rank, h, base.copy())
        assert_exact(got, want)
        # the conditions on the inputs: a weaker input must not hide a failure
        assert (want[..., 3] == base[..., 3]).all(), "channel A has strength 0"
        assert (want[~inside] == base[~inside]).all()
        if name == "miss":
            assert not inside.any() and (want == base).all()
        elif name != "texel":   # one texel may hold its own rank-th byte
            assert (want != base).any(), "no byte changed where the brush hits"
    if name in ("corner", "far_corner"):
        assert (ms.clamped_axes(base.shape[:3], centre, radius, h) == 3).any(), "no cube clamped on three axes"


@pytest.mark.parametrize("iname", INPUT_IDS)
def test_a_whole_volume_rank_is_the_rank_th_element(inputs, iname):
    """`whole`, hard edge, full strength: every byte becomes the rank-th element of its cube (the Jacobi result);
    the ranks are ordered; 0 and N - 1 are what vr_brush_morph_apply leaves."""
    import volumetricrenderer_amd as vr
    base = inputs[iname]
    centre, radius = ps.BRUSHES["whole"]
    inside, _ = ps.spec_weights(base.shape[:3], centre, radius, 0)
    assert inside.all()
    for h in rs.HALF_WIDTHS:
        got = {}
        for rank in ranks(h):
            want = np.stack([rs.cube_rank(np.ascontiguousarray(base[..., c]), h, rank) for c in range(4)], axis=-1).astype(np.uint8)
            got[rank] = vr.brush_rank_apply(brush(centre, radius, 0, rs.FULL), rank, h, base.copy())
            assert_exact(got[rank], want)
        last = rs.window(h) - 1
        assert (got[0] <= got[5]).all() and (got[5] <= got[rs.MEDIAN]).all() and (got[rs.MEDIAN] <= got[last]).all()
        assert (got[0] <= base).all() and (base <= got[last]).all()
        assert_exact(vr.brush_rank_apply(brush(centre, radius, 0, rs.FULL), rs.resolve(rs.MEDIAN, h), h, base.copy()), got[rs.MEDIAN])


@pytest.mark.parametrize("iname", INPUT_IDS)
@pytest.mark.parametrize("falloff,fname", ps.FALLOFFS, ids=[n for _, n in ps.FALLOFFS])
def test_first_and_last_rank_are_erode_and_dilate(inputs, iname, falloff, fname):
    import volumetricrenderer_amd as vr
    base = inputs[iname]
    for name in ("straddle", "corner", "max"):
        centre, radius = ps.BRUSHES[name]
        b = brush(centre, radius, falloff)
        for h in rs.HALF_WIDTHS:
            for rank, op in ((0, ms.ERODE), (rs.window(h) - 1, ms.DILATE)):
                want = vr.brush_morph_apply(b, op, h, base.copy())
                assert (want != base).any()
                assert_exact(vr.brush_rank_apply(b, rank, h, base.copy()), want)


def test_edge_volumes():
    import volumetricrenderer_amd as vr
    one = np.array([[[[9, 200, 0, 255]]]], np.uint8)
    rng = np.random.default_rng(11)
    thin = rng.integers(0, 256, size=(1, 3, 2, 4), dtype=np.uint8)   # 2 x 3 x 1: thinner than any window
    line = rng.integers(0, 256, size=(1, 1, 5, 4), dtype=np.uint8)   # 5 x 1 x 1
    vol = rng.integers(0, 256, size=(9, 7, 12, 4), dtype=np.uint8)
    vol[..., 1] = 77                                                 # a constant channel stays constant
    for h in rs.HALF_WIDTHS:
        for rank in ranks(h) + (1, rs.window(h) - 2):
            for falloff in (0, 1):
                got = vr.brush_rank_apply(brush((0, 0, 0), (255, 255, 255), falloff, rs.FULL), rank, h, one.copy())
                assert_exact(got, one)   # every neighbour is the texel itself
                assert_exact(rs.spec_rank(one, (0, 0, 0), (255, 255, 255), rank, h, falloff, rs.FULL), one)
            for small, centre in ((thin, (1, 1, 0)), (line, (2, 0, 0))):
                want = rs.spec_rank(small, centre, (4, 4, 4), rank, h, 1, rs.FULL)
                assert (want != small).any()
                assert_exact(vr.brush_rank_apply(brush(centre, (4, 4, 4), 1, rs.FULL), rank, h, small.copy()), want)
            got = vr.brush_rank_apply(brush((5, 3, 4), (6, 6, 6), 1, rs.FULL), rank, h, vol.copy())
            assert (got[..., 1] == 77).all()
            assert (got[..., 0] != vol[..., 0]).any()
            assert_exact(got, rs.spec_rank(vol, (5, 3, 4), (6, 6, 6), rank, h, 1, rs.FULL))
    with pytest.raises(ValueError):
        vr.brush_rank_apply(brush((0, 0, 0), (1, 1, 1)), 0, 1, np.zeros((2, 2, 2, 3), np.uint8))


def test_refusals_leave_the_array_untouched():
    from volumetricrenderer_amd import _lib
    lib = _lib.load()
    vol = np.random.default_rng(5).integers(0, 256, size=(4, 4, 4, 4), dtype=np.uint8)
    keep = vol.copy()
    vp = vol.ctypes.data_as(ctypes.c_void_p)
    good = brush((1, 1, 1), (2, 2, 2))
    for rank, h in ((-1, 1), (0, 1), (26, 1), (124, 2), (342, 3), (-1, 3)):
        assert lib.vr_brush_rank_apply(ctypes.byref(good), rank, h, vp, 4, 4, 4) == 0, (rank, h)
        assert (vol != keep).any()
        vol[...] = keep
    bad = [(brush((1, 1, 1), (2, 2, 2), op=1), 0, 1), (brush((1, 1, 1), (2, 2, 2), op=2), -1, 1),
           (brush((1, 1, 1), (2, 2, 2), op=3), 0, 1),
           (good, 27, 1), (good, 125, 2), (good, 343, 3), (good, -2, 1), (good, 2**31 - 1, 1), (good, -2**31, 3),
           (good, 0, 0), (good, 1, 4), (good, -1, -1), (good, -1, 0), (good, 1, 2**31 - 1), (good, 0, -2**31),
           (brush((1, 1, 1), (2, -1, 2)), 0, 1), (brush((1, 1, 1), (256, 2, 2)), -1, 1),
           (brush((1, 1, 1), (2, 2, 2), falloff=2), 0, 1)]
    for k in range(2):
        b = brush((1, 1, 1), (2, 2, 2))
        b.reserved[k] = 1
        bad.append((b, k, 1))
    for b, rank, h in bad:
        assert lib.vr_brush_rank_apply(ctypes.byref(b), rank, h, vp, 4, 4, 4) == 1, (b.op, rank, h)   # VR_ERR_INVALID
        assert "vr_brush_rank_apply:" in lib.vr_last_error().decode()
        assert lib.vr_rank(None, ctypes.byref(b), rank, h, None) == 1
        assert (vol == keep).all()
    for dims in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
        assert lib.vr_brush_rank_apply(ctypes.byref(good), 0, 1, vp, *dims) == 1
    for name, args in (("vr_brush_rank_apply", (None, 0, 1, vp, 4, 4, 4)),
                       ("vr_brush_rank_apply", (ctypes.byref(good), 0, 1, None, 4, 4, 4)),
                       ("vr_rank", (None, ctypes.byref(good), 0, 1, None)),
                       ("vr_rank", (ctypes.c_void_p(8), None, 0, 1, None))):
        assert getattr(lib, name)(*args) == 1, name
        msg = lib.vr_last_error().decode()
        assert name + ":" in msg and "null" in msg, msg
    assert (vol == keep).all()


def test_prototypes_exports_and_signatures():
    import volumetricrenderer_amd as vr
    from volumetricrenderer_amd import _lib
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vr.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(vr_[a-z_0-9]+)\s*\(", src))
    for name, nargs in (("vr_rank", 5), ("vr_brush_rank_apply", 7)):
        assert name in declared and name in _lib.exported_symbols() and hasattr(lib, name), name
        m = re.search(r"vr_status\s+" + name + r"\s*\(([^)]*)\)", src)
        assert m and len(m.group(1).split(",")) == nargs == len(_lib._SIGS[name][1]), name
        assert _lib._SIGS[name][0] is ctypes.c_int
    assert re.search(r"#define\s+VR_RANK_MAX_HALF\s+3\b", src) and vr.RANK_MAX_HALF == 3
    assert re.search(r"#define\s+VR_RANK_MEDIAN\s+\(-1\)", src) and vr.RANK_MEDIAN == -1
    assert lib.vr_abi_version() == 2
    assert callable(vr.Renderer.rank) and callable(vr.brush_rank_apply)
    for name in ("brush_rank_apply", "RANK_MEDIAN", "RANK_MAX_HALF"):
        assert name in vr.__all__
    hpp = open(os.path.join(ROOT, "include", "vr_renderer.hpp")).read()
    assert "vr_rank(" in hpp and "vr_brush_rank_apply(" in hpp
